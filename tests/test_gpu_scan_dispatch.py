"""Every branch of QueryBuild::scan_dispatch that a PRE-BUILT kernel answers (viyadb_amd/csrc/vhh_launch.h, the launchers of vh_launch.h),
and the tails behind a partitioned scan: one query each, all under PLAN_NO_JIT, on C3Host(3, 5000, 8192) with predpack([D2, D3, D4],
sliced=True) — two full 2048-row chunks, one of 904 rows and a last plane word of 8 rows, as in tests/test_gpu_agg_sliced.py — and, for the
aggregate on the planes, a second projection of (d2, m0, count) as in tests/test_gpu_plane_agg.py.

Per branch: the result equals the oracle (tests/parity.compare) and vh_result_kernel is the literal of KERNELS below. The launcher that
instantiates a kernel writes its name, so the literals pin the template arguments that are launched: mode, block size, memory scope (3 = workgroup:
a private copy per XCD, 4 = agent), and the number of predicate columns NP — the filters have one, two and three of them (F1, F2, F3).
The literals were recorded by running these queries on the commit BEFORE the launchers named their kernels (where a separate chain of
snprintf in decompose_work derived the names), not on the code under test.

Two levels of DENSE_PART need more than 64 LDS-sized ranges. GROUP BY (d0, d2) has 4000 group ids, the most a dense plan of 15 000 rows
reaches with C3's columns besides (d0, d1)'s 100 000 (beyond the dense limit of 4 x rows: the hash path), so VH_PART_TABLE_KB shrinks the
ranges: 1 KB makes 125 ranges of 32 groups for three-word tuples (21 bytes of states per group), the unit-step split; two-word tuples have at
most 16 bytes of states per group and 1 KB still holds 64 groups (63 ranges, one level), so their case runs with 0 KB: a group per range.
Not reachable here: part_split_ring_kernel<256, 4> and <256, 8> split ONE-word tuples (VhPlanDev::gid_bits), which only a compiled scan
writes — never under PLAN_NO_JIT."""
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare
from tests.test_gpu_agg_sliced import AND, METRIC, REL
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
ROWS, CAP = 5000, 8192
F1 = AND(REL(D3, "lt", 447))
F2 = AND(REL(D3, "lt", 447), REL(D4, "ge", 553))
F3 = AND(REL(D2, "eq", 1), REL(D3, "lt", 447), REL(D4, "ge", 553))
SUM_COUNT = ("m0", "count")
NO_FAST, NO_LANES, LANES, SLICED = capi.PLAN_NO_FAST, capi.PLAN_NO_LANES, capi.PLAN_FORCE_LANES, capi.PLAN_SLICED_PREBUILT | capi.PLAN_NO_LANES
GLOBAL, ONE_COPY, HASH, PART, NO_SHAPE = capi.PLAN_FORCE_GLOBAL, capi.PLAN_NO_XCD_PRIVATE, capi.PLAN_FORCE_HASH, capi.PLAN_FORCE_PART, capi.PLAN_NO_SHAPE
BY_D2, BY_D0_D2 = (D2,), (0, D2)
PART_AGG = " + part_agg_kernel<1024>"

# id: (filter, dimensions, metrics, flags (| PLAN_NO_JIT), flags2, VH_PART_TABLE_KB or None, path)
CASES = {
    "generic_lds":             (F3, BY_D2, SUM_COUNT, NO_FAST, 0, None, "dense_lds"),
    "generic_global_private":  (F2, BY_D2, SUM_COUNT, NO_FAST | GLOBAL, 0, None, "dense_global"),
    "generic_global_one_copy": (F1, BY_D2, SUM_COUNT, NO_FAST | GLOBAL | ONE_COPY, 0, None, "dense_global"),
    "generic_hash":            (F3, BY_D2, SUM_COUNT, NO_FAST | HASH, 0, None, "hash"),
    "fast_lds":                (F3, BY_D2, SUM_COUNT, NO_LANES, 0, None, "dense_lds"),
    "fast_lds_one_copy":       (F1, BY_D2, SUM_COUNT, NO_LANES | ONE_COPY, 0, None, "dense_lds"),
    "fast_global_private":     (F1, BY_D2, SUM_COUNT, NO_LANES | GLOBAL, 0, None, "dense_global"),
    "fast_global_one_copy":    (F2, BY_D2, SUM_COUNT, NO_LANES | GLOBAL | ONE_COPY, 0, None, "dense_global"),
    "fast_hash":               (F3, BY_D2, SUM_COUNT, NO_LANES | HASH, 0, None, "hash"),
    "fast_part_shape":         (F3, BY_D0_D2, SUM_COUNT, NO_LANES | PART, 0, None, "dense_part"),
    "fast_part_no_shape":      (F2, BY_D0_D2, SUM_COUNT, NO_LANES | PART | NO_SHAPE, 0, None, "dense_part"),
    "lanes_lds":               (F1, BY_D2, SUM_COUNT, LANES, 0, None, "dense_lds"),
    "lanes_lds_one_copy":      (F3, BY_D2, SUM_COUNT, LANES | ONE_COPY, 0, None, "dense_lds"),
    "lanes_hash":              (F2, BY_D2, SUM_COUNT, LANES | HASH, 0, None, "hash"),
    "lanes_part":              (F3, BY_D0_D2, SUM_COUNT, LANES | PART, 0, None, "dense_part"),
    "sliced_lds":              (F3, BY_D2, SUM_COUNT, SLICED, 0, None, "dense_lds"),
    "sliced_global":           (F2, BY_D2, SUM_COUNT, SLICED | GLOBAL, 0, None, "dense_global"),
    "sliced_hash":             (F1, BY_D2, SUM_COUNT, SLICED | HASH, 0, None, "hash"),
    "sliced_part":             (F3, BY_D0_D2, SUM_COUNT, SLICED | PART, 0, None, "dense_part"),
    "plane_agg":               (F3, BY_D2, SUM_COUNT, 0, capi.PLAN2_PLANE_AGG, None, "dense_lds"),
    "plane_agg_one_copy":      (F1, BY_D2, SUM_COUNT, ONE_COPY, capi.PLAN2_PLANE_AGG, None, "dense_lds"),
    "two_level_ring_split":    (F3, BY_D0_D2, SUM_COUNT, NO_LANES | PART, 0, 0, "dense_part"),
    "two_level_split":         (F2, BY_D0_D2, ("m0", "m1", "m4"), NO_LANES | PART, 0, 1, "dense_part"),
}

# vh_result_kernel of every case, as the commit before this test's printed it
KERNELS = {
    "generic_lds":             "scan_agg_kernel<1, 1024, 3>",
    "generic_global_private":  "scan_agg_kernel<2, 256, 3>",
    "generic_global_one_copy": "scan_agg_kernel<2, 256, 4>",
    "generic_hash":            "scan_agg_kernel<3, 256, 4>",
    "fast_lds":                "scan_agg_fast_kernel<1, 1024, 3, 3>",
    "fast_lds_one_copy":       "scan_agg_fast_kernel<1, 1024, 4, 1>",
    "fast_global_private":     "scan_agg_fast_kernel<2, 256, 3, 1>",
    "fast_global_one_copy":    "scan_agg_fast_kernel<2, 256, 4, 2>",
    "fast_hash":               "scan_agg_fast_kernel<3, 256, 4, 3>",
    "fast_part_shape":         "scan_agg_shape_kernel<4, 256, 4, 3, 1>" + PART_AGG,
    "fast_part_no_shape":      "scan_agg_fast_kernel<4, 256, 4, 2>" + PART_AGG,
    "lanes_lds":               "scan_agg_lanes_kernel<1, 1024, 3, 1>",
    "lanes_lds_one_copy":      "scan_agg_lanes_kernel<1, 1024, 4, 3>",
    "lanes_hash":              "scan_agg_lanes_kernel<3, 256, 4, 2>",
    "lanes_part":              "scan_agg_lanes_kernel<4, 256, 4, 3>" + PART_AGG,
    "sliced_lds":              "scan_agg_sliced_kernel<1, 1024, 3>",
    "sliced_global":           "scan_agg_sliced_kernel<2, 256, 3>",
    "sliced_hash":             "scan_agg_sliced_kernel<3, 256, 4>",
    "sliced_part":             "scan_agg_sliced_kernel<4, 256, 4>" + PART_AGG,
    "plane_agg":               "scan_agg_planes_kernel<256, 3>",
    "plane_agg_one_copy":      "scan_agg_planes_kernel<256, 4>",
    "two_level_ring_split":    "scan_agg_shape_kernel<4, 256, 4, 3, 1> + part_split_ring_kernel<256, 16>" + PART_AGG,
    "two_level_split":         "scan_agg_fast_kernel<4, 256, 4, 2> + part_split_kernel<256>" + PART_AGG,
}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def shared():
    h = C3Host(3, ROWS, CAP)
    h.dt.predpack([D2, D3, D4], sliced=True)
    h.dt.predpack([D2, METRIC["m0"], METRIC["count"]], sliced=True)      # the aggregate on the planes reads group and metric columns off a projection too
    yield h
    h.close()


_WANT = {}


def oracle(h, filt, dims, metrics):
    """The oracle's answer, computed once per query and shared by the branches that run it."""
    key = (repr(filt[1]), dims, metrics)
    if key not in _WANT:
        q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics), "filter": filt[1]}
        _WANT[key] = vo.scan_aggregate(vo.parse_query(h.tab, q))
    return _WANT[key]


def run_case(h, name, setenv):
    filt, dims, metrics, flags, flags2, table_kb, path = CASES[name]
    if table_kb is not None:
        setenv("VH_PART_TABLE_KB", str(table_kb))
    res = h.dt.query_agg(AggPlan(filter=filt[0], groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics],
                                 flags=capi.PLAN_NO_JIT | flags, flags2=flags2))
    print(f"{name}: path {res.path}, flags {res.flags:#x}, passed {res.passed_recs}, groups {res.ngroups}, kernel {res.kernel!r}")
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_branch(shared, monkeypatch, name):
    filt, dims, metrics, _, _, _, path = CASES[name]
    res = run_case(shared, name, monkeypatch.setenv)
    compare(res, oracle(shared, filt, dims, metrics), name)
    assert 0 < res.passed_recs < res.scanned_recs, name
    assert not res.jit and res.path == path, (name, res.path, hex(res.flags))
    assert res.kernel == KERNELS[name], (name, res.kernel)


def test_every_np_is_named():
    """The cases cover NP = 1, 2 and 3 in the names of the kernels that carry it."""
    for stem in ("scan_agg_fast_kernel<", "scan_agg_lanes_kernel<"):
        nps = {k.split(" + ")[0].rstrip(">").split(", ")[3] for k in KERNELS.values() if k.startswith(stem)}
        assert nps == {"1", "2", "3"}, (stem, nps)
