"""Aggregates on the bit-sliced predicate planes through the PRE-BUILT scan (scan_agg_sliced_kernel over viyadb_amd/csrc/vh_bits_eval.h and
vh_sliced_walk.h; opt-in: VH_PLAN_SLICED_PREBUILT, or VH_SLICED_PREBUILT=1 for a process). Tables are C3Host(3, 5000, 8192) with
predpack([D2, D3, D4], sliced=True): 5000 rows are two full 2048-row chunks and one of 904, and the last plane word holds 8 rows.

Every case runs its plan with PLAN_SLICED_PREBUILT | PLAN_NO_JIT | PLAN_NO_LANES and its twin without PLAN_SLICED_PREBUILT — the path such a
query takes today — and asserts: both equal the oracle over the host's current arrays (tests/parity.compare: groups, ngroups, scanned_recs,
scanned_segments, passed_recs); the two agree with each other, integer and MIN / MAX states bit for bit, double sums within 1e-9 relative
(the summation order differs); vh_result_info.reserved bit 26 is set exactly where the planner's rule says, with bits 4 / 11 / 13 and without
bits 0 / 1 / 5, and the kernel is then scan_agg_sliced_kernel<..>; the twin has bit 26 clear and names another kernel; `path` is the same.
The partitioned dense organisation is reached by GROUP BY (d0, d2) under VH_PLAN_FORCE_PART: at 15 000 rows (d0, d1) has more group ids than
the planner's dense limit (4 x rows) and takes the hash path whatever the flag.
Nothing here is compiled at run time: the file runs under VH_JIT=off too.

C3's schema has no AVG metric, so "AVG without COUNT" has no case here. The oracle knows no row-id metric: the search query's positions are
held against the host arrays, its counters against the oracle's COUNT of the same query."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare, sort_rows
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, CAP = 5000, 8192
ID = 6                                           # C3's row-id column: in no projection
METRIC = {"m0": 7, "m1": 8, "count": 9, "m3": 10, "m4": 11}
PREBUILT = capi.PLAN_SLICED_PREBUILT
BASE = capi.PLAN_NO_JIT | capi.PLAN_NO_LANES
BIT26 = capi.INFO_SLICED_PREBUILT
ON_PLANES = capi.INFO_ON_PLANES      # vh_result_info.reserved: narrowed, a predicate projection, its bit-sliced form
OFF = capi.INFO_FAST | capi.INFO_LANES | capi.INFO_JIT      # a register-resident kernel, its lanes form, a compiled kernel
SETS = capi.INFO_INSET | capi.INFO_INSET_SLICED
OPS = [("eq", capi.OP_EQ), ("ne", capi.OP_NE), ("lt", capi.OP_LT), ("le", capi.OP_LE), ("gt", capi.OP_GT), ("ge", capi.OP_GE)]
SUM_COUNT = ("m0", "count")
# The partitioned dense organisation at this size: GROUP BY (d0, d2) is 4000 group ids — beyond an LDS table (52 KB of states) and within the
# dense limit of 4 x 15 000 rows. (d0, d1) is 100 000 ids, beyond that limit: the hash path, with or without VH_PLAN_FORCE_PART.
PART = ((0, D2), capi.PLAN_FORCE_PART, 0)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _host():
    h = C3Host(3, ROWS, CAP)
    h.dt.predpack([D2, D3, D4], sliced=True)
    return h


@pytest.fixture(scope="module")
def shared():
    """One table for the cases that change nothing."""
    h = _host()
    yield h
    h.close()


@pytest.fixture
def host():
    h = _host()
    yield h
    h.close()


def REL(col, name, v):
    return ("rel", col, dict(OPS)[name], v), {"op": name, "column": "id" if col == ID else f"d{col}", "value": str(v)}


def SET(col, values, equal=True, kind="in"):
    f = {"op": "in", "column": f"d{col}", "values": [str(v) for v in values]}
    return (kind, col, equal, [int(v) for v in values]), f if equal else {"op": "not", "filter": f}


def AND(*leaves):
    return [l[0] for l in leaves] + [("and", len(leaves))], {"op": "and", "filters": [l[1] for l in leaves]}


def OR(*leaves):
    return [l[0] for l in leaves] + [("or", len(leaves))], {"op": "or", "filters": [l[1] for l in leaves]}


C3 = AND(REL(D2, "eq", 1), REL(D3, "lt", 447), REL(D4, "ge", 553))
EVERY_ROW = AND(REL(D3, "ne", 1023))             # d3 holds 0 .. 999


def c3_mask(seg, rows):
    d = seg["d"]
    return (d[D2][:rows] == 1) & (d[D3][:rows] < 447) & (d[D4][:rows] >= 553)


def agree(a, b, label):
    """The two runs: integer and MIN / MAX states bit for bit, double sums within 1e-9 relative."""
    assert (a.ngroups, a.passed_recs, a.scanned_recs, a.scanned_segments) == (b.ngroups, b.passed_recs, b.scanned_recs, b.scanned_segments), label
    pa, pb = sort_rows(a.keys, a.states), sort_rows(b.keys, b.states)
    for x, y in zip(a.keys + a.states, b.keys + b.states):
        assert x.dtype == y.dtype and len(x) == len(y), label
        if x.dtype.kind == "f":
            np.testing.assert_allclose(x[pa], y[pb], rtol=1e-9, atol=0, err_msg=label)
        else:
            assert np.array_equal(x[pa], y[pb]), label


def both(h, filt, dims=(D2,), metrics=SUM_COUNT, flags=0, seg_rows=None, on=True, path=None, sets=False, hint=0, label=""):
    """The plan with PLAN_SLICED_PREBUILT and its twin without: each against the oracle, against each other, and the path each took.
    on: the rule says the pre-built scan over the planes answers the flagged run. -> the flagged run."""
    nodes, qfilter = filt
    q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics)}
    if qfilter is not None:
        q["filter"] = qfilter
    want = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    label = f"{label} by={list(dims)} metrics={list(metrics)} flags={flags:#x} snapshot={seg_rows}"

    def run(fl):
        return h.dt.query_agg(AggPlan(filter=nodes, groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics],
                                      flags=BASE | flags | fl, groups_hint=hint, seg_rows=seg_rows))
    a, b = run(PREBUILT), run(0)
    print(f"{label}: path {a.path} / {b.path}, flags {a.flags:#x} / {b.flags:#x}, passed {a.passed_recs}, groups {a.ngroups}, kernel {a.kernel} / {b.kernel}")
    compare(a, want, label + " [pre-built on the planes]")
    compare(b, want, label + " [twin]")
    agree(a, b, label)
    assert a.path == b.path and (path is None or a.path == path), (label, a.path, b.path, path)
    expect_flags(a, b, on, sets, label)
    return a


def expect_flags(a, b, on, sets, label):
    assert bool(a.flags & BIT26) == on and a.sliced_prebuilt == on, (label, hex(a.flags), a.kernel)
    assert not a.flags & capi.INFO_JIT and not a.jit, (label, hex(a.flags))
    if on:
        assert a.flags & ON_PLANES == ON_PLANES and not a.flags & OFF, (label, hex(a.flags))
        assert a.kernel.startswith("scan_agg_sliced_kernel<"), (label, a.kernel)
        assert a.flags & SETS == (SETS if sets else 0), (label, hex(a.flags))
    else:
        assert "scan_agg_sliced_kernel" not in a.kernel, (label, a.kernel)
        assert a.flags == b.flags and a.kernel == b.kernel, (label, hex(a.flags), hex(b.flags), a.kernel, b.kernel)      # the flag changed nothing
    assert not b.flags & BIT26 and not b.sliced_prebuilt and "scan_agg_sliced_kernel" not in b.kernel, (label, hex(b.flags), b.kernel)


# ---- 1. every organisation on C3's filter (fails without the feature: no such flag, no such kernel, bit 26 never set)
@pytest.mark.parametrize("dims, flags, path, hint", [
    ((D2,), 0, "dense_lds", 0),
    ((D2,), capi.PLAN_FORCE_GLOBAL, "dense_global", 0),
    ((D2,), capi.PLAN_FORCE_GLOBAL | capi.PLAN_NO_XCD_PRIVATE, "dense_global", 0),
    ((D2,), capi.PLAN_FORCE_HASH, "hash", 0),
    ((D2,), capi.PLAN_FORCE_HASH | capi.PLAN_NO_LDS_HASH, "hash", 0),
    ((0, 1), 0, "hash", 100_000),
    ((0, D2), capi.PLAN_FORCE_PART, "dense_part", 0),
    ((0, D2), capi.PLAN_FORCE_PART | capi.PLAN_NO_SHAPE, "dense_part", 0),
    ((), 0, "scalar", 0),
], ids=["lds", "global", "global_one_copy", "hash", "hash_no_lds_table", "d0_d1_as_planned", "part", "part_generic_drain", "scalar"])
def test_organisations(shared, dims, flags, path, hint):
    a = both(shared, C3, dims=dims, flags=flags, path=path, hint=hint, label="C3")
    assert 0 < a.passed_recs < a.scanned_recs
    if path == "dense_part":
        assert a.kernel.endswith("part_agg_kernel<1024>"), a.kernel      # (the tail behind the scan is unchanged)


# ---- 2. metric kinds through the generic sink (LDS table and hash table) and the search query's row positions
@pytest.mark.parametrize("metrics", [("m0", "count"), ("m1",), ("m4",), ("m3",), ("m0", "m1", "count", "m3", "m4")],
                         ids=["sum_count", "max_i64", "min_u32", "sum_f64", "all_five"])
def test_metrics(shared, metrics):
    for flags in (0, capi.PLAN_FORCE_HASH):
        both(shared, C3, metrics=metrics, flags=flags, label="C3")


def test_row_positions(shared):
    """VH_COL_ROWID alone: MIN (segment << 32 | row) of the passing rows by d2."""
    h = shared
    nodes, qfilter = AND(REL(D3, "lt", 447), REL(D4, "ge", 553))
    q = {"type": "aggregate", "table": "synth", "dimensions": ["d2"], "metrics": ["count"], "filter": qfilter}
    want = vo.scan_aggregate(vo.parse_query(h.tab, q))
    first = {}
    for s, seg in enumerate(h.tab.segments):
        d = seg["d"]
        m = (d[D3][:ROWS] < 447) & (d[D4][:ROWS] >= 553)
        for v in np.unique(d[D2][:ROWS][m]):
            first.setdefault(int(v), (s << 32) | int(np.nonzero(m & (d[D2][:ROWS] == v))[0][0]))
    for flags in (0, capi.PLAN_FORCE_HASH):
        runs = [h.dt.query_agg(AggPlan(filter=nodes, groups=[GroupSpec(D2)], metrics=[capi.COL_ROWID], flags=BASE | flags | fl)) for fl in (PREBUILT, 0)]
        for r in runs:
            assert (r.ngroups, r.passed_recs, r.scanned_recs, r.scanned_segments) == (want.ngroups, want.passed_recs, want.scanned_recs, want.scanned_segments)
            assert dict(zip(r.keys[0].tolist(), [int(x) for x in r.states[0]])) == first, hex(r.flags)
        agree(runs[0], runs[1], "row positions")
        assert runs[0].path == runs[1].path
        expect_flags(runs[0], runs[1], True, False, f"row positions flags={flags:#x}")


# ---- 3. queue pressure: 2048 survivors a step, none at all, and more than 64 in a chunk of C3's own
def test_queue_pressure(shared):
    h = shared
    for dims, flags, hint in (((D2,), 0, 0), ((0, 1), 0, 100_000), PART):
        a = both(h, EVERY_ROW, dims=dims, flags=flags, hint=hint, label="every row passes")
        assert a.passed_recs == a.scanned_recs == 3 * ROWS
        z = both(h, AND(REL(D3, "lt", 447), REL(D3, "ge", 447)), dims=dims, flags=flags, hint=hint, label="no row passes")
        assert z.passed_recs == 0 and z.ngroups == 0 and z.scanned_segments == 3      # (each leaf alone lies within every segment's min / max: the segments are scanned)
    per_chunk = [int(c3_mask(seg, ROWS)[k:k + 2048].sum()) for seg in h.tab.segments for k in range(0, ROWS, 2048)]
    assert max(per_chunk) > 64, per_chunk         # the drain inside a step runs for C3's own filter


# ---- 4. snapshots of the middle segment: nothing at or beyond seg_rows passes, the word that straddles it is masked
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2047, 2048, 2049, 4999])
def test_snapshots(shared, n):
    snap = [ROWS, n, ROWS]
    both(shared, C3, seg_rows=snap, label="C3")
    a = both(shared, EVERY_ROW, seg_rows=snap, label="every row passes")      # (the planes' bits beyond the snapshot are those of real rows)
    assert a.passed_recs == 2 * ROWS + n
    a = both(shared, EVERY_ROW, dims=PART[0], flags=PART[1], seg_rows=snap, path="dense_part", label="every row passes")


# ---- 5. filter forms
def test_relations(shared):
    some = none = 0
    for name, _ in OPS:
        for lit in (0, 446, 447, 999, 1000, 1024, 2 ** 40):
            a = both(shared, AND(REL(D3, name, lit)), label=f"d3 {name} {lit}")
            some += a.passed_recs > 0
            none += a.passed_recs == 0
    assert some and none


def test_in_lists_sets_and_the_stack(shared):
    held = np.unique(np.concatenate([seg["d"][D4][:ROWS] for seg in shared.tab.segments]))
    for n in (1, 2, 8):
        values = [int(v) for v in held[:: max(1, len(held) // n)][:n]]
        for equal in (True, False):
            a = both(shared, AND(SET(D4, values, equal)), label=f"d4 {'IN' if equal else 'NOT IN'} {values}")
            assert 0 < a.passed_recs < a.scanned_recs
    for equal in (True, False):
        a = both(shared, AND(SET(D2, [1, 3], equal, kind="inset"), REL(D3, "lt", 447)), sets=True, label=f"a set leaf on d2 (2-bit field), {'IN' if equal else 'NOT IN'}")
        assert 0 < a.passed_recs < a.scanned_recs
    x, y = AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), AND(REL(D2, "eq", 2), REL(D4, "ge", 553))
    a = both(shared, (x[0] + y[0] + [("or", 2)], {"op": "or", "filters": [x[1], y[1]]}), label="(d2 == 1 & d3 < 447) | (d2 == 2 & d4 >= 553)")
    assert 0 < a.passed_recs < a.scanned_recs


# ---- 6. where the rule says no: the flag is set, bit 26 is clear, nothing else differs from the twin, and the result is right
def test_where_the_rule_says_no(shared):
    h = shared
    both(h, AND(REL(D2, "eq", 1), REL(ID, "lt", 9000)), on=False, label="a leaf on id")
    both(h, ([], None), on=False, label="no filter")
    for flag in (capi.PLAN_NO_SLICED, capi.PLAN_NO_PREDPACK, capi.PLAN_NO_NARROW):
        both(h, C3, flags=flag, on=False, label="C3")
    long_or = OR(*[REL(D3, "eq", v) for v in range(100, 130)])           # 30 leaves, folded pairwise: 59 nodes, beyond the inline program
    a = both(h, long_or, on=False, label="an OR of 30 comparisons")
    assert 0 < a.passed_recs < a.scanned_recs
    # a plan that takes a no-compaction (lanes) form keeps it
    nodes = C3[0]
    runs = [h.dt.query_agg(AggPlan(filter=nodes, groups=[GroupSpec(D2)], metrics=[METRIC["m0"], METRIC["count"]],
                                   flags=capi.PLAN_NO_JIT | capi.PLAN_FORCE_LANES | fl)) for fl in (PREBUILT, 0)]
    want = vo.scan_aggregate(vo.parse_query(h.tab, {"type": "aggregate", "table": "synth", "dimensions": ["d2"], "metrics": ["m0", "count"], "filter": C3[1]}))
    for r in runs:
        compare(r, want, "C3 by d2, PLAN_FORCE_LANES")
        assert r.lanes and r.kernel.startswith("scan_agg_lanes_kernel<"), (hex(r.flags), r.kernel)
    agree(runs[0], runs[1], "lanes")
    expect_flags(runs[0], runs[1], False, False, "C3 by d2, PLAN_FORCE_LANES")


def test_no_sliced_projection():
    h = C3Host(3, ROWS, CAP)
    try:
        both(h, C3, on=False, label="C3, no projection")
        assert not [x for x in h.dt.layouts()[0] if x.kind in (capi.LAYOUT_PRED_BYTES, capi.LAYOUT_PRED_SLICED)]      # ... and the query built none
        h.dt.predpack([D2, D3, D4], sliced=False)          # byte planes are not what this kernel reads
        both(h, C3, on=False, label="C3, byte planes only")
        h.dt.predpack([D2, D3], sliced=True)               # a bit-sliced projection that lacks one of the filter's columns
        both(h, C3, on=False, label="C3, planes of d2 and d3 only")
        both(h, AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), label="d2 and d3 alone")
    finally:
        h.close()


# ---- 7. after syncs: the planes followed the journal, an append crosses a chunk and a word boundary, a new segment moves arenas and planes
def test_after_syncs(host):
    h = host
    before = both(h, C3, label="before")
    h.change(1, 1000, 1500, flip=True)
    h.sync(1, 1000, 1500)
    changed = both(h, C3, label="after a change of 1500 rows")
    want = sum(int(c3_mask(seg, seg["size"]).sum()) for seg in h.tab.segments)
    assert changed.passed_recs == want and want != before.passed_recs
    h.append(2, 700)                                       # rows 5000 .. 5699: the word that held 8 rows fills up, chunk 2 ends at 6144
    grown = both(h, C3, label="after 700 appended rows")
    assert grown.scanned_recs == before.scanned_recs + 700
    both(h, EVERY_ROW, label="after 700 appended rows, every row passes")
    h.append(2, 500)                                       # ... and across the chunk's end
    both(h, EVERY_ROW, dims=(0, 1), hint=100_000, label="after 1200 appended rows, every row passes")
    h.add_segment(3000)                                    # beyond the reserve: arenas and planes moved
    more = both(h, C3, label="after a fourth segment")
    assert more.scanned_recs == before.scanned_recs + 1200 + 3000 and more.scanned_segments == 4
    both(h, EVERY_ROW, dims=PART[0], flags=PART[1], path="dense_part", label="after a fourth segment, every row passes")


# ---- 8. the layout budget sees the use, and the projection is held at the query's tick
def test_uses_are_counted(shared):
    def sliced():
        lay, summ = shared.dt.layouts()
        lay = [x for x in lay if x.kind == capi.LAYOUT_PRED_SLICED]
        assert len(lay) == 1
        return lay[0], summ
    n = sliced()[0].uses
    plan = AggPlan(filter=C3[0], groups=[GroupSpec(D2)], metrics=[METRIC["m0"], METRIC["count"]], flags=BASE | PREBUILT)
    for k in range(3):
        res = shared.dt.query_agg(plan)
        assert res.sliced_prebuilt
        lay, summ = sliced()
        assert lay.uses == n + k + 1 and lay.last_use == summ.tick, (lay.uses, lay.last_use, summ.tick)
    res = shared.dt.query_agg(AggPlan(filter=C3[0], groups=[GroupSpec(D2)], metrics=[METRIC["m0"], METRIC["count"]], flags=BASE))
    assert not res.sliced_prebuilt and sliced()[0].uses == n + 3      # the twin reads the arenas


# ---- 9. the environment switch: read once per process, so one child each way
CHILD = """
import sys
sys.path.insert(0, {root!r})
import tests.conftest
from viyadb_amd import capi, executor
from viyadb_amd.executor import AggPlan, GroupSpec
from tests.test_gpu_layout_lifecycle import C3Host
executor.init(0)
h = C3Host(3, 5000, 8192)
h.dt.predpack([2, 3, 4], sliced=True)
p = h.w.plan
res = h.dt.query_agg(AggPlan(filter=p.filter, groups=[GroupSpec(2)], metrics=p.metrics, flags=capi.PLAN_NO_JIT | capi.PLAN_NO_LANES))
print("FLAGS", res.flags, res.passed_recs, res.kernel)
h.close()
"""


@pytest.mark.parametrize("value", ["1", None], ids=["VH_SLICED_PREBUILT=1", "unset"])
def test_the_environment_switch(shared, value):
    env = {k: v for k, v in os.environ.items() if k != "VH_SLICED_PREBUILT"}
    if value is not None:
        env["VH_SLICED_PREBUILT"] = value
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("FLAGS ")][-1].split(None, 3)
    flags, passed, kernel = int(line[1]), int(line[2]), line[3]
    here = shared.dt.query_agg(AggPlan(filter=C3[0], groups=[GroupSpec(D2)], metrics=[METRIC["m0"], METRIC["count"]], flags=BASE))
    assert passed == here.passed_recs
    if value is not None:
        assert flags & BIT26 and flags & ON_PLANES == ON_PLANES and not flags & OFF and kernel.startswith("scan_agg_sliced_kernel<"), (hex(flags), kernel)
    else:
        # (the child's table is fresh: the layouts this module's queries had built unasked on the shared one are not compared)
        assert not flags & BIT26 and "scan_agg_sliced_kernel" not in kernel and kernel.split("<")[0] == here.kernel.split("<")[0], (hex(flags), kernel, here.kernel)
