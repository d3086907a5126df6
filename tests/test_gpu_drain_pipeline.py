"""The pipelined drain of the compiled scan (vj_drain_pipe, viyadb_amd/csrc/vh_jit_body.h): a wave keeps the raw records of one or two groups
of 64 survivors in flight while it sinks the group before them. VH_TEST_DRAIN_DEPTH (0, 1, 2; read when the shape is built) switches the
depth between two queries; depth 0 is one drain after another. Every answer is compared with the oracle (tests/parity.compare) and the
depths must agree bit for bit — keys and states after sort_rows, and passed_recs — from different code objects wherever the plan gathers one
packed record, from the same one where it does not. Tables: 3 segments of 5 000 mirrored rows (two full tiles and one of 904) with room
for 8 192, so a wave owns one tile per segment and every segment change flushes what the wave holds."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare, sort_rows
from tests.planner import mirror_table
from tests.test_gpu_layout_lifecycle import C3Host, D2
from tests.test_gpu_typed import F, run
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="the drain lives in the compiled scan")]
PART, JIT, PACK = 64, capi.PLAN_FORCE_JIT, capi.PLAN_FORCE_PACK
HOT = PART | JIT | PACK
ROWS, CAP, TILE = 5000, 8192, 2048
DEPTHS = (0, 1, 2)
FORMS = (("clustered planes", HOT), ("row-order planes over grouped records", HOT | capi.PLAN_NO_GPLANES), ("row-order records", HOT | capi.PLAN_NO_GROUPED))
ARENAS = PART | JIT | capi.PLAN_NO_PACK


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def leaf(col, op, name, v):
    return ("rel", col, op, v), {"op": name, "column": f"d{col}", "value": str(v)}


C3 = [leaf(D2, capi.OP_EQ, "eq", 1), leaf(3, capi.OP_LT, "lt", 447), leaf(4, capi.OP_GE, "ge", 553)]


def ask(h, flags, depth, monkeypatch, seg_rows=None, label=""):
    monkeypatch.setenv("VH_TEST_DRAIN_DEPTH", str(depth))
    filt = [l[0] for l in C3] + [("and", len(C3))]
    q = dict(h.w.query, filter={"op": "and", "filters": [l[1] for l in C3]})
    p = h.w.plan
    res = h.dt.query_agg(AggPlan(filter=filt, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint, seg_rows=seg_rows))
    compare(res, vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows), f"{label} depth={depth} flags={flags:#x} snapshot={seg_rows}")
    assert res.jit, (label, res.path, res.kernel)
    print(f"{label} depth={depth} snapshot={seg_rows}: {res.path} {res.kernel} passed={res.passed_recs} retries={res.retries}")
    return res


def fold_d0(h, n):
    """d0 modulo n: n x 100 groups. The planner keeps a dense table only up to four groups per scanned row — C3's 100 000 groups over 15 000
    rows go through the hash table — so folded tables are what sends these small scans through DENSE_PART and its ring writer."""
    for s, seg in enumerate(h.tab.segments):
        seg["d"][0][:] %= n
        h.sync(s, 0, ROWS)


def same_bits(a, b, label):
    pa, pb = sort_rows(a.keys, a.states), sort_rows(b.keys, b.states)
    assert a.passed_recs == b.passed_recs, label
    for x, y in zip(a.keys + a.states, b.keys + b.states):
        assert x.dtype == y.dtype and x.dtype.kind in "iu" and np.array_equal(x[pa], y[pb]), label


def every_depth(h, flags, monkeypatch, seg_rows=None, label="", pipelined=True):
    """The query at depths 0, 1 and 2: the oracle's answer each time, the same bits, and a code object per depth (or one, without a packed record)."""
    res = [ask(h, flags, d, monkeypatch, seg_rows, label) for d in DEPTHS]
    for d in DEPTHS[1:]:
        same_bits(res[0], res[d], f"{label}: depth 0 against depth {d}")
    names = {r.kernel for r in res}
    assert len(names) == (len(DEPTHS) if pipelined else 1), (label, [r.kernel for r in res])
    return res[0]


def every_form(h, monkeypatch, seg_rows=None, label="", planes=True):
    first = None
    for name, flags in FORMS:
        r = every_depth(h, flags, monkeypatch, seg_rows, f"{label}, {name}")
        assert r.packed and r.pack_rec_bytes == 4, (label, name, hex(r.flags))
        assert r.grouped_planes == (planes and flags == HOT) and r.grouped_payload == (not flags & capi.PLAN_NO_GROUPED), (label, name, hex(r.flags))
        if first is not None:
            same_bits(first, r, f"{label}: clustered planes against {name}")
        first = first or r
    return first


@pytest.fixture
def host():
    h = C3Host(3, ROWS, CAP)
    yield h
    h.close()


def warm(h):
    flags = h.dt.warm(h.plan(HOT))
    assert flags & capi.INFO_GROUPED_PAYLOAD and flags & capi.INFO_GROUPED_PLANES, hex(flags)


def set_counts(h, counts):
    """counts[s][tile] rows of the tile hold d2 == 1, and every one of them passes d3 and d4; no other row of the tile passes."""
    rng = np.random.default_rng(11)
    for s, per_tile in enumerate(counts):
        seg = h.tab.segments[s]
        for tile, n in enumerate(per_tile):
            sl = slice(tile * TILE, min((tile + 1) * TILE, ROWS))
            d2 = seg["d"][D2][sl]
            d2[d2 == 1] = 0
            at = rng.choice(len(d2), size=n, replace=False)
            d2[at] = 1
            seg["d"][3][sl][at] = 5
            seg["d"][4][sl][at] = 900
        h.sync(s, 0, ROWS)


# a wave's queue holds exactly its tile's count when the segment ends. 64, 128 and 192: the queue is EMPTY at the flush while one or two whole
# groups are still pending — a flush that looks at the queue's count alone loses them; 63 / 65 / 127 / 129: a part group beside them
@pytest.mark.parametrize("counts, fold", [(((0, 1, 63), (64, 65, 127), (128, 129, 192)), 0), (((0, 1, 63), (64, 65, 127), (128, 129, 192)), 250),
                                          (((192, 128, 64), (129, 65, 1), (127, 63, 0)), 250), (((64, 64, 64), (128, 128, 128), (192, 192, 192)), 0)],
                         ids=["rising-hash", "rising-part", "whole-groups-first-part", "whole-groups-everywhere-hash"])
def test_exact_survivor_counts(host, monkeypatch, counts, fold):
    warm(host)
    if fold:
        fold_d0(host, fold)
    set_counts(host, counts)
    r = every_form(host, monkeypatch, label=f"counts {counts}")
    assert r.passed_recs == sum(map(sum, counts)), (r.passed_recs, counts)
    assert r.path == ("dense_part" if fold else "hash"), r.path
    # ... and the tiles one by one from the clustered planes (whole-tile snapshots): a group left pending when the wave's work ends
    for snap in ([TILE, 0, 0], [0, TILE, 0], [0, 0, TILE]):
        s = every_depth(host, HOT, monkeypatch, seg_rows=snap, label=f"counts {counts}, snapshot {snap}")
        assert s.passed_recs == sum(c[0] for c, n in zip(counts, snap) if n), (s.passed_recs, snap)


@pytest.mark.parametrize("fold", [0, 250], ids=["hash", "part"])
@pytest.mark.parametrize("snap", [None, [ROWS, 0, ROWS], [2048, 4096, ROWS]])
def test_segment_change(host, monkeypatch, snap, fold):
    """The segments hold different d0 / d1 / m0 at equal places (generated from their own row numbers): a pending group sunk under the next
    segment's base, or carried past a segment the snapshot hides, changes the groups."""
    warm(host)
    if fold:
        fold_d0(host, fold)
    a, b = host.tab.segments[0], host.tab.segments[2]
    assert not np.array_equal(a["d"][0][:ROWS], b["d"][0][:ROWS]) and not np.array_equal(a["m"][0][:ROWS], b["m"][0][:ROWS])
    assert every_form(host, monkeypatch, seg_rows=snap, label="segment change").passed_recs > 0


def test_arenas_keep_their_kernel(host, monkeypatch):
    """VH_PLAN_NO_PACK: a survivor's values come out of four arenas — no packed record, no pipeline, and the depth is no part of the shape.
    (The plan is asked a few times first: its third sighting builds predicate layouts unasked, which is a new shape at any depth.)"""
    warm(host)
    for _ in range(4):
        r0 = ask(host, ARENAS, 0, monkeypatch, label="the arenas")
    assert not r0.packed and r0.passed_recs > 0
    for d in DEPTHS:
        r = ask(host, ARENAS, d, monkeypatch, label="the arenas")
        same_bits(r0, r, f"the arenas: depth 0 against depth {d}")
        assert r.kernel == r0.kernel, (d, r0.kernel, r.kernel)


def test_every_row_passing_two_partitions(host, monkeypatch):
    """5 000 survivors a segment — drain after drain with both pending groups full — into the two LDS-sized ranges 80 x 100 groups make (as in
    the ring stress case of tests/test_gpu_skew.py): every call of the ring writer goes through its wait loop with a gather in flight."""
    warm(host)
    for s, seg in enumerate(host.tab.segments):
        seg["d"][0][:] %= 80
        seg["d"][D2][:] = 1
        seg["d"][3][:] = 5
        seg["d"][4][:] = 900
        host.sync(s, 0, ROWS)
    for name, flags in FORMS[:2]:
        flags |= capi.PLAN_NO_QPAY         # (from 15 % of the rows on the scan would stream the records beside the planes: nothing to gather)
        r2 = ask(host, flags, 2, monkeypatch, label=f"every row passes, {name}")
        assert r2.passed_recs == 3 * ROWS and r2.path == "dense_part" and r2.pack_rec_bytes == 4, (name, r2.passed_recs, hex(r2.flags), r2.path)
        r0 = ask(host, flags, 0, monkeypatch, label=f"every row passes, {name}")
        same_bits(r0, r2, f"every row passes, {name}: depth 0 against depth 2")
        assert r0.kernel != r2.kernel, r0.kernel
        same_bits(r0, ask(host, flags, 1, monkeypatch, label=f"every row passes, {name}"), f"every row passes, {name}: depth 0 against depth 1")


def test_eight_byte_record(monkeypatch):
    """A compressed projection at byte widths (negative values: no bit fields) whose five columns take one 8-byte record: rec_load is an 8-byte
    load, rec_unpack sign-extends. The column ranges of tests/test_gpu_pack.py::test_compressed_records_follow_syncs_and_outgrown_widths."""
    rng = np.random.default_rng(23)
    desc = {"name": "t", "segment_size": 30000, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "int"}, {"name": "f", "type": "uint"}],
            "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}, {"name": "w", "type": "int_min"}]}
    tab = vo.Table(desc)
    for n in (30000, 20000, 64 * 7):
        tab.add_segment_arrays([rng.integers(0, 50, n).astype(np.uint32), rng.integers(-40, 40, n).astype(np.int32), rng.integers(0, 100, n).astype(np.uint32)],
                               [rng.integers(-100, 100, n).astype(np.int64), rng.integers(1, 4, n).astype(np.uint32), rng.integers(-100, 100, n).astype(np.int32)], None, n)
    dt = mirror_table(tab, reserve=3)
    q = {"dimensions": ["a", "b"], "metrics": ["v", "count", "w"], "filter": F("lt", "f", "8")}
    try:
        dt.pack([0, 1, 3, 4, 5], compressed=True)
        res = []
        for d in DEPTHS:
            monkeypatch.setenv("VH_TEST_DRAIN_DEPTH", str(d))
            r, _ = run(tab, dt, q, flags=JIT | capi.PLAN_NO_LANES)
            assert r.packed and r.packed_compressed and r.jit and not r.pack_bits and r.pack_rec_bytes == 8, (hex(r.flags), r.pack_rec_bytes, r.kernel)
            res.append(r)
        same_bits(res[0], res[1], "8-byte record: depth 0 against depth 1")
        same_bits(res[0], res[2], "8-byte record: depth 0 against depth 2")
        assert len({r.kernel for r in res}) == 3, [r.kernel for r in res]
    finally:
        dt.close()
