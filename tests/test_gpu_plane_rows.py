"""The ROW SINK of the aggregate on the bit-sliced planes (PLAN2_PLANE_ROWS in vh_plan.flags2; vh_plane_agg.h: vh_plane_agg_rows;
scan_agg_planes_rows_kernel): plans of more than 64 group ids take the plane path, every surviving row's record rebuilt from the plane words
in registers and added to the block's LDS table once per metric.

Tables are three segments of 5000 rows, capacity 8192 — two full 2048-row chunks and one of 904 per segment, the last plane word holding 8
rows —: tests/test_gpu_plane_agg.py's `Small`, and `Wide`, a table of this file for what Small lacks: a group column of 2500 ids, a filter
column whose passing rows are planted chunk by chunk, a column that puts every row into one id, a column that names its segment.

Every case runs three ways: the plan with PLAN2_PLANE_ROWS, its twin without, and the oracle (tests/parity.compare). The flagged run and
the twin agree bit for bit (every state here is an integer). Where the rule says the row sink runs, the flagged run shows bit 27 with its
company, plane_sink == 2 and a kernel scan_agg_planes_rows_kernel<..>; where it says the loop runs (at most 64 ids), plane_sink == 1 and
scan_agg_planes_kernel<..>; where it says neither, plane_sink == 0 and flags and kernel are the twin's. The twin always has plane_sink == 0.
All plans but one carry PLAN_NO_JIT: nothing is compiled at run time.

Small has no plan of exactly 60 ids: its 64-id plan (a, b) holds 60 groups, b = 7 being in no row; that one, under a filter and without, the
4-id plan and the 13-id plan go through both sinks with VH_TEST_PLANE_ROWS_MIN=1."""
import dataclasses

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_agg_sliced import agree
from tests.test_gpu_plane_agg import BASE, BIT27, CAP, KERNEL, NSEG, OFF, ON_PLANES, ROWS, F, Small, sliced_layouts
from tests.test_gpu_sync_batch import seg_columns
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
AGG, ROWS2 = capi.PLAN2_PLANE_AGG, capi.PLAN2_PLANE_ROWS
RKERNEL = "scan_agg_planes_rows_kernel<"
HOOK = "VH_TEST_PLANE_ROWS_MIN"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def expect(a, b, sink, label):
    """a: the flagged run, b: its twin. sink: what the rule says of a."""
    assert a.plane_sink == sink and b.plane_sink == 0, (label, a.plane_sink, b.plane_sink, a.kernel, b.kernel)
    assert not b.flags & BIT27 and KERNEL not in b.kernel and RKERNEL not in b.kernel, (label, hex(b.flags), b.kernel)
    if sink:
        assert a.flags & BIT27 and a.plane_agg and a.flags & ON_PLANES == ON_PLANES and not a.flags & OFF, (label, hex(a.flags))
        assert a.kernel.startswith(RKERNEL if sink == 2 else KERNEL), (label, a.kernel)
    else:
        assert a.flags == b.flags and a.kernel == b.kernel, (label, hex(a.flags), hex(b.flags), a.kernel, b.kernel)      # the flag changed nothing


def run3(dt, plan, want, sink, label="", flags2=ROWS2):
    """The plan with `flags2`, its twin without, the oracle. -> the flagged run."""
    a, b = dt.query_agg(dataclasses.replace(plan, flags2=flags2)), dt.query_agg(plan)
    print(f"{label}: path {a.path} / {b.path}, sink {a.plane_sink} / {b.plane_sink}, flags {a.flags:#x} / {b.flags:#x}, passed {a.passed_recs}, "
          f"groups {a.ngroups}, retries {a.retries} / {b.retries}, kernel {a.kernel} / {b.kernel}")
    if want is not None:
        compare(a, want, label + " [flagged]")
        compare(b, want, label + " [twin]")
    agree(a, b, label)
    assert a.path == b.path and a.returned == b.returned, (label, a.path, b.path)
    expect(a, b, sink, label)
    return a


def ask(t, dims, metrics, flt=None, sink=2, flags=BASE, seg_rows=None, label="", flags2=ROWS2, **post):
    """t: Small or Wide (a `tab` and a `dt`)."""
    q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
    if flt is not None:
        q["filter"] = flt
    aq = vo.parse_query(t.tab, q)
    want = None if post else vo.scan_aggregate(aq, seg_rows=seg_rows)      # (a post stage: the twin stands in for the oracle)
    plan = dataclasses.replace(plan_from_query(t.tab, aq, flags=flags, seg_rows=seg_rows), **post)
    return run3(t.dt, plan, want, sink, f"{label} by={list(dims)} metrics={list(metrics)} snapshot={seg_rows}", flags2)


# ---- the table of this file
G_, H_, K_, P_, S_, O_ = range(6)
LS, CN = 6, 7
# passing rows (p = 1) per 2048-row chunk, planted: (segment, chunk) -> rows of the chunk. A survivor's place in the wave's queue is its
# slice (8 bits of a lane's word), then its lane, then its bit: 63 / 64 / 65 survivors of ONE slice are a drain group short of one, full, and a
# second group of one; 128 / 129 the same at two groups; ONE survivor at bit 0 of lane 0 and at bit 31 of lane 63; none; all 2048.
# (A segment's third chunk has 904 rows, 28 words and 8 rows: its 63 survivors are three bits of one slice in 21 lanes.)
LANES = np.arange(64) * 32
PLANT = {(0, 0): np.arange(2048), (0, 1): np.array([2047]), (0, 2): np.array([], dtype=np.int64),
         (1, 0): LANES + 3, (1, 1): np.concatenate([LANES + 3, [10 * 32 + 4]]), (1, 2): np.concatenate([LANES[:21] + 1, LANES[:21] + 3, LANES[:21] + 5]),
         (2, 0): np.concatenate([LANES + 3, LANES + 5]), (2, 1): np.concatenate([LANES + 3, LANES + 5, [63 * 32 + 7]]), (2, 2): np.array([0])}
PLANTED = {k: len(v) for k, v in PLANT.items()}


class Wide:
    def __init__(self, seed=11):
        rng = np.random.default_rng(seed)
        self.tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": n, "type": "uint"} for n in ("g", "h", "k", "p", "s", "o")],
                             "metrics": [{"name": "ls", "type": "long_sum"}, {"name": "c", "type": "uint_sum"}]})
        for s in range(NSEG):
            n = ROWS
            g = rng.permutation(np.arange(n) % 2500).astype(np.uint32)      # every one of the 2500 ids, twice per segment
            h = rng.integers(0, 2, n).astype(np.uint32)
            h[0], h[1] = 0, 1
            k = rng.integers(3, 73, n).astype(np.uint32)              # 70 ids that start at 3
            k[0], k[1] = 3, 72
            p = np.zeros(n, dtype=np.uint32)
            for c in range(3):
                p[2048 * c + PLANT[(s, c)]] = 1
            o = np.full(n, 7, dtype=np.uint32)                        # every row in ONE of 70 ids, but the two that span the range
            o[0], o[1] = 0, 69
            d = [g, h, k, p, np.full(n, s, dtype=np.uint32), o]
            m = [rng.integers(0, 32768, n).astype(np.int64), rng.integers(1, 4, n).astype(np.uint32)]
            m[0][2], m[0][3] = 0, 32767
            self.tab.add_segment_arrays(d, m, None, n)
        self.dt = mirror_table(self.tab)
        for cols in ([G_, H_, LS, CN], [K_, H_, O_, LS, CN], [P_, S_]):      # 12 + 1 + 15 + 2, 7 + 1 + 7 + 15 + 2 (all 32) and 1 + 2 planes
            before = len(sliced_layouts(self.dt))
            self.dt.predpack(cols, sliced=True)
            assert len(sliced_layouts(self.dt)) == before + 1, cols

    def close(self):
        self.dt.close()


@pytest.fixture(scope="module")
def wide():
    t = Wide()
    yield t
    t.close()


@pytest.fixture(scope="module")
def small():
    t = Small()
    yield t
    t.close()


# ---- 1. the smallest row plan: 65 ids. With PLAN2_PLANE_AGG alone it stays off the planes, as before this flag
def test_65_ids_take_the_row_sink(small):
    a = ask(small, ["c", "e"], ["im"], label="65 ids")
    assert a.path == "dense_lds" and a.ngroups > 50
    ask(small, ["c", "e"], ["im"], sink=0, flags2=AGG, label="65 ids with PLAN2_PLANE_AGG alone: not on the planes")
    a = ask(small, ["c", "e"], ["im"], flags2=AGG | ROWS2, label="65 ids with both flags")
    a = ask(small, ["c", "e"], ["im"], flt=F("ge", "c", 11), label="the two rows at bit 0 and bit 31 of their words")
    assert a.passed_recs == 2 and a.ngroups == 2
    ask(small, ["a", "b"], ["um"], sink=1, label="64 ids with PLAN2_PLANE_ROWS: the loop, as with PLAN2_PLANE_AGG")
    ask(small, [], ["us"], sink=1, label="a total with PLAN2_PLANE_ROWS: the loop")


# ---- 2. 2500 ids: a table of 22 KB and of 32 KB; a column more and the organisation is no longer the LDS table
def test_2500_ids_and_beyond_the_lds_table(wide):
    a = ask(wide, ["g"], ["ls"], label="2500 ids")
    assert a.path == "dense_lds" and a.ngroups == 2500 and a.passed_recs == NSEG * ROWS
    a = ask(wide, ["g"], ["ls", "c"], label="2500 ids, 13 bytes each")
    assert a.path == "dense_lds"
    a = ask(wide, ["g"], ["ls", "c"], flt=F("eq", "p", 1), label="2500 ids under the planted filter")
    assert a.passed_recs == sum(PLANTED.values())
    a = ask(wide, ["g", "h"], ["ls", "c"], sink=0, label="5000 ids: beyond the LDS table")
    assert a.path != "dense_lds" and a.ngroups > 4000


# ---- 3. survivors per chunk at the drain group's and the slice's boundaries
def test_planted_survivor_counts(wide):
    assert sorted(PLANTED.values()) == [0, 1, 1, 63, 64, 65, 128, 129, 2048]
    a = ask(wide, ["k"], ["ls", "c"], flt=F("eq", "p", 1), label="planted survivors")
    assert a.passed_recs == sum(PLANTED.values()) and a.path == "dense_lds"
    for s in range(NSEG):                                           # segment by segment, and chunk by chunk through the snapshot
        for upto in (2048, 4096, ROWS):
            snap = [upto if i == s else 0 for i in range(NSEG)]
            a = ask(wide, ["k"], ["ls"], flt=F("eq", "p", 1), seg_rows=snap, label=f"planted survivors of segment {s} up to row {upto}")
            assert a.passed_recs == sum(PLANTED[(s, c)] for c in range(3) if 2048 * c < upto), (s, upto, a.passed_recs)


# ---- 4. every row in ONE id; ids that start above 0; two group columns
def test_one_hot_id_offsets_and_strides(wide):
    a = ask(wide, ["o"], ["ls"], label="every row but six in one of 70 ids")
    assert a.ngroups == 3 and a.path == "dense_lds"
    hot = dict(zip(a.keys[0].tolist(), a.states[0].tolist()))[7]
    assert hot == sum(int(seg["m"][0][:ROWS][seg["d"][O_][:ROWS] == 7].sum()) for seg in wide.tab.segments)
    a = ask(wide, ["k"], ["ls"], label="70 ids from 3 on")
    assert a.ngroups == 70 and min(a.keys[0].tolist()) == 3 and max(a.keys[0].tolist()) == 72
    a = ask(wide, ["k", "h"], ["ls"], label="two group columns: 140 ids")
    assert a.ngroups == 140
    a = ask(wide, ["h", "k"], ["ls"], label="... in the other order")
    assert a.ngroups == 140
    a = ask(wide, ["h", "k"], ["ls", "c"], flt=F("eq", "p", 1), label="... under the planted filter")
    assert a.passed_recs == sum(PLANTED.values())


# ---- 5. states. Small's wrapping and 64-bit sums and its MIN / MAX of other projections have at most 64 ids: the hook sends them through
def test_states(small, monkeypatch):
    a = ask(small, ["c", "e"], ["im", "zm", "av"], label="int_min, a MAX of zeros, AVG with the hidden count")
    assert a.hidden_count is not None and not a.states[1].any()
    want = vo.scan_aggregate(vo.parse_query(small.tab, {"type": "aggregate", "table": "t", "dimensions": ["c", "e"], "metrics": ["im"]}))
    cut = sorted(int(x) for x in want.states[0])[len(want.states[0]) // 2]
    a = ask(small, ["c", "e"], ["im"], label="HAVING im > cut", having=[("rel", 2, capi.OP_GT, cut)])
    assert 0 < a.returned < a.ngroups and all(int(x) > cut for x in a.states[0])
    a = ask(small, ["c", "e"], ["im"], label="top 5 by im", top=(2, True, 5))
    assert a.returned >= 5
    monkeypatch.setenv(HOOK, "1")
    a = ask(small, [], ["us"], label="uint_sum of 31-bit values through the row sink")
    exact = sum(int(seg["m"][0][:ROWS].astype(np.uint64).sum()) for seg in small.tab.segments)
    assert exact > 1 << 32 and int(a.states[0][0]) == exact % (1 << 32)                  # it wrapped, as the reference's u32 does
    a = ask(small, [], ["ls"], label="long_sum over 32-bit fields")
    assert int(a.states[0][0]) > 1 << 32
    ask(small, ["a", "b"], ["um"], label="uint_min")
    ask(small, ["a"], ["lm"], label="long_max")
    ask(small, ["c"], ["im", "zm", "av"], label="13 ids: int_min, a MAX of zeros, AVG")


# ---- 6. a ragged snapshot and a skipped segment
def test_snapshots_and_a_skipped_segment(wide):
    for snap in ([2048 + 32 * 5 + 13, 0, ROWS], [1, ROWS - 9, 33], [0, 0, 9]):
        a = ask(wide, ["g"], ["ls", "c"], seg_rows=snap, label="ragged")
        assert a.passed_recs == sum(snap)
        ask(wide, ["k"], ["ls"], flt=F("eq", "p", 1), seg_rows=snap, label="ragged, planted filter")
    a = ask(wide, ["g"], ["ls"], flt=F("ge", "s", 1), label="segment 0 skipped by its min / max")
    assert a.scanned_segments == 2 and a.passed_recs == 2 * ROWS
    a = ask(wide, ["k"], ["ls"], flt={"op": "and", "filters": [F("eq", "s", 1), F("eq", "p", 1)]}, label="segments 0 and 2 skipped")
    assert a.scanned_segments == 1 and a.passed_recs == sum(PLANTED[(1, c)] for c in range(3))


# ---- 7. a value beyond the planned range, synced in between two queries: the kernel raises the range error, the re-plan answers
def test_a_value_outside_the_planned_range():
    rng = np.random.default_rng(5)
    tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": "s", "type": "string"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "uint_sum"}, {"name": "count", "type": "count"}]})
    dic = tab.dicts["s"]
    while len(dic.c2v) < 70:
        dic.v2c[f"v{len(dic.c2v)}"] = len(dic.c2v)
        dic.c2v.append(f"v{len(dic.c2v)}")
    for _ in range(NSEG):
        s_ = rng.integers(0, 70, CAP).astype(np.uint32)
        s_[0], s_[1] = 0, 69
        tab.add_segment_arrays([s_, rng.integers(0, 1000, CAP).astype(np.uint32)],
                               [rng.integers(0, 500, CAP).astype(np.uint32), rng.integers(1, 4, CAP).astype(np.uint32)], None, ROWS)
    dt = mirror_table(tab)
    try:
        dt.predpack([0, 1], sliced=True)
        dt.predpack([0, 2, 3], sliced=True)
        assert len(sliced_layouts(dt)) == 2
        q = {"type": "aggregate", "table": "t", "dimensions": ["s"], "metrics": ["v", "count"], "filter": F("lt", "f", 800)}
        aq = vo.parse_query(tab, q)
        plan = plan_from_query(tab, aq, flags=BASE)
        assert plan.groups[0].cardinality == 70
        a = run3(dt, plan, vo.scan_aggregate(aq), 2, label="70 codes, 70 ids")
        assert a.ngroups == 70 and a.retries == 0
        dic.v2c["z"] = 70
        dic.c2v.append("z")
        seg = tab.segments[1]
        seg["d"][0][2048 + 31], seg["d"][1][2048 + 31] = 70, 0              # it passes the filter, and fits the 7-bit field: the projections stay
        dt.sync_batch([(1, 2048 + 31, 1, ROWS, seg_columns(tab, seg), 0)])
        want = vo.scan_aggregate(vo.parse_query(tab, q))
        assert want.ngroups == 71
        a = run3(dt, plan, want, 0, label="a 71st code behind the plan's back")      # the plan still says 70 ids
        assert a.retries >= 1 and a.ngroups == 71 and len(sliced_layouts(dt)) == 2
        a = run3(dt, plan_from_query(tab, vo.parse_query(tab, q), flags=BASE), want, 2, label="planned again with 71 ids")
        assert a.ngroups == 71 and a.retries == 0
    finally:
        dt.close()


# ---- 8. both sinks in one process: VH_TEST_PLANE_ROWS_MIN=1 sends plans of at most 64 ids through the row sink
def test_both_sinks_agree(small, monkeypatch):
    flt = {"op": "and", "filters": [F("lt", "f", 500), F("ge", "a", 6)]}
    cases = [(["a"], ["lm"], None, "4 ids"), (["a", "b"], ["um"], None, "64 ids, 60 groups"), (["a", "b"], ["um"], flt, "64 ids under a filter"),
             (["c"], ["im", "zm", "av"], None, "13 ids"), ([], ["us"], None, "a total")]
    for dims, metrics, f, label in cases:
        monkeypatch.setenv(HOOK, "1")
        rows = ask(small, dims, metrics, flt=f, sink=2, label=label + " [row sink]")
        loop_hooked = ask(small, dims, metrics, flt=f, sink=1, flags2=AGG, label=label + " [PLAN2_PLANE_AGG under the hook: the loop]")
        monkeypatch.setenv(HOOK, "64")
        at64 = ask(small, dims, metrics, flt=f, sink=2 if label.startswith("64 ids") else 1, label=label + " [the hook at 64]")
        monkeypatch.delenv(HOOK)
        loop = ask(small, dims, metrics, flt=f, sink=1, label=label + " [loop]")
        for other in (loop_hooked, at64, loop):
            agree(rows, other, label)
            assert rows.returned == other.returned
    monkeypatch.setenv(HOOK, "1000")                                # (never above the loop's bound: 65 ids stay with the row sink)
    ask(small, ["c", "e"], ["im"], sink=2, label="65 ids, the hook at 1000")


# ---- 9. where the rule says no, the new flag changes nothing
def test_ineligible_plans(small, wide):
    ask(small, ["c", "e"], ["dd"], sink=0, label="a double metric")
    ask(small, ["c", "e"], ["ng"], sink=0, label="a metric with negative values")
    ask(small, ["c", "e"], ["lm"], sink=0, label="a metric in no projection with c and e")
    ask(small, ["z"], ["lm"], sink=0, label="a group column in no projection")
    for flag in (capi.PLAN_NO_SLICED, capi.PLAN_NO_PREDPACK, capi.PLAN_NO_NARROW, capi.PLAN_FORCE_GLOBAL, capi.PLAN_FORCE_HASH):
        ask(small, ["c", "e"], ["im"], sink=0, flags=BASE | flag, label=f"kept off by flag {flag:#x}")
    # a compiled kernel wins (none is compiled with the JIT switched off: then the row sink answers)
    a = ask(wide, ["k"], ["ls", "c"], flt=F("eq", "p", 1), sink=2 if JIT_OFF else 0, flags=capi.PLAN_FORCE_JIT, label="a compiled kernel present")
    assert a.jit == (not JIT_OFF)


def test_a_group_column_with_granularity():
    from tests import time_edges as te
    tab = te._fill(vo.Table(te._schema([te._time_dim("ts", "time")])), [te._edge_columns("time")])
    dt = mirror_table(tab)
    try:
        aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "select": [{"column": "ts", "granularity": "year"}, {"column": "count"}]})
        run3(dt, plan_from_query(tab, aq, now=te.NOW, flags=BASE), vo.scan_aggregate(aq, now=te.NOW), 0, label="GROUP BY ts truncated to years")
    finally:
        dt.close()
