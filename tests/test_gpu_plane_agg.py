"""Aggregates computed ON the bit-sliced predicate planes (scan_agg_planes_kernel over viyadb_amd/csrc/vh_bits_agg.h; opt-in: PLAN2_PLANE_AGG
in vh_plan.flags2, or VH_PLANE_AGG=1 for a process): sums and min / max by popcount, no row materialised.

Tables are three segments of 5000 rows, capacity 8192: two full 2048-row chunks and one of 904 per segment, the last plane word holding 8
rows. C3Host carries C3's schema with F = [d2, d3, d4] and V = [d2, m0, count] (a second host has ONE projection [d2, d3, m0, count], V = F:
C3's three filter columns and its two metrics together need 34 planes, and a projection has 32). `Small` is a table of its own for what
C3's schema lacks: group columns that start above 0, 64 and 65 group ids, sums that wrap, MIN / MAX kinds, AVG with the hidden count.

Every case runs its plan under PLAN_NO_JIT with PLAN2_PLANE_AGG and its twin without, and asserts: both equal the oracle over the host's
current arrays (tests/parity.compare: groups, ngroups, scanned_recs, scanned_segments, passed_recs); the two agree bit for bit (every state
here is an integer); vh_result_info.reserved bit 27 is set exactly where the planner's rule says, with bits 4 / 11 / 13, without bits 0 / 1 /
5 / 26, and the kernel is then scan_agg_planes_kernel<..>; where the rule says no, flags and kernel equal the twin's; the twin never has bit 27.
Nothing here is compiled at run time: the file runs under VH_JIT=off too.

A 32-bit unsigned column whose values need all 32 bits has no field: a projection of it alone would save nothing and is not built
(predpack_describe). So `uint_sum of 0xFFFFFFFF values` wraps through the fallback here (bit 27 clear, the oracle's wrapped sums), and the
wrap ON the planes is shown with 31-bit values, whose sum over 15 000 rows passes 2^32 thousands of times."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_agg_sliced import AND, OR, REL, SET, agree
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from tests.test_gpu_sync_batch import seg_columns
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSEG, ROWS, CAP = 3, 5000, 8192
ID, M0, M1, COUNT, M3, M4 = 6, 7, 8, 9, 10, 11       # C3's columns behind the dimensions
METRIC = {"m0": M0, "m1": M1, "count": COUNT, "m3": M3, "m4": M4}
FLAG2 = capi.PLAN2_PLANE_AGG
BASE = capi.PLAN_NO_JIT
BIT27 = capi.INFO_PLANE_AGG
ON_PLANES = capi.INFO_ON_PLANES      # vh_result_info.reserved: narrowed, a predicate projection, its bit-sliced form
OFF = capi.INFO_FAST | capi.INFO_LANES | capi.INFO_JIT | capi.INFO_SLICED_PREBUILT      # a register-resident kernel, its lanes form, a compiled kernel, the pre-built scan over the planes
SETS = capi.INFO_INSET | capi.INFO_INSET_SLICED
KERNEL = "scan_agg_planes_kernel<"
C3F = AND(REL(D2, "eq", 1), REL(D3, "lt", 447), REL(D4, "ge", 553))
EVERY_ROW = AND(REL(D3, "ne", 1023))                  # d3 holds 0 .. 999
NO_FILTER = ([], None)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def sliced_layouts(dt):
    return [x for x in dt.layouts()[0] if x.kind == capi.LAYOUT_PRED_SLICED]


def _host():
    h = C3Host(NSEG, ROWS, CAP)
    h.dt.predpack([D2, D3, D4], sliced=True)          # F
    h.dt.predpack([D2, M0, COUNT], sliced=True)       # V
    assert len(sliced_layouts(h.dt)) == 2
    return h


@pytest.fixture(scope="module")
def shared():
    """One C3 table, F and V two projections, for the cases that change nothing."""
    h = _host()
    yield h
    h.close()


@pytest.fixture
def host():
    h = _host()
    yield h
    h.close()


@pytest.fixture(scope="module")
def one():
    """One C3 table with ONE projection that holds filter, group and metric columns: V is F."""
    h = C3Host(NSEG, ROWS, CAP)
    h.dt.predpack([D2, D3, M0, COUNT], sliced=True)
    assert len(sliced_layouts(h.dt)) == 1
    yield h
    h.close()


def expect(a, b, on, sets, label):
    assert bool(a.flags & BIT27) == on and a.plane_agg == on, (label, hex(a.flags), a.kernel)
    assert not a.flags & capi.INFO_JIT and not a.jit, (label, hex(a.flags))
    if on:
        assert a.flags & ON_PLANES == ON_PLANES and not a.flags & OFF, (label, hex(a.flags))
        assert a.kernel.startswith(KERNEL), (label, a.kernel)
        assert a.flags & SETS == (SETS if sets else 0), (label, hex(a.flags))
    else:
        assert a.flags == b.flags and a.kernel == b.kernel, (label, hex(a.flags), hex(b.flags), a.kernel, b.kernel)      # the flag changed nothing
    assert not b.flags & BIT27 and not b.plane_agg and KERNEL not in b.kernel, (label, hex(b.flags), b.kernel)


def run_both(dt, plan, want, on, sets=False, label=""):
    """The plan with PLAN2_PLANE_AGG and its twin without: each against the oracle, against each other, and the path each took. -> the flagged run."""
    a, b = dt.query_agg(dataclasses.replace(plan, flags2=FLAG2)), dt.query_agg(plan)
    print(f"{label}: path {a.path} / {b.path}, flags {a.flags:#x} / {b.flags:#x}, passed {a.passed_recs}, groups {a.ngroups}, kernel {a.kernel} / {b.kernel}")
    compare(a, want, label + " [on the planes]")
    compare(b, want, label + " [twin]")
    agree(a, b, label)
    assert a.path == b.path, (label, a.path, b.path)
    expect(a, b, on, sets, label)
    return a


def both(h, filt, dims=(D2,), metrics=("m0", "count"), flags=0, seg_rows=None, on=True, sets=False, label="", having=(), top=None):
    """C3's table: `filt` in the two forms tests/test_gpu_agg_sliced.py writes filters in."""
    nodes, qfilter = filt
    q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics)}
    if qfilter is not None:
        q["filter"] = qfilter
    want = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    plan = AggPlan(filter=nodes, groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics], flags=BASE | flags, seg_rows=seg_rows,
                   having=having, top=top)
    return run_both(h.dt, plan, want, on, sets, f"{label} by={list(dims)} metrics={list(metrics)} flags={flags:#x} snapshot={seg_rows}")


# ---- 1. forms: scalar and grouped, no filter, 5 % and every row; V a second projection, and V = F
def test_forms_with_two_projections(shared):
    h = shared
    a = both(h, NO_FILTER, dims=(), label="no filter")
    assert a.path == "scalar" and a.ngroups == 1 and a.passed_recs == NSEG * ROWS
    a = both(h, C3F, dims=(), label="C3")
    assert a.path == "scalar" and 0 < a.passed_recs < a.scanned_recs
    a = both(h, C3F, label="C3")
    assert a.path == "dense_lds" and 0.03 < a.passed_recs / a.scanned_recs < 0.08
    a = both(h, EVERY_ROW, label="every row passes")
    assert a.passed_recs == a.scanned_recs == NSEG * ROWS and a.ngroups == 4
    both(h, NO_FILTER, label="no filter")
    z = both(h, AND(REL(D3, "lt", 447), REL(D3, "ge", 447)), label="no row passes")
    assert z.passed_recs == 0 and z.ngroups == 0 and z.scanned_segments == NSEG


def test_forms_with_one_projection(one):
    h = one
    two = AND(REL(D2, "eq", 1), REL(D3, "lt", 447))
    both(h, NO_FILTER, dims=(), label="V = F, no filter")
    both(h, two, dims=(), label="V = F")
    a = both(h, two, label="V = F")
    assert 0 < a.passed_recs < a.scanned_recs
    a = both(h, EVERY_ROW, label="V = F, every row passes")
    assert a.passed_recs == NSEG * ROWS
    both(h, C3F, on=False, label="V = F lacks d4: a filter column outside F")


# ---- 2. snapshots: nothing at or beyond seg_rows counts, the word that straddles it is masked; the planes beyond hold real rows
@pytest.mark.parametrize("snap", [[ROWS, n, ROWS] for n in (0, 1, 31, 32, 33, 2047, 2048, 2049, 4999)] + [[1, 31, 33], [0, 4999, 4097]],
                         ids=lambda s: "-".join(map(str, s)))
def test_snapshots(shared, snap):
    both(shared, C3F, seg_rows=snap, label="C3")
    a = both(shared, EVERY_ROW, seg_rows=snap, label="every row passes")
    assert a.passed_recs == sum(snap)
    a = both(shared, NO_FILTER, dims=(), seg_rows=snap, label="no filter")
    assert a.passed_recs == sum(snap)


def test_a_segment_skipped_by_its_min_max(host):
    h = host
    seg = h.tab.segments[1]
    seg["d"][D3][:ROWS] = 500 + seg["d"][D3][:ROWS] % 500           # d3 < 447 holds for no row of segment 1: its min / max say so
    h.sync(1, 0, ROWS)
    a = both(h, AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), label="segment 1 skipped")
    assert a.scanned_segments == 2 and a.scanned_recs == NSEG * ROWS and a.passed_recs > 0
    a = both(h, AND(REL(D3, "lt", 447)), dims=(), label="segment 1 skipped")
    assert a.scanned_segments == 2


# ---- 3. a table of its own: group columns above 0, 64 and 65 ids, wrapping sums, MIN / MAX kinds, AVG with the hidden count
A, B, C_, E, F_, Z = range(6)
SMALL_DIMS = ["a", "b", "c", "e", "f", "z"]
SMALL_METRICS = [("us", "uint_sum"), ("ls", "long_sum"), ("um", "uint_min"), ("lm", "long_max"), ("im", "int_min"), ("zm", "uint_max"),
                 ("av", "uint_avg"), ("ng", "int_sum"), ("dd", "double_sum"), ("full", "uint_sum")]
US, LS, UM, LM, IM, ZM, AV, NG, DD, FULL = range(6, 16)
HIDDEN = 16


class Small:
    def __init__(self, seed=7):
        rng = np.random.default_rng(seed)
        self.tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": n, "type": "uint"} for n in SMALL_DIMS],
                             "metrics": [{"name": n, "type": t} for n, t in SMALL_METRICS]})
        assert self.tab.has_hidden_count                          # an AVG metric and no COUNT
        for s in range(NSEG):
            n = ROWS
            b = rng.integers(0, 16, n).astype(np.uint32)
            b[b == 7] = 6                                         # the value 7 lies within b's range and in no row
            b[0], b[1] = 0, 15
            c = rng.integers(0, 11, n).astype(np.uint32)          # 0 .. 10, and two planted values: 11 in ONE row at bit 0 of a plane word,
            if s == 0:                                            # 12 in ONE row at bit 31 of another
                c[64] = 11
            if s == 1:
                c[2048 + 31] = 12
            e = rng.integers(0, 5, n).astype(np.uint32)
            e[0], e[1] = 0, 4
            d = [rng.integers(5, 9, n).astype(np.uint32), b, c, e, rng.integers(0, 1000, n).astype(np.uint32), np.arange(s * n, (s + 1) * n, dtype=np.uint32)]
            d[A][0], d[A][1] = 5, 8
            m = [(0x7FFFFFF0 + rng.integers(0, 16, n)).astype(np.uint32),                  # us: 31-bit values, the u32 sum wraps
                 (0xFFFFFF00 + rng.integers(0, 256, n)).astype(np.int64),                  # ls: 32-bit fields, the total passes 2^32
                 rng.integers(0, 1_000_000, n).astype(np.uint32),                          # um
                 rng.integers(0, 1_000_000, n).astype(np.int64),                           # lm
                 rng.integers(0, 1000, n).astype(np.int32),                                # im: non-negative
                 np.zeros(n, dtype=np.uint32),                                             # zm: a MAX of all zeros
                 rng.integers(0, 101, n).astype(np.uint32),                                # av
                 rng.integers(-50, 50, n).astype(np.int32),                                # ng: negative values, no field
                 rng.integers(0, 100, n).astype(np.float64),                               # dd
                 np.full(n, 0xFFFFFFFF, dtype=np.uint32)]                                  # full: needs all 32 bits, no projection is built
            self.tab.add_segment_arrays(d, m, rng.integers(1, 4, n).astype(np.uint64), n)
        self.dt = mirror_table(self.tab)
        for cols in ([A, B, F_], [A, B, UM], [US], [LS], [A, LM], [C_, E, IM, ZM, AV, HIDDEN]):
            before = len(sliced_layouts(self.dt))
            self.dt.predpack(cols, sliced=True)
            assert len(sliced_layouts(self.dt)) == before + 1, cols
        for cols in ([FULL], [A, NG]):                            # all 32 bits of a 4-byte column; negative values
            self.dt.predpack(cols, sliced=True)
        assert len(sliced_layouts(self.dt)) == 6

    def both(self, dims, metrics, flt=None, on=True, flags=0, label=""):
        q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
        if flt is not None:
            q["filter"] = flt
        aq = vo.parse_query(self.tab, q)
        want = vo.scan_aggregate(aq)
        plan = plan_from_query(self.tab, aq, flags=BASE | flags)
        return run_both(self.dt, plan, want, on, False, f"{label} by={list(dims)} metrics={list(metrics)} flags={flags:#x}"), want

    def close(self):
        self.dt.close()


@pytest.fixture(scope="module")
def small():
    t = Small()
    yield t
    t.close()


def F(op, col, v):
    return {"op": op, "column": col, "value": str(v)}


def test_groups(small):
    a, want = small.both(["a"], ["lm"], label="a group column whose values start at 5")
    assert a.ngroups == 4 and sorted(a.keys[0].tolist()) == [5, 6, 7, 8]
    a, _ = small.both(["a", "b"], ["um"], label="64 ids, b = 7 in no row")
    assert a.path == "dense_lds" and a.ngroups == 4 * 15 and 7 not in a.keys[1].tolist()
    a, _ = small.both(["a", "b"], ["um"], flt={"op": "and", "filters": [F("lt", "f", 500), F("ge", "a", 6)]}, label="64 ids under a filter on F = [a, b, f]")
    assert 0 < a.passed_recs < a.scanned_recs and 5 not in a.keys[0].tolist()
    a, _ = small.both(["c", "e"], ["im"], on=False, label="65 ids: beyond VH_PLANE_AGG_MAX_GROUPS")
    assert a.path == "dense_lds" and a.ngroups > 50


def test_states(small):
    a, want = small.both([], ["us"], label="uint_sum of 31-bit values")
    exact = sum(int(seg["m"][0][:ROWS].astype(np.uint64).sum()) for seg in small.tab.segments)
    assert exact > 1 << 32 and int(a.states[0][0]) == exact % (1 << 32)                  # it wrapped, as the reference's u32 does
    a, _ = small.both([], ["full"], on=False, label="uint_sum of 0xFFFFFFFF values: no 32-bit field of a 4-byte column")
    assert int(a.states[0][0]) == (NSEG * ROWS * 0xFFFFFFFF) % (1 << 32)
    a, _ = small.both([], ["ls"], label="long_sum over 32-bit fields")
    assert int(a.states[0][0]) > 1 << 32
    small.both(["a", "b"], ["um"], label="uint_min")
    small.both(["a"], ["lm"], label="long_max")
    small.both([], ["lm"], label="long_max")
    a, _ = small.both(["c"], ["im", "zm", "av"], label="int_min, a MAX of zeros, AVG with the hidden count")
    assert a.ngroups == 13 and a.hidden_count is not None and not a.states[1].any()       # every group present, its MAX 0
    rows = dict(zip(a.keys[0].tolist(), a.hidden_count.tolist()))
    assert set(rows) == set(range(13)) and 1 <= rows[11] <= 3 and 1 <= rows[12] <= 3      # the groups of ONE row each: bit 0 and bit 31 of their words
    a, _ = small.both(["c"], ["av"], flt=F("ge", "c", 11), label="the two groups of one row each alone (F = V = the projection with c)")
    assert a.passed_recs == 2 and a.ngroups == 2
    small.both(["e"], ["im"], label="int_min by e")


def test_ineligible_plans_of_the_small_table(small):
    small.both(["a"], ["dd"], on=False, label="a double metric")
    small.both(["a"], ["ng"], on=False, label="a metric with negative values")
    small.both(["a"], ["av"], on=False, label="a metric in no projection with a")
    small.both(["z"], ["lm"], on=False, label="a group column in no projection (15 000 ids besides)")


# ---- 4. filter kinds
def test_filter_kinds(shared):
    h = shared
    a = both(h, C3F, label="flat AND")
    x, y = AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), AND(REL(D2, "eq", 2), REL(D4, "ge", 553))
    a = both(h, (x[0] + y[0] + [("or", 2)], {"op": "or", "filters": [x[1], y[1]]}), label="(d2 == 1 & d3 < 447) | (d2 == 2 & d4 >= 553)")
    assert 0 < a.passed_recs < a.scanned_recs
    held = np.unique(np.concatenate([seg["d"][D4][:ROWS] for seg in h.tab.segments]))
    values = [int(v) for v in held[::len(held) // 8][:8]]
    for equal in (True, False):
        a = both(h, AND(SET(D4, values, equal)), label=f"d4 {'IN' if equal else 'NOT IN'} {values}")
        assert 0 < a.passed_recs < a.scanned_recs
        a = both(h, AND(SET(D4, values, equal, kind="inset"), REL(D2, "ne", 3)), sets=True, label=f"a set leaf on d4 (10-bit field), {'IN' if equal else 'NOT IN'}")
        assert 0 < a.passed_recs < a.scanned_recs
    both(h, OR(REL(D2, "eq", 0), REL(D3, "gt", 900)), dims=(), label="flat OR, scalar")


# ---- 5. where the rule says no: the flag is set, bit 27 is clear, nothing differs from the twin, and the result is right
def test_ineligible_plans(shared):
    h = shared
    both(h, C3F, metrics=("m3",), on=False, label="a double metric")
    both(h, C3F, metrics=("m0", "m1"), on=False, label="m1 in no projection with d2")
    both(h, AND(REL(D2, "eq", 1), REL(ID, "lt", 9000)), on=False, label="a filter column outside F")
    both(h, C3F, flags=capi.PLAN_FORCE_GLOBAL, on=False, label="FORCE_GLOBAL")
    both(h, C3F, flags=capi.PLAN_FORCE_HASH, on=False, label="FORCE_HASH")
    for flag in (capi.PLAN_NO_SLICED, capi.PLAN_NO_PREDPACK, capi.PLAN_NO_NARROW):
        both(h, C3F, flags=flag, on=False, label="kept off the planes")
        both(h, NO_FILTER, flags=flag, on=False, label="kept off the planes, no filter")
    # VH_COL_ROWID: the oracle knows no row-id metric; the two runs agree and the flag changes nothing
    runs = [h.dt.query_agg(AggPlan(filter=C3F[0], groups=[GroupSpec(D2)], metrics=[capi.COL_ROWID], flags=BASE, flags2=f2)) for f2 in (FLAG2, 0)]
    agree(runs[0], runs[1], "row positions")
    expect(runs[0], runs[1], False, False, "VH_COL_ROWID")
    # both switches: the aggregate on the planes wins
    a = both(h, C3F, flags=capi.PLAN_SLICED_PREBUILT | capi.PLAN_NO_LANES, label="with PLAN_SLICED_PREBUILT")
    assert not a.sliced_prebuilt


def test_a_group_column_with_granularity():
    from tests import time_edges as te
    tab = te._fill(vo.Table(te._schema([te._time_dim("ts", "time")])), [te._edge_columns("time")])
    dt = mirror_table(tab)
    try:
        aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "select": [{"column": "ts", "granularity": "year"}, {"column": "count"}]})
        now = te.NOW
        want = vo.scan_aggregate(aq, now=now)
        run_both(dt, plan_from_query(tab, aq, now=now, flags=BASE), want, False, label="GROUP BY ts truncated to days")
    finally:
        dt.close()


# ---- 6. HAVING and top-N behind the same table
def test_post_stages(shared):
    h = shared
    nodes, qfilter = EVERY_ROW
    q = {"type": "aggregate", "table": "synth", "dimensions": ["d2"], "metrics": ["m0", "count"], "filter": qfilter}
    want = vo.scan_aggregate(vo.parse_query(h.tab, q))
    sums = sorted(int(x) for x in want.states[0])
    cut = sums[1]                                                   # two of the four groups have a larger sum
    for kw in ({"having": [("rel", 1, capi.OP_GT, cut)]}, {"top": (1, True, 2)}):
        plan = AggPlan(filter=nodes, groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=BASE, **kw)
        a, b = h.dt.query_agg(dataclasses.replace(plan, flags2=FLAG2)), h.dt.query_agg(plan)
        assert a.returned == b.returned and a.ngroups == b.ngroups == 4, (kw, a.returned, b.returned)
        got = sorted(int(x) for x in a.states[0])
        if "having" in kw:
            assert got == sums[2:], kw
        else:                                                       # top-N delivers a superset of the first k rows (here it may be all four)
            assert set(sums[2:]) <= set(got) and a.returned >= 2, kw
        agree(a, b, str(kw))
        expect(a, b, True, False, str(kw))


# ---- 7. coherence: the planes follow the journal; a value that outgrows V's field drops V; a value outside the planned range re-plans
def test_after_syncs(host):
    h = host
    before = both(h, C3F, label="before")
    h.change(1, 1000, 1500, flip=True)                              # m0 and count changed in place, the filter columns moved across the literals
    h.sync(1, 1000, 1500)
    changed = both(h, C3F, label="after a change of 1500 rows")
    assert changed.passed_recs != before.passed_recs
    h.append(2, 700)                                                # rows 5000 .. 5699: the word that held 8 rows fills up
    grown = both(h, EVERY_ROW, label="after 700 appended rows")
    assert grown.scanned_recs == NSEG * ROWS + 700 and grown.passed_recs == grown.scanned_recs
    both(h, NO_FILTER, dims=(), label="after 700 appended rows, no filter")
    # m0 = 1001 .. 2000 needs 11 bits, V's field has 10: V is dropped, the query falls back, the rows are the oracle's
    h.tab.segments[0]["m"][0][:100] += 1500
    h.sync(0, 0, 100)
    both(h, C3F, on=False, label="m0 outgrew its field")
    assert len(sliced_layouts(h.dt)) == 1                           # F is still there
    both(h, C3F, metrics=("count",), on=False, label="no projection holds d2 and count any more")


def test_a_group_value_that_outgrows_its_field(host):
    """d2's fields have two bits. A row with d2 = 5 drops F and V, which both hold the column: the query falls back and finds the fifth group."""
    h = host
    h.tab.segments[2]["d"][D2][10] = 3                              # (stays within the field and the range: the plane path answers)
    h.sync(2, 10, 1)
    both(h, EVERY_ROW, label="d2 within its range")
    h.tab.segments[2]["d"][D2][10] = 5                              # 3 bits: beyond the 2-bit field, the projections with d2 go; the arenas answer
    h.sync(2, 10, 1)
    a = both(h, EVERY_ROW, on=False, label="d2 = 5 synced in")
    assert a.ngroups == 5


def test_a_value_outside_the_planned_range():
    """A string column's ids are planned by the caller's cardinality. The plan is made while the dictionary has three codes; a row with a fourth
    code is synced in afterwards (it fits the 2-bit field, so the projections stay). That row passes and belongs to no id: the kernel raises the
    range error and the existing re-plan (the hash organisation) returns the oracle's rows."""
    rng = np.random.default_rng(3)
    tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": "s", "type": "string"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "uint_sum"}, {"name": "count", "type": "count"}]})
    dic = tab.dicts["s"]
    for name in ("x", "y"):
        dic.v2c[name] = len(dic.c2v)
        dic.c2v.append(name)
    for _ in range(NSEG):
        s_ = rng.integers(0, 3, CAP).astype(np.uint32)
        s_[0], s_[1] = 0, 2
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
        assert plan.groups[0].cardinality == 3
        a = run_both(dt, plan, vo.scan_aggregate(aq), True, label="three codes, three ids")
        assert a.ngroups == 3
        dic.v2c["z"] = 3
        dic.c2v.append("z")
        seg = tab.segments[1]
        seg["d"][0][2048 + 31], seg["d"][1][2048 + 31] = 3, 0              # it passes the filter
        dt.sync_batch([(1, 2048 + 31, 1, ROWS, seg_columns(tab, seg), 0)])
        want = vo.scan_aggregate(vo.parse_query(tab, q))
        assert want.ngroups == 4
        a = run_both(dt, plan, want, False, label="a fourth code behind the plan's back")      # the plan still says three ids
        assert a.path == "hash" and len(sliced_layouts(dt)) == 2
        a = run_both(dt, plan_from_query(tab, vo.parse_query(tab, q), flags=BASE), want, True, label="planned again with four ids")
        assert a.ngroups == 4
    finally:
        dt.close()


# ---- 8. the layout budget sees the uses of F and V
def test_uses_are_counted(shared):
    def uses():
        return {tuple(x.cols[:x.ncols]): x.uses for x in sliced_layouts(shared.dt)}
    f, v = (D2, D3, D4), (D2, M0, COUNT)
    plan = AggPlan(filter=C3F[0], groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=BASE)
    n = uses()
    assert set(n) == {f, v}
    for k in range(3):
        res = shared.dt.query_agg(dataclasses.replace(plan, flags2=FLAG2))
        assert res.plane_agg
        assert uses() == {f: n[f] + k + 1, v: n[v] + k + 1}, (uses(), n)          # F and V, one use each per query
    res = shared.dt.query_agg(plan)
    assert not res.plane_agg and uses() == {f: n[f] + 3, v: n[v] + 3}              # the twin moves neither
    res = shared.dt.query_agg(dataclasses.replace(plan, filter=[], flags2=FLAG2))
    assert res.plane_agg and uses() == {f: n[f] + 3, v: n[v] + 4}                  # no filter: V alone


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
h.dt.predpack([2, 7, 9], sliced=True)
p = h.w.plan
res = h.dt.query_agg(AggPlan(filter=p.filter, groups=[GroupSpec(2)], metrics=p.metrics, flags=capi.PLAN_NO_JIT))
print("FLAGS", res.flags, res.passed_recs, res.kernel)
h.close()
"""


@pytest.mark.parametrize("value", ["1", None], ids=["VH_PLANE_AGG=1", "unset"])
def test_the_environment_switch(shared, value):
    env = {k: v for k, v in os.environ.items() if k != "VH_PLANE_AGG"}
    if value is not None:
        env["VH_PLANE_AGG"] = value
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("FLAGS ")][-1].split(None, 3)
    flags, passed, kernel = int(line[1]), int(line[2]), line[3]
    here = shared.dt.query_agg(AggPlan(filter=C3F[0], groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=BASE))
    assert passed == here.passed_recs
    if value is not None:
        assert flags & BIT27 and flags & ON_PLANES == ON_PLANES and not flags & OFF and kernel.startswith(KERNEL), (hex(flags), kernel)
    else:
        assert not flags & BIT27 and KERNEL not in kernel and kernel.split("<")[0] == here.kernel.split("<")[0], (hex(flags), kernel, here.kernel)
