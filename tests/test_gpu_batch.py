"""A batch of aggregates in one call (vh_query_agg_batch): the members that take the aggregate on the bit-sliced planes are answered by ONE
fused launch of scan_agg_planes_batch_kernel per group, everything else as the single query it is.

The tables are those of tests/test_gpu_plane_agg.py: C3Host(3, 5000, 8192) — two full 2048-row chunks and one of 904 rows per segment, the last
plane word holding 8 rows — with F = [d2, d3, d4] and V = [d2, m0, count]; the one-projection host [d2, d3, m0, count]; and its `Small` table
for 64 and 65 ids, MIN / MAX kinds, wrapping sums and AVG with the hidden count. Plans run under PLAN_NO_JIT | PLAN2_PLANE_AGG unless a case
says otherwise; nothing is compiled at run time, so the file runs under VH_JIT=off too.

For EVERY member of every batch: tests.parity.compare against the oracle over the host's arrays; `agree` bit for bit with dt.query_agg of
the same plan (every state here is an integer or a MIN / MAX: no tolerance anywhere) and the same counters and returned rows; a fused member
carries bit 30 on top of exactly the flags its single query has (bit 27 and its company), names the batch kernel and reports the fused
launch's time; a member that is not fused carries exactly the flags and the kernel name of its single query. BatchInfo must count what the
case expects. There is no external-stream case: the suite has no helper that hands the library a stream of the caller's."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_agg_sliced import AND, REL, SET, agree
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3
from tests.test_gpu_plane_agg import (BASE, BIT27, C3F, CAP, COUNT, EVERY_ROW, FLAG2, KERNEL, M0, METRIC, NO_FILTER, NSEG, OFF, ON_PLANES, ROWS, SETS,
                                      F, Small, _host, sliced_layouts)
from tests.test_gpu_sync_batch import seg_columns
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT30 = capi.INFO_BATCH_FUSED
BATCH_KERNEL = "scan_agg_planes_batch_kernel<256, "
TWO = AND(REL(D2, "eq", 1), REL(D3, "lt", 447))       # C3's filter without d4: what the one-projection host can answer


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def shared():
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
    h = C3Host(NSEG, ROWS, CAP)
    h.dt.predpack([D2, D3, M0, COUNT], sliced=True)
    yield h
    h.close()


@pytest.fixture(scope="module")
def small():
    t = Small()
    yield t
    t.close()


@dataclasses.dataclass
class Member:
    plan: AggPlan
    want: object            # the oracle's AggState (None: a post stage — the single query and the case's own assertions stand in)
    fused: bool
    sets: bool = False
    label: str = ""


def c3(h, filt, dims=(D2,), metrics=("m0", "count"), flags=0, flags2=FLAG2, seg_rows=None, fused=True, sets=False, label=""):
    nodes, qfilter = filt
    q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics)}
    if qfilter is not None:
        q["filter"] = qfilter
    want = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    plan = AggPlan(filter=nodes, groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics], flags=BASE | flags, flags2=flags2, seg_rows=seg_rows)
    return Member(plan, want, fused, sets, f"{label} by={list(dims)} metrics={list(metrics)} snapshot={seg_rows}")


def check_member(dt, r, m, info, groups, single=None):
    single = dt.query_agg(m.plan) if single is None else single
    print(f"{m.label}: fused {r.batch_fused}, flags {r.flags:#x} / single {single.flags:#x}, passed {r.passed_recs}, groups {r.ngroups}, kernel {r.kernel} / {single.kernel}")
    if m.want is not None:
        compare(r, m.want, m.label + " [batch]")
        compare(single, m.want, m.label + " [single]")
    agree(r, single, m.label)
    assert r.returned == single.returned and r.path == single.path, (m.label, r.returned, single.returned, r.path, single.path)
    assert r.batch_fused == m.fused and bool(r.flags & BIT30) == m.fused, (m.label, hex(r.flags), r.kernel)
    if m.fused:
        assert r.flags == single.flags | BIT30, (m.label, hex(r.flags), hex(single.flags))              # bit 30 and nothing else differs ...
        assert r.flags & BIT27 and r.flags & ON_PLANES == ON_PLANES and not r.flags & OFF, (m.label, hex(r.flags))      # ... from bit 27 and its company
        assert r.flags & SETS == (SETS if m.sets else 0), (m.label, hex(r.flags))
        assert r.kernel.startswith(BATCH_KERNEL) and single.kernel.startswith(KERNEL), (m.label, r.kernel, single.kernel)
        assert r.kernel[len(BATCH_KERNEL):] == single.kernel[len(KERNEL + "256, "):], (r.kernel, single.kernel)          # the same memory scope
        assert r.scan_kernel_ms > 0
        if groups == 1:
            assert r.scan_kernel_ms == pytest.approx(info.fused_kernel_ms, rel=1e-6), (r.scan_kernel_ms, info.fused_kernel_ms)
    else:
        assert r.flags == single.flags and r.kernel == single.kernel, (m.label, hex(r.flags), hex(single.flags), r.kernel, single.kernel)
    return single


def run_batch(dt, members, groups=None, label=""):
    res, info = dt.query_agg_batch([m.plan for m in members])
    nf = sum(m.fused for m in members)
    groups = (1 if nf else 0) if groups is None else groups
    print(f"{label}: {info.nplans} plans, {info.fused_groups} fused launch(es) of {info.fused_members} members, {info.singles} single, {info.fused_kernel_ms:.4f} ms")
    assert len(res) == len(members) == info.nplans
    assert (info.fused_groups, info.fused_members, info.singles) == (groups, nf, len(members) - nf), (label, info.fused_groups, info.fused_members, info.singles)
    assert (info.fused_kernel_ms > 0) == (groups > 0)
    for r, m in zip(res, members):
        check_member(dt, r, m, info, groups)
    return res, info


# ---- 1. mixed members, all fused: sizes 2, 3 and 8 on both hosts, each in two member orders
def kinds(h, filt):
    """Eight members over one V: totals and GROUP BY d2, no filter / `filt` / every row / a set leaf / OR."""
    held = np.unique(np.concatenate([seg["d"][D3][:ROWS] for seg in h.tab.segments]))
    values = [int(v) for v in held[::len(held) // 8][:8]]
    x, y = AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), AND(REL(D2, "eq", 2), REL(D3, "ge", 553))
    either = (x[0] + y[0] + [("or", 2)], {"op": "or", "filters": [x[1], y[1]]})
    return [c3(h, NO_FILTER, dims=(), label="total, no filter"),
            c3(h, filt, dims=(), label="total under the filter"),
            c3(h, filt, label="GROUP BY d2 at 5 %"),
            c3(h, EVERY_ROW, label="GROUP BY d2, every row passes"),
            c3(h, AND(SET(D3, values, True, kind="inset"), REL(D2, "ne", 3)), sets=True, label="a set leaf on d3 (10-bit field)"),
            c3(h, either, label="(d2 == 1 & d3 < 447) | (d2 == 2 & d3 >= 553)"),
            c3(h, AND(REL(D2, "eq", 2), REL(D3, "lt", 100)), dims=(), metrics=("count",), label="another literal, count alone"),
            c3(h, NO_FILTER, metrics=("m0",), label="GROUP BY d2, no filter, m0 alone")]


@pytest.mark.parametrize("which", ["two projections", "one projection"])
def test_mixed_members_are_fused(shared, one, which):
    h, filt = (shared, C3F) if which == "two projections" else (one, TWO)
    all8 = kinds(h, filt)
    assert 0.03 < all8[2].want.passed_recs / all8[2].want.scanned_recs < 0.08 or which == "one projection"
    for members in (all8[1:3], all8[4:6], all8[:3], all8[3:6], all8):
        for order in (members, members[::-1]):
            res, info = run_batch(h.dt, order, label=f"{which}, {len(order)} members")
            assert info.fused_groups == 1 and info.fused_members == len(order)


# ---- 2. per-member snapshots and skipped segments
def test_every_member_keeps_its_own_snapshot(shared):
    snaps = [[ROWS, ROWS, ROWS], [ROWS, 0, 4097], [1, 2048, 2049], [0, 0, 0]]
    members = [c3(shared, C3F, seg_rows=s, label="C3") for s in snaps] + [c3(shared, EVERY_ROW, seg_rows=s, label="every row passes") for s in snaps]
    res, _ = run_batch(shared.dt, members, label="four snapshots, twice")
    for r, s in zip(res[4:], snaps):
        assert r.passed_recs == sum(s) and r.scanned_recs == sum(s)
    assert all(r.scanned_segments == m.want.scanned_segments for r, m in zip(res, members))      # (a snapshot of no rows is not a skipped segment: the oracle counts it)
    totals = [c3(shared, NO_FILTER, dims=(), seg_rows=s, label="no filter") for s in snaps]
    res, _ = run_batch(shared.dt, totals[::-1], label="four snapshots, totals")
    assert [r.passed_recs for r in res] == [sum(s) for s in snaps[::-1]]


def test_a_segment_one_member_skips_and_the_others_scan(host):
    h = host
    seg = h.tab.segments[1]
    seg["d"][D3][:ROWS] = 500 + seg["d"][D3][:ROWS] % 500           # d3 < 447 holds for no row of segment 1: its min / max say so
    h.sync(1, 0, ROWS)
    members = [c3(h, TWO, label="segment 1 skipped"), c3(h, EVERY_ROW, label="every segment"), c3(h, AND(REL(D3, "lt", 447)), dims=(), label="segment 1 skipped, total"),
               c3(h, NO_FILTER, dims=(), label="every segment, total")]
    res, _ = run_batch(h.dt, members, label="min / max skip one member's segment")
    assert [r.scanned_segments for r in res] == [2, 3, 2, 3] and all(r.scanned_recs == NSEG * ROWS for r in res) and res[0].passed_recs > 0


# ---- 3. the small table: MIN / MAX / AVG / wrapping sums, 64 ids fused; 65 ids single; a group column that starts above 0
def small_member(t, dims, metrics, flt=None, fused=True, label=""):
    q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
    if flt is not None:
        q["filter"] = flt
    aq = vo.parse_query(t.tab, q)
    plan = dataclasses.replace(plan_from_query(t.tab, aq, flags=BASE), flags2=FLAG2)
    return Member(plan, vo.scan_aggregate(aq), fused, False, f"{label} by={list(dims)} metrics={list(metrics)}")


def test_the_small_table(small):
    t = small
    members = [small_member(t, ["a", "b"], ["um"], label="64 ids, uint_min"),
               small_member(t, ["c"], ["im", "zm", "av"], label="int_min, a MAX of zeros, AVG with the hidden count"),
               small_member(t, [], ["us"], label="uint_sum of 31-bit values: it wraps"),
               small_member(t, ["c", "e"], ["im"], fused=False, label="65 ids: beyond VH_PLANE_AGG_MAX_GROUPS"),
               small_member(t, ["a", "b"], ["um"], flt={"op": "and", "filters": [F("lt", "f", 500), F("ge", "a", 6)]}, label="64 ids under a filter on [a, b, f]"),
               small_member(t, ["e"], ["im"], label="int_min by e"),
               small_member(t, [], ["us"], flt=F("lt", "f", 500), label="uint_sum under a filter on another projection"),
               small_member(t, ["a"], ["lm"], fused=False, label="long_max by a column that starts at 5: the only candidate of its V")]
    res, info = run_batch(t.dt, members, groups=3, label="the small table: three V, a lone candidate, a plan of 65 ids")
    assert res[0].ngroups == 60 and res[3].ngroups > 50 and res[1].hidden_count is not None
    exact = sum(int(seg["m"][0][:ROWS].astype(np.uint64).sum()) for seg in t.tab.segments)
    assert exact > 1 << 32 and int(res[2].states[0][0]) == exact % (1 << 32)
    assert res[7].plane_agg and sorted(res[7].keys[0].tolist()) == [5, 6, 7, 8]                        # the lone candidate took the single kernel
    pair = [small_member(t, ["a"], ["lm"], label="long_max by a"), small_member(t, [], ["lm"], label="long_max"), small_member(t, [], ["ls"], fused=False, label="long_sum: its own V")]
    res, _ = run_batch(t.dt, pair, label="a group column with lo > 0, fused")
    assert sorted(res[0].keys[0].tolist()) == [5, 6, 7, 8] and int(res[2].states[0][0]) > 1 << 32


# ---- 4. mixed eligibility
def test_mixed_eligibility(shared):
    h = shared
    wide = c3(h, C3F, metrics=("m0", "m1", "count", "m4") * 5, fused=False, label="20 metrics: more than one pass carries")
    members = [c3(h, C3F, dims=(), label="total under C3's filter"),
               c3(h, C3F, metrics=("m3",), fused=False, label="a double metric"),
               c3(h, C3F, flags2=0, fused=False, label="no PLAN2_PLANE_AGG"),
               c3(h, EVERY_ROW, label="every row passes"),
               wide,
               c3(h, C3F, flags=capi.PLAN_FORCE_HASH, fused=False, label="FORCE_HASH"),
               c3(h, NO_FILTER, label="no filter")]
    res, _ = run_batch(h.dt, members, label="candidates among plans the rule refuses")
    assert len(res[4].states) == 20 and not res[2].plane_agg
    one_candidate = [dataclasses.replace(members[3], fused=False)]
    res, info = run_batch(h.dt, [members[1], one_candidate[0], members[2]], groups=0, label="exactly one candidate")
    assert info.fused_groups == 0 and res[1].plane_agg and res[1].kernel.startswith(KERNEL)
    res, info = run_batch(h.dt, one_candidate, groups=0, label="n == 1")
    assert info.nplans == 1 and info.singles == 1
    res, info = h.dt.query_agg_batch([])
    assert res == [] and (info.nplans, info.fused_groups, info.fused_members, info.singles) == (0, 0, 0, 0)


def test_a_group_column_with_granularity_is_answered_singly():
    from tests import time_edges as te
    tab = te._fill(vo.Table(te._schema([te._time_dim("ts", "time")])), [te._edge_columns("time")])
    dt = mirror_table(tab)
    try:
        aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "select": [{"column": "ts", "granularity": "year"}, {"column": "count"}]})
        want = vo.scan_aggregate(aq, now=te.NOW)
        plan = dataclasses.replace(plan_from_query(tab, aq, now=te.NOW, flags=BASE), flags2=FLAG2)
        run_batch(dt, [Member(plan, want, False, False, "GROUP BY ts truncated to years")] * 2, groups=0, label="a granularity")
    finally:
        dt.close()


# ---- 5. post stages: HAVING and top-N on fused members see their own groups
def test_post_stages(shared):
    h = shared
    every = c3(h, EVERY_ROW, label="every row passes")
    sums = sorted(int(x) for x in every.want.states[0])
    cut = sums[1]                                                   # two of the four groups have a larger sum
    having = Member(dataclasses.replace(every.plan, having=[("rel", 1, capi.OP_GT, cut)]), None, True, False, "HAVING sum(m0) > cut")
    top = Member(dataclasses.replace(every.plan, top=(1, True, 2)), None, True, False, "top 2 by sum(m0)")
    low = c3(h, C3F, label="C3")
    having_low = Member(dataclasses.replace(low.plan, having=[("rel", 2, capi.OP_GT, 10 ** 9)]), None, True, False, "HAVING that keeps no group of ITS member")
    res, _ = run_batch(h.dt, [having, every, top, having_low, low], label="HAVING and top-N among plain members")
    assert res[0].ngroups == 4 and res[0].returned == 2 and sorted(int(x) for x in res[0].states[0]) == sums[2:]
    assert res[2].ngroups == 4 and res[2].returned >= 2 and set(sums[2:]) <= set(int(x) for x in res[2].states[0])
    assert res[3].returned == 0 and res[3].ngroups == low.want.ngroups and res[4].returned == low.want.ngroups


# ---- 6. a value outside the planned range in ONE member: it comes back right through its re-plan, the others are fused
def test_one_member_is_planned_again():
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

        def member(dims, flt, plan=None, fused=True, label=""):
            q = {"type": "aggregate", "table": "t", "dimensions": dims, "metrics": ["v", "count"]}
            if flt is not None:
                q["filter"] = flt
            aq = vo.parse_query(tab, q)
            plan = dataclasses.replace(plan_from_query(tab, aq, flags=BASE), flags2=FLAG2) if plan is None else plan
            return Member(plan, vo.scan_aggregate(aq), fused, False, label)

        by_s = member(["s"], F("lt", "f", 800), label="GROUP BY s, three codes")
        assert by_s.plan.groups[0].cardinality == 3
        stale = by_s.plan
        run_batch(dt, [by_s, member([], F("lt", "f", 800), label="total"), member([], None, label="total, no filter")], label="three codes, three ids")
        dic.v2c["z"] = 3
        dic.c2v.append("z")
        seg = tab.segments[1]
        seg["d"][0][2048 + 31], seg["d"][1][2048 + 31] = 3, 0              # a fourth code in a row that passes; it fits the 2-bit field, the projections stay
        dt.sync_batch([(1, 2048 + 31, 1, ROWS, seg_columns(tab, seg), 0)])
        again = member(["s"], F("lt", "f", 800), plan=stale, fused=False, label="a fourth code behind the plan's back")      # the plan still says three ids
        assert again.want.ngroups == 4
        others = [member([], F("lt", "f", 800), label="total"), member(["s"], F("ge", "f", 800), label="GROUP BY s, planned with four ids"), member([], None, label="total, no filter")]
        res, info = run_batch(dt, [others[0], again, others[1], others[2]], groups=1, label="one member is planned again")
        assert res[1].path == "hash" and res[1].retries >= 1 and len(sliced_layouts(dt)) == 2
        assert info.fused_members == 3 and info.singles == 1
    finally:
        dt.close()


# ---- 7. after vh_table_sync_batch between two batches: appends and in-place updates
def test_batches_follow_the_syncs(host):
    h = host

    def members():
        return [c3(h, C3F, label="C3"), c3(h, EVERY_ROW, label="every row passes"), c3(h, NO_FILTER, dims=(), label="total, no filter"), c3(h, C3F, dims=(), label="C3 total")]
    before, _ = run_batch(h.dt, members(), label="before")
    h.change(1, 1000, 1500, flip=True)
    h.sync(1, 1000, 1500)
    changed, _ = run_batch(h.dt, members(), label="after a change of 1500 rows")
    assert changed[0].passed_recs != before[0].passed_recs
    h.append(2, 700)                                                # rows 5000 .. 5699: the word that held 8 rows fills up
    grown, _ = run_batch(h.dt, members(), label="after 700 appended rows")
    assert grown[1].scanned_recs == NSEG * ROWS + 700 == grown[1].passed_recs == grown[2].passed_recs


# ---- 8. VH_TEST_NO_BATCH_FUSE=1: the same batches answered singly, the same results
def batches_for_the_child(h):
    all8 = kinds(h, C3F)
    return [all8, all8[1:3][::-1], all8[3:6]]


def rows_of(r):
    o = np.lexsort([k for k in reversed(r.keys)]) if r.keys and len(r.keys[0]) else np.arange(r.returned)
    return {"keys": [k[o].tolist() for k in r.keys], "states": [s[o].tolist() for s in r.states], "counters": [r.ngroups, r.scanned_recs, r.scanned_segments, r.passed_recs, r.returned],
            "fused": r.batch_fused, "kernel": r.kernel}


CHILD = """
import json, sys
sys.path.insert(0, {root!r})
import tests.conftest
from viyadb_amd import executor
from tests import test_gpu_batch as tb
executor.init(0)
h = tb._host()
out = []
for members in tb.batches_for_the_child(h):
    res, info = h.dt.query_agg_batch([m.plan for m in members])
    out.append({{"info": [info.nplans, info.fused_groups, info.fused_members, info.singles], "rows": [tb.rows_of(r) for r in res]}})
print("RESULT " + json.dumps(out))
h.close()
"""


def test_the_hook_answers_every_member_singly(shared):
    env = dict(os.environ, VH_TEST_NO_BATCH_FUSE="1", VH_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    child = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    batches = batches_for_the_child(shared)
    assert len(child) == len(batches)
    for members, got in zip(batches, child):
        res, info = run_batch(shared.dt, members, label="the fused run")
        assert got["info"] == [len(members), 0, 0, len(members)]
        for r, m, c in zip(res, members, got["rows"]):
            mine = rows_of(r)
            assert not c["fused"] and c["kernel"].startswith(KERNEL) and mine["fused"], (m.label, c["kernel"])
            assert (c["keys"], c["states"], c["counters"]) == (mine["keys"], mine["states"], mine["counters"]), m.label


# ---- 9. all or nothing
def test_a_failing_member_fails_the_batch_and_leaks_nothing(shared):
    h = shared
    good = [c3(h, C3F, label="C3"), c3(h, EVERY_ROW, label="every row passes"), c3(h, NO_FILTER, dims=(), label="total"), c3(h, C3F, dims=(), label="C3 total")]
    plans = [good[0].plan, good[1].plan, good[0].plan, good[2].plan, good[3].plan]
    built = [h.dt._build_plan(p) for p in plans]
    assert built[2][0].nmetrics == 2
    built[2][0].metrics[1] = 99                                        # member 2: a metric column the table does not have
    ptrs = (C.POINTER(capi.Plan) * len(plans))(*[C.pointer(b[0]) for b in built])
    one_res = C.c_void_p()
    single_rc = h.dt.lib.vh_query_agg(h.dt.handle, C.byref(built[2][0]), C.byref(one_res))
    single_msg = h.dt.lib.vh_last_error().decode()
    assert single_rc != 0 and not one_res.value
    for attempt in range(17):                                          # more failures than VH_MAX_EXEC has contexts: none may stay behind
        out = (C.c_void_p * len(plans))(*[1] * len(plans))
        info = capi.BatchInfo()
        rc = h.dt.lib.vh_query_agg_batch(h.dt.handle, ptrs, len(plans), out, C.byref(info))
        msg = h.dt.lib.vh_last_error().decode()
        assert rc == single_rc and msg.startswith("plan 2: ") and msg[len("plan 2: "):] == single_msg[:len(msg) - len("plan 2: ")], (attempt, rc, msg, single_msg)
        assert all(out[i] is None for i in range(len(plans))), attempt
        assert info.nplans == 0
    eight = kinds(h, C3F)
    run_batch(h.dt, eight, label="eight members after seventeen failures")
    run_batch(h.dt, good, label="the table answers the next batch")


# ---- 10. one tick for the whole batch: a later member's build and the trim never take F or V from under a fused launch to come
def test_a_later_members_projection_does_not_evict_the_planes(host):
    h = host
    fused = [c3(h, C3F, label="C3"), c3(h, EVERY_ROW, label="every row passes")]
    packer = c3(h, C3F, dims=(0, 1), flags=capi.PLAN_FORCE_PACK, flags2=0, fused=False, label="FORCE_PACK: a payload projection is built for it")
    singles = [h.dt.query_agg(m.plan) for m in fused]
    planes = sliced_layouts(h.dt)
    assert len(planes) == 2
    for x in planes:                                                   # built by an explicit call, hence pinned: only unpinned layouts can be evicted at all
        h.dt.pin_layout(x.serial, False)
    h.dt.set_layout_budget(sum(x.bytes for x in planes) + 1)           # F and V fit; nothing fits beside them
    res, info = h.dt.query_agg_batch([fused[0].plan, packer.plan, fused[1].plan])
    lay, summ = h.dt.layouts()
    print("layouts after the batch:", [(x.kind, x.bytes) for x in lay], "budget", summ.budget, "bytes", summ.bytes, "evictions", summ.evictions, "packed", res[1].packed)
    assert {x.serial for x in planes} <= {x.serial for x in lay}, "F and V are still listed after the call"
    assert res[1].packed and summ.bytes > summ.budget          # the projection was built inside the batch, past the budget: the trim had every reason to evict
    assert (info.fused_groups, info.fused_members, info.singles) == (1, 2, 1)
    for r, m, s in zip([res[0], res[2]], fused, singles):
        compare(r, m.want, m.label)
        agree(r, s, m.label)
        assert r.batch_fused and r.flags & ~capi.INFO_EVICTED == s.flags | BIT30, (m.label, hex(r.flags), hex(s.flags))
    compare(res[1], packer.want, packer.label)
    assert not res[1].batch_fused
    evicted = [bool(r.flags & capi.INFO_EVICTED) for r in res]
    assert len(set(evicted)) == 1 and evicted[0] == (summ.evictions > 0), (evicted, summ.evictions)      # bit 24: on every result of the batch, or on none


# ---- 11. two threads, each running 20 batches of 4 on one table
def test_two_threads_run_batches_on_one_table(shared):
    h = shared
    members = kinds(h, C3F)
    sets = [[members[(i + k) % 8] for k in range(4)] for i in range(8)]
    errors = []

    def loop(tid):
        try:
            for it in range(20):
                ms = sets[(it + 3 * tid) % 8]
                res, info = h.dt.query_agg_batch([m.plan for m in ms])
                assert (info.fused_groups, info.fused_members) == (1, 4), (tid, it, info.fused_groups, info.fused_members)
                for r, m in zip(res, ms):
                    compare(r, m.want, f"thread {tid}, batch {it}: {m.label}")
                    assert r.batch_fused
        except Exception as e:   # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=loop, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:3]
