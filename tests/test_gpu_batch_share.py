"""Members of one fused launch that have the same pass mask evaluate it ONCE (vh_batch.h: vh_batch_share; VhBatchMember::mask_of;
vh_result_batch_member): the dashboard's shape, K breakdowns under one filter.

Tables and helpers are those of tests/test_gpu_batch.py and tests/test_gpu_plane_agg.py: C3Host(3, 5000, 8192) — two full 2048-row chunks and one
of 904 rows per segment, the last plane word holding 8 rows — with F = [d2, d3, d4] and V = [d2, m0, count], and the one-projection host
[d2, d3, m0, count]. Plans run under PLAN_NO_JIT | PLAN2_PLANE_AGG; nothing is compiled at run time.

EVERY member of every case goes through test_gpu_batch.check_member: the oracle over the host's arrays, bit-for-bit agreement with its single
query, flags = single | bit 30. On top of that each case asserts batch_member: fused, launch, position, members, mask_of and mask_classes. A
mask taken from the wrong member therefore fails twice — the assertion on mask_of, and the comparison with the oracle, because the near
misses are chosen so that their passed_recs differ from their neighbour's (asserted on the oracle's figures before anything runs)."""
import dataclasses
import json
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_agg_sliced import AND, OR, REL, SET
from tests.test_gpu_batch import (TWO, Member, _init, c3, host, one, rows_of, run_batch, shared)  # noqa: F401  (fixtures; run_batch sends every member through check_member)
from tests.test_gpu_layout_lifecycle import D2, D3, D4
from tests.test_gpu_plane_agg import BASE, C3F, CAP, FLAG2, NO_FILTER, NSEG, ROWS, F, _host
from tests.test_gpu_sync_batch import seg_columns
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("fused", "launch", "position", "members", "mask_of", "mask_classes")
C3B = AND(REL(D2, "eq", 1), REL(D3, "lt", 448), REL(D4, "ge", 553))      # C3's filter with one literal moved by one


def member_info(r):
    return tuple(int(getattr(r.batch_member, f)) for f in FIELDS)


def assert_share(res, mask_of, label=""):
    """mask_of: per member of the batch, the position it must report — None: not fused, all zeros. One fused launch."""
    fused = [w for w in mask_of if w is not None]
    classes, pos = len(set(fused)), 0
    for i, (r, w) in enumerate(zip(res, mask_of)):
        got = member_info(r)
        print(f"{label} member {i}: batch_member {dict(zip(FIELDS, got))}")
        if w is None:
            assert got == (0,) * 6 and not r.batch_fused, (label, i, got)
            continue
        assert got == (1, 0, pos, len(fused), w, classes), (label, i, got, (1, 0, pos, len(fused), w, classes))
        assert r.batch_fused
        pos += 1


def breakdowns(h, filt):
    """Eight different breakdowns under ONE filter: totals and GROUP BY d2 over m0 / count / both (in either order)."""
    out = []
    for metrics in (("m0", "count"), ("m0",), ("count",), ("count", "m0")):
        out.append(c3(h, filt, dims=(), metrics=metrics, label="total"))
        out.append(c3(h, filt, dims=(D2,), metrics=metrics, label="GROUP BY d2"))
    return out


# ---- 1. one filter, K breakdowns: K = 2, 3, 8 on both hosts, each in two member orders
@pytest.mark.parametrize("which", ["two projections", "one projection"])
def test_breakdowns_under_one_filter_share_one_mask(shared, one, which):
    h, filt = (shared, C3F) if which == "two projections" else (one, TWO)
    all8 = breakdowns(h, filt)
    assert 0 < all8[0].want.passed_recs < all8[0].want.scanned_recs
    for members in (all8[:2], all8[3:6], all8):
        for order in (members, members[::-1]):
            res, info = run_batch(h.dt, order, label=f"{which}, {len(order)} breakdowns")
            assert_share(res, [0] * len(order), f"{which}, K = {len(order)}")
            assert len({r.passed_recs for r in res}) == 1


# ---- 2. two filters interleaved, and members without a filter
def test_two_filters_and_no_filter_make_three_classes(shared):
    h = shared
    a, b, n = (lambda **kw: c3(h, C3F, label="A", **kw)), (lambda **kw: c3(h, C3B, label="B", **kw)), (lambda **kw: c3(h, NO_FILTER, label="none", **kw))
    members = [a(), b(dims=()), a(dims=(), metrics=("m0",)), n(dims=()), b(), n(metrics=("count",)), a(metrics=("count",))]
    assert members[0].want.passed_recs != members[1].want.passed_recs          # (a row with d3 == 447 passes B and not A)
    res, _ = run_batch(h.dt, members, label="A B A none B none A")
    assert_share(res, [0, 1, 0, 3, 1, 3, 0], "A B A none B none A")


# ---- 3. near misses that must NOT share, each next to a twin that does
def test_near_misses_in_the_program_do_not_share(shared):
    h = shared
    leaves = (REL(D2, "eq", 1), REL(D3, "lt", 447), REL(D4, "ge", 553))
    le = AND(REL(D2, "eq", 1), REL(D3, "le", 447), REL(D4, "ge", 553))
    members = [c3(h, C3F, label="A"), c3(h, C3F, dims=(), label="A's twin"), c3(h, C3B, label="d3 < 448"), c3(h, le, label="d3 <= 447"),
               c3(h, OR(*leaves), label="the leaves under OR"), c3(h, OR(*leaves), dims=(), metrics=("count",), label="... and its twin"),
               c3(h, AND(*leaves), metrics=("m0",), label="A again, behind the others")]
    passed = [m.want.passed_recs for m in members]
    assert passed[0] == passed[1] == passed[6] and passed[4] == passed[5] and len({passed[0], passed[2], passed[4]}) == 3, passed
    assert passed[3] == passed[2] != passed[0]                                  # (d3 <= 447 passes what d3 < 448 passes: equal masks, other programs)
    res, _ = run_batch(h.dt, members, label="near misses in the program")
    assert_share(res, [0, 0, 2, 3, 4, 4, 0], "near misses in the program")


def test_near_misses_in_the_snapshot_do_not_share(shared):
    h = shared
    lo = int(h.tab.segments[NSEG - 1]["d"][D3][ROWS - 8:ROWS].min())
    filt = AND(REL(D3, "ge", lo))                                    # every row of the last segment's 8-row word passes it, and not every row of the table
    full, one_less, in_word, short = None, [ROWS, ROWS, ROWS - 1], [ROWS, ROWS, ROWS - 5], [ROWS, 0, 2049]
    members = [c3(h, filt, seg_rows=full, label="the table's rows"), c3(h, filt, dims=(), seg_rows=[ROWS] * NSEG, label="the same rows, spelled out"),
               c3(h, filt, seg_rows=one_less, label="one row fewer in the last segment"), c3(h, filt, seg_rows=in_word, label="ends inside the 8-row word"),
               c3(h, filt, seg_rows=short, label="a short snapshot"), c3(h, filt, dims=(), metrics=("count",), seg_rows=short, label="... and its twin"),
               c3(h, filt, dims=(), metrics=("m0",), seg_rows=one_less, label="one row fewer, again")]
    passed = [m.want.passed_recs for m in members]
    assert passed[0] == passed[1] < NSEG * ROWS and passed[2] == passed[6] == passed[0] - 1 and passed[3] == passed[0] - 5 and passed[4] == passed[5] < passed[3], passed
    res, _ = run_batch(h.dt, members, label="near misses in the snapshot")
    assert_share(res, [0, 0, 2, 3, 4, 4, 2], "near misses in the snapshot")
    assert [r.passed_recs for r in res] == passed


# ---- 4. a set leaf's table is the member's own: identical twins evaluate for themselves
def test_identical_set_leaves_do_not_share(shared):
    h = shared
    held = np.unique(np.concatenate([seg["d"][D3][:ROWS] for seg in h.tab.segments]))
    values = [int(v) for v in held[::len(held) // 8][:8]]
    filt = AND(SET(D3, values, True, kind="inset"), REL(D2, "ne", 3))
    members = [c3(h, filt, sets=True, label="a set leaf on d3"), c3(h, filt, sets=True, label="the identical set leaf"), c3(h, filt, dims=(), sets=True, label="... as a total")]
    res, _ = run_batch(h.dt, members, label="identical set leaves")
    assert_share(res, [0, 1, 2], "identical set leaves")
    assert res[0].passed_recs == res[1].passed_recs == res[2].passed_recs > 0


# ---- 5. the class leader is planned again: it comes back as a single query's result, its follower stands on the leader's mask
def test_the_leader_is_planned_again_and_the_follower_stands():
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

        under = F("lt", "f", 800)
        by_s = member(["s"], under, label="GROUP BY s, three codes")
        stale = by_s.plan
        res, _ = run_batch(dt, [member([], None, label="total, no filter"), by_s, member([], under, label="total under the filter")], label="before the sync")
        assert_share(res, [0, 1, 1], "before the sync")
        dic.v2c["z"] = 3
        dic.c2v.append("z")
        seg = tab.segments[1]
        seg["d"][0][2048 + 31], seg["d"][1][2048 + 31] = 3, 0              # a fourth code in a row that passes; it fits the 2-bit field, the projections stay
        dt.sync_batch([(1, 2048 + 31, 1, ROWS, seg_columns(tab, seg), 0)])
        leader = member(["s"], under, plan=stale, fused=False, label="the leader: a fourth code behind the plan's back")
        assert leader.want.ngroups == 4
        members = [member([], None, label="total, no filter"), leader, member([], under, label="the follower: total under the leader's filter"),
                   member(["s"], F("ge", "f", 800), label="GROUP BY s under another filter, planned with four ids")]
        res, info = run_batch(dt, members, groups=1, label="the leader is planned again")
        assert res[1].retries >= 1 and member_info(res[1]) == (0,) * 6 and not res[1].batch_fused
        assert (info.fused_members, info.singles) == (3, 1)
        # the launch had four members and three masks; the leader held position 1 in it
        assert [member_info(r) for r in (res[0], res[2], res[3])] == [(1, 0, 0, 4, 0, 3), (1, 0, 2, 4, 1, 3), (1, 0, 3, 4, 3, 3)]
    finally:
        dt.close()


# ---- 6. after vh_table_sync_batch changed and appended rows: the same batch shares again, over the new state
def test_the_classes_follow_the_syncs(host):
    h = host

    def members():
        return [c3(h, C3F, label="C3"), c3(h, C3F, dims=(), label="C3 total"), c3(h, C3F, metrics=("m0",), label="C3, m0 alone"), c3(h, NO_FILTER, dims=(), label="total, no filter"),
                c3(h, NO_FILTER, metrics=("count",), label="count by d2, no filter")]
    want = [0, 0, 0, 3, 3]
    before, _ = run_batch(h.dt, members(), label="before")
    assert_share(before, want, "before")
    h.change(1, 1000, 1500, flip=True)
    h.sync(1, 1000, 1500)
    changed, _ = run_batch(h.dt, members(), label="after a change of 1500 rows")
    assert_share(changed, want, "after a change of 1500 rows")
    assert changed[0].passed_recs != before[0].passed_recs and changed[1].passed_recs == changed[0].passed_recs
    h.append(2, 700)                                                # rows 5000 .. 5699: the word that held 8 rows fills up
    grown, _ = run_batch(h.dt, members(), label="after 700 appended rows")
    assert_share(grown, want, "after 700 appended rows")
    assert grown[3].passed_recs == NSEG * ROWS + 700 == grown[4].passed_recs and grown[2].passed_recs == grown[0].passed_recs


# ---- 7. VH_TEST_NO_BATCH_SHARE=1: the fused launch with every member evaluating its own mask, the same rows
def batches_for_the_child(h):
    all8 = breakdowns(h, C3F)
    mixed = [c3(h, C3F, label="A"), c3(h, C3B, dims=(), label="B"), c3(h, C3F, dims=(), label="A"), c3(h, NO_FILTER, dims=(), label="none"), c3(h, NO_FILTER, label="none")]
    return [all8, all8[2:5], mixed]


CHILD = """
import json, sys
sys.path.insert(0, {root!r})
import tests.conftest
from viyadb_amd import executor
from tests import test_gpu_batch_share as ts
executor.init(0)
h = ts._host()
out = []
for members in ts.batches_for_the_child(h):
    res, info = h.dt.query_agg_batch([m.plan for m in members])
    out.append({{"info": [info.nplans, info.fused_groups, info.fused_members, info.singles], "rows": [ts.rows_of(r) for r in res],
                "member": [list(ts.member_info(r)) for r in res]}})
print("RESULT " + json.dumps(out))
h.close()
"""


def test_the_hook_makes_every_member_evaluate_its_own_mask(shared):
    env = dict(os.environ, VH_TEST_NO_BATCH_SHARE="1", VH_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    child = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    batches = batches_for_the_child(shared)
    shipped = [[0] * 8, [0] * 3, [0, 1, 0, 3, 3]]
    assert len(child) == len(batches)
    for members, got, mask_of in zip(batches, child, shipped):
        K = len(members)
        res, info = run_batch(shared.dt, members, label="the shipped run")
        assert_share(res, mask_of, "the shipped run")
        assert got["info"] == [K, 1, K, 0]
        assert got["member"] == [[1, 0, k, K, k, K] for k in range(K)], got["member"]
        for r, m, c in zip(res, members, got["rows"]):
            mine = rows_of(r)
            assert c["fused"] and mine["fused"] and c["kernel"] == mine["kernel"], (m.label, c["kernel"])
            assert (c["keys"], c["states"], c["counters"]) == (mine["keys"], mine["states"], mine["counters"]), m.label


# ---- 8. outside a fused launch
def test_outside_a_fused_launch_everything_is_zero(shared):
    h = shared
    single = h.dt.query_agg(c3(h, C3F).plan)
    assert single.plane_agg and member_info(single) == (0,) * 6
    members = [c3(h, C3F, label="A"), c3(h, C3F, flags2=0, fused=False, label="A without PLAN2_PLANE_AGG: answered singly"), c3(h, C3F, dims=(), label="A total")]
    res, _ = run_batch(h.dt, members, label="a single among fused members")
    assert_share(res, [0, None, 0], "a single among fused members")
    lone = [dataclasses.replace(members[0], fused=False)]
    res, _ = run_batch(h.dt, lone, groups=0, label="a lone candidate")
    assert_share(res, [None], "a lone candidate")
    lib = h.dt.lib
    info = capi.BatchMemberInfo()
    assert lib.vh_result_batch_member(None, C.byref(info)) == -1                # VH_E_INVALID
    p, keep = h.dt._build_plan(members[0].plan)
    r = C.c_void_p()
    capi.check(lib.vh_query_agg(h.dt.handle, C.byref(p), C.byref(r)))
    try:
        assert lib.vh_result_batch_member(r, None) == -1
        assert b"null argument" in lib.vh_last_error()
        assert lib.vh_result_batch_member(r, C.byref(info)) == 0 and [getattr(info, f) for f in FIELDS] == [0] * 6
    finally:
        lib.vh_result_free(r)
