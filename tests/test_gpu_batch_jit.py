"""Members of a batch that carry PLAN2_PLANE_JIT are answered by ONE kernel compiled for the BATCH SHAPE — the ordered list of the members'
shapes, who takes whose pass mask, the memory scope (viyadb_amd/csrc/vh_jit.hip writes the text, vh_jit_planes_batch.h is the frame; the rule:
include/viya_hip.h, vh_query_agg_batch and "Aggregates on the bit-sliced planes, compiled").

Tables are the smallest the suite has: C3Host(3, 5000, 8192) with F = [d2, d3, d4] and V = [d2, m0, count] — two full 2048-row chunks, one of
904 rows and a last plane word of 8 rows in every segment —, the one-projection host [d2, d3, m0, count], tests/test_gpu_plane_agg.py's
`Small` and three tables of tests/plane_shapes.py.

EVERY member of every batch is held to the oracle (tests.parity.compare) and, bit for bit, to its single query (`agree`: every state is an
integer). A member of a compiled fused launch has its single query's flags | bit 30 with bits 27 and 5 set, a kernel name with the
viya_jit_scan_ prefix that is the same across the launch and is not its single query's, its single query's sink, and the batch_member record
tests/test_gpu_batch_share.py expects of a pre-built launch. A batch shape costs a compile of 0.25 s and more: no test makes more than four,
and cases about data reuse a shape with other data."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import plane_shapes as S
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.planner import plan_from_query
from tests.test_gpu_agg_sliced import AND, REL, SET, agree
from tests.test_gpu_batch import Member
from tests.test_gpu_batch_share import C3B, assert_share, member_info
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from tests.test_gpu_plane_agg import C3F, CAP, COUNT, F, M0, METRIC, NO_FILTER, NSEG, ROWS, Small, _host
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
needs_jit = pytest.mark.skipif(JIT_OFF, reason="VH_JIT=off: no kernel is compiled, no batch shape either (the child of the last case runs that)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JIT2 = capi.PLAN2_PLANE_JIT
FORCED = 0 if JIT_OFF else capi.PLAN_FORCE_JIT
BIT30, BIT27, BIT5, BIT19 = capi.INFO_BATCH_FUSED, capi.INFO_PLANE_AGG, capi.INFO_JIT, capi.INFO_BUILD_PENDING
COMPILED = "viya_jit_scan_"
PREBUILT_BATCH = "scan_agg_planes_batch_kernel<256, "
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


def c3(h, filt, dims=(D2,), metrics=("m0", "count"), flags=FORCED, flags2=JIT2, seg_rows=None, fused=True, sets=False, label=""):
    nodes, qfilter = filt
    q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics)}
    if qfilter is not None:
        q["filter"] = qfilter
    want = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    plan = AggPlan(filter=nodes, groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics], flags=flags, flags2=flags2, seg_rows=seg_rows)
    return Member(plan, want, fused, sets, f"{label} by={list(dims)} metrics={list(metrics)} snapshot={seg_rows}")


def check_member(dt, r, m):
    single = dt.query_agg(m.plan)
    print(f"{m.label}: fused {r.batch_fused}, flags {r.flags:#x} / single {single.flags:#x}, passed {r.passed_recs}, groups {r.ngroups}, kernel {r.kernel} / {single.kernel}")
    compare(r, m.want, m.label + " [batch]")
    compare(single, m.want, m.label + " [single]")
    agree(r, single, m.label)
    assert r.returned == single.returned and r.passed_recs == m.want.passed_recs, (m.label, r.returned, single.returned, r.passed_recs)
    assert r.batch_fused == m.fused, (m.label, hex(r.flags), r.kernel)
    if not m.fused:
        assert r.flags == single.flags and r.kernel == single.kernel and member_info(r) == (0,) * 6, (m.label, hex(r.flags), hex(single.flags), r.kernel, single.kernel)
        return single
    assert r.flags == single.flags | BIT30, (m.label, hex(r.flags), hex(single.flags))
    assert r.plane_sink == single.plane_sink and r.plane_sink in (1, 2), (m.label, r.plane_sink, single.plane_sink)
    assert r.scan_kernel_ms > 0
    if m.plan.flags2 & JIT2:          # a compiled fused launch
        assert r.flags & BIT27 and r.flags & BIT5 and r.batch_compiled and r.plane_jit, (m.label, hex(r.flags))
        assert r.kernel.startswith(COMPILED) and single.kernel.startswith(COMPILED) and r.kernel != single.kernel, (m.label, r.kernel, single.kernel)
    else:                             # a pre-built one
        assert r.flags & BIT27 and not r.flags & BIT5 and not r.batch_compiled and r.kernel.startswith(PREBUILT_BATCH), (m.label, hex(r.flags), r.kernel)
    return single


def run_batch(dt, members, mask_of=None, groups=1, compiled=1, label=""):
    """One batch; every member through check_member. mask_of: what ONE fused launch must report per member (None: answered singly)."""
    res, info = dt.query_agg_batch([m.plan for m in members])
    nf = sum(m.fused for m in members)
    print(f"{label}: {info.nplans} plans, {info.fused_groups} fused launch(es), {info.compiled_groups} of them compiled, {info.fused_members} members, "
          f"{info.singles} single, {info.fused_kernel_ms:.4f} ms")
    assert (info.nplans, info.fused_groups, info.compiled_groups, info.fused_members, info.singles) == (len(members), groups, compiled, nf, len(members) - nf), \
        (label, info.fused_groups, info.compiled_groups, info.fused_members, info.singles)
    for r, m in zip(res, members):
        check_member(dt, r, m)
    if mask_of is not None:
        assert_share(res, mask_of, label)
        assert len({r.kernel for r, w in zip(res, mask_of) if w is not None}) == (1 if groups else 0), [r.kernel for r in res]
    return res, info


def breakdowns(h, filt):
    """Eight different breakdowns under ONE filter: totals and GROUP BY d2 over m0 / count / both (in either order)."""
    out = []
    for metrics in (("m0", "count"), ("m0",), ("count",), ("count", "m0")):
        out.append(c3(h, filt, dims=(), metrics=metrics, label="total"))
        out.append(c3(h, filt, dims=(D2,), metrics=metrics, label="GROUP BY d2"))
    return out


# ---- 1. K breakdowns under one filter: one compiled launch, one mask class; both hosts, K = 2, 3, 8, each in two member orders
@needs_jit
@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("which", ["two projections", "one projection"])
def test_breakdowns_under_one_filter(shared, one, which, K):
    h, filt = (shared, C3F) if which == "two projections" else (one, TWO)
    all8 = breakdowns(h, filt)
    assert 0 < all8[0].want.passed_recs < all8[0].want.scanned_recs
    members = {2: all8[:2], 3: all8[3:6], 8: all8}[K]
    names = set()
    for order in (members, members[::-1]):
        res, info = run_batch(h.dt, order, [0] * K, label=f"{which}, {K} breakdowns")
        assert info.compiled_groups == 1 and len({r.passed_recs for r in res}) == 1
        names.add(res[0].kernel)
    assert len(names) == 2, names                 # the members' order is part of the shape


# ---- 2. data is not shape: other literals and other snapshots under one kernel, without another compile
def _twice(dt, first, second, mask_of, label):
    a, _ = run_batch(dt, first, mask_of, label=label + ", first")
    before = dt.build_info().inline_builds
    res, info = dt.query_agg_batch([m.plan for m in second])
    assert dt.build_info().inline_builds == before, (label, before, dt.build_info().inline_builds)      # nothing was compiled for the second batch
    assert info.compiled_groups == 1
    b, _ = run_batch(dt, second, mask_of, label=label + ", second")
    assert {r.kernel for r in a} == {r.kernel for r in b} == {res[0].kernel}, (label, a[0].kernel, b[0].kernel, res[0].kernel)
    assert [r.passed_recs for r in res] == [m.want.passed_recs for m in second]
    return a, b


@needs_jit
def test_data_is_not_shape(shared):
    h = shared
    first = [c3(h, C3F, label="C3"), c3(h, C3F, dims=(), label="C3 total"), c3(h, C3B, label="d3 < 448")]
    second = [c3(h, C3B, label="d3 < 448"), c3(h, C3B, dims=(), label="d3 < 448 total"), c3(h, C3F, label="C3")]
    assert first[0].want.passed_recs != second[0].want.passed_recs              # (a row with d3 == 447 passes d3 < 448 and not C3's filter)
    _twice(h.dt, first, second, [0, 0, 2], "other literals")
    # the near-miss snapshots of test_near_misses_in_the_snapshot_do_not_share, where they give the same mask_of vector
    lo = int(h.tab.segments[NSEG - 1]["d"][D3][ROWS - 8:ROWS].min())
    filt = AND(REL(D3, "ge", lo))
    one_less, in_word, short = [ROWS, ROWS, ROWS - 1], [ROWS, ROWS, ROWS - 5], [ROWS, 0, 2049]
    first = [c3(h, filt, seg_rows=None, label="the table's rows"), c3(h, filt, dims=(), seg_rows=[ROWS] * NSEG, label="the same rows, spelled out"),
             c3(h, filt, seg_rows=one_less, label="one row fewer in the last segment")]
    second = [c3(h, filt, seg_rows=short, label="a short snapshot"), c3(h, filt, dims=(), seg_rows=short, label="... and its twin"),
              c3(h, filt, seg_rows=in_word, label="ends inside the 8-row word")]
    p1, p2 = [m.want.passed_recs for m in first], [m.want.passed_recs for m in second]
    assert p1[0] == p1[1] == p1[2] + 1 and p2[0] == p2[1] < p2[2] == p1[0] - 5, (p1, p2)
    _twice(h.dt, first, second, [0, 0, 2], "other snapshots")


# ---- 3. classes
@needs_jit
def test_two_filters_and_no_filter_make_three_classes(shared):
    h = shared
    a, b, n = (lambda **kw: c3(h, C3F, label="A", **kw)), (lambda **kw: c3(h, C3B, label="B", **kw)), (lambda **kw: c3(h, NO_FILTER, label="none", **kw))
    members = [a(), b(dims=()), a(dims=(), metrics=("m0",)), n(dims=()), b(), n(metrics=("count",)), a(metrics=("count",))]
    assert members[0].want.passed_recs != members[1].want.passed_recs
    run_batch(h.dt, members, [0, 1, 0, 3, 1, 3, 0], label="A B A none B none A")


@needs_jit
def test_identical_set_leaves_do_not_share_and_their_tables_are_data(shared):
    h = shared
    held = np.unique(np.concatenate([seg["d"][D3][:ROWS] for seg in h.tab.segments]))
    passed, names = [], set()
    for values in ([int(v) for v in held[::len(held) // 8][:8]], [int(v) for v in held[3::len(held) // 5][:5]]):
        filt = AND(SET(D3, values, True, kind="inset"), REL(D2, "ne", 3))
        members = [c3(h, filt, sets=True, label="a set leaf on d3"), c3(h, filt, sets=True, label="the identical set leaf"), c3(h, filt, dims=(), sets=True, label="... as a total")]
        res, _ = run_batch(h.dt, members, [0, 1, 2], label=f"identical set leaves of {len(values)} values")
        assert res[0].passed_recs == res[1].passed_recs == res[2].passed_recs > 0
        passed.append(res[0].passed_recs)
        names.add(res[0].kernel)
    assert passed[0] != passed[1] and len(names) == 1, (passed, names)          # other members of the set, the same code object


# ---- 4. a row-sink member among loop members
def small_member(t, dims, metrics, flt=None, rows2=0, label=""):
    q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
    if flt is not None:
        q["filter"] = flt
    aq = vo.parse_query(t.tab, q)
    plan = dataclasses.replace(plan_from_query(t.tab, aq, flags=FORCED), flags2=JIT2 | rows2)
    return Member(plan, vo.scan_aggregate(aq), True, False, f"{label} by={list(dims)} metrics={list(metrics)}")


@needs_jit
def test_a_row_sink_member_among_loop_members(small):
    t = small
    for flt, label in ((None, "every row passes"), (F("ge", "c", 11), "a sparse filter: the two planted rows")):
        members = [small_member(t, ["c"], ["im", "zm", "av"], flt, label="13 ids: the loop"),
                   small_member(t, ["c", "e"], ["im"], flt, rows2=capi.PLAN2_PLANE_ROWS, label="65 ids: the row sink"),
                   small_member(t, [], ["im"], flt, label="the total"),
                   small_member(t, ["e"], ["im"], flt, label="5 ids: the loop")]
        res, _ = run_batch(t.dt, members, [0, 0, 0, 0], label=label)
        assert [r.plane_sink for r in res] == [1, 2, 1, 1]
        assert res[0].passed_recs == (NSEG * ROWS if flt is None else 2)
        assert res[1].ngroups > 50 if flt is None else res[1].ngroups == 2


# ---- 5. field edges: a field that ends at plane 31, the single 32-plane field, signed MIN / MAX kinds; literals held at bit 0, bit 31 and in the 8-row word
@needs_jit
@pytest.mark.parametrize("shape", ["bytes", "long32"])
def test_fields_at_the_top_plane(shape):
    h = S.ShapeHost(shape)
    try:
        col = "d" if shape == "bytes" else "l"          # bytes: d is planes 24 .. 31; long32: l is all 32
        top = str(S.column(shape, col)[3])
        cases = [S.composite(shape, "and"), S.composite(shape, "nest")]
        rels = [S._rel(shape, col, op, top) for op in ("eq", "lt")]          # the top value is planted at bit 0, at bit 31 and in the 8-row word of every segment
        members = []
        for nodes, query, label in [(c.nodes, c.query, c.label) for c in cases] + [([r[0]], r[1], f"{shape}: {col} {r[1]['op']} {top}") for r in rels]:
            metrics = ("v", "count") if len(members) % 2 == 0 else ("count",)
            plan = AggPlan(filter=nodes, groups=[], metrics=[h.index[m] for m in metrics], flags=FORCED, flags2=JIT2)
            members.append(Member(plan, h.want(query, (), metrics), True, False, label))
        if shape == "bytes":
            # four mask classes of 32 + 16 + 8 + 8 filter planes: exactly the 64 a batch shape may read
            res, _ = run_batch(h.dt, members, [0, 1, 2, 3], label="bytes: four filters, 64 filter planes")
        else:
            # every filter reads all 32 planes of l: four classes are 128 planes, no batch shape — each member runs its own compiled kernel ...
            singly = [dataclasses.replace(m, fused=False) for m in members]
            run_batch(h.dt, singly, [None] * 4, groups=0, compiled=0, label="long32: four filters, 128 filter planes")
            # ... and two classes are the 64 that fit: the AND twice, under one mask, and `== top`
            again = dataclasses.replace(members[0], plan=dataclasses.replace(members[0].plan, metrics=[h.index["count"]]), want=h.want(cases[0].query, (), ("count",)))
            members = [members[0], again, members[2]]
            res, _ = run_batch(h.dt, members, [0, 0, 2], label="long32: two classes, 64 filter planes")
        assert all(0 < r.passed_recs < r.scanned_recs for r in res), [r.passed_recs for r in res]
        assert res[2].passed_recs >= 3 * 2                                   # `== top`: the planted rows at least (two segments hold all three)
    finally:
        h.close()


@needs_jit
def test_signed_min_max_kinds():
    h = S.ShapeHost("values")
    try:
        case = S.composite("values", "and")
        members = []
        for dims, metrics in ((("g",), ("mx", "sm")), ((), ("mx", "sm")), (("g",), ("lm",)), ((), ("lm",))):
            plan = AggPlan(filter=case.nodes, groups=[GroupSpec(h.index[d]) for d in dims], metrics=[h.index[m] for m in metrics], flags=FORCED, flags2=JIT2)
            members.append(Member(plan, h.want(case.query, dims, metrics), True, False, f"values: {case.label} by={dims} metrics={metrics}"))
        # two value projections, [g, h, mx, sm] and [g, lm]: two compiled launches of two members each, one mask class in each
        res, info = run_batch(h.dt, members, None, groups=2, compiled=2, label="values: ushort_max, int_sum and long_max")
        assert [member_info(r) for r in res] == [(1, 0, 0, 2, 0, 1), (1, 0, 1, 2, 0, 1), (1, 1, 0, 2, 0, 1), (1, 1, 1, 2, 0, 1)]
        assert res[0].kernel == res[1].kernel != res[2].kernel == res[3].kernel
    finally:
        h.close()


# ---- 6. a mixed batch: compiled candidates, pre-built candidates, a plan that is no candidate
@needs_jit
def test_a_mixed_batch(shared):
    h = shared
    pre = dict(flags=capi.PLAN_NO_JIT, flags2=capi.PLAN2_PLANE_AGG)
    members = [c3(h, C3F, label="compiled"), c3(h, C3F, label="pre-built", **pre), c3(h, C3F, dims=(), flags=capi.PLAN_NO_JIT, flags2=0, fused=False, label="no candidate"),
               c3(h, C3F, dims=(), label="compiled total"), c3(h, NO_FILTER, dims=(), label="pre-built total, no filter", **pre)]
    for _ in range(8):          # (the table narrows and packs columns unasked after a few scans of one kind: let the single's plan settle first)
        h.dt.query_agg(members[2].plan)
    res, info = run_batch(h.dt, members, None, groups=2, compiled=1, label="two kinds and a single")
    assert (info.fused_groups, info.compiled_groups, info.singles) == (2, 1, 1)
    assert [member_info(r) for r in res] == [(1, 0, 0, 2, 0, 1), (1, 1, 0, 2, 0, 2), (0,) * 6, (1, 0, 1, 2, 0, 1), (1, 1, 1, 2, 1, 2)]
    assert res[0].kernel == res[3].kernel and res[0].kernel.startswith(COMPILED) and res[1].kernel == res[4].kernel and res[1].kernel.startswith(PREBUILT_BATCH)
    # a lone compiled candidate is the single compiled query it is
    lone = [dataclasses.replace(members[0], fused=False), members[1], members[4]]
    res, _ = run_batch(h.dt, lone, None, groups=1, compiled=0, label="a lone compiled candidate")
    assert res[0].kernel.startswith(COMPILED) and res[0].plane_jit and not res[0].batch_fused


# ---- 7. VH_JIT=off, in a child: the flag's members are single queries of the pre-built plane kernel
CHILD = """
import json, sys
sys.path.insert(0, {root!r})
import tests.conftest
from viyadb_amd import executor
from tests import test_gpu_batch_jit as tj
from tests.parity import compare
executor.init(0)
assert tj.JIT_OFF
h = tj._host()
members = tj.breakdowns(h, tj.C3F)[3:6]
res, info = h.dt.query_agg_batch([m.plan for m in members])
for r, m in zip(res, members):
    compare(r, m.want, m.label)
print("RESULT " + json.dumps({{"info": [info.nplans, info.fused_groups, info.compiled_groups, info.fused_members, info.singles],
                              "flags": [r.flags for r in res], "kernel": [r.kernel for r in res], "passed": [r.passed_recs for r in res],
                              "want": [m.want.passed_recs for m in members]}}))
h.close()
"""


def test_under_jit_off_nothing_is_compiled():
    env = {k: v for k, v in os.environ.items() if k not in ("VH_PLANE_AGG", "VH_PLANE_JIT")}
    env.update(VH_JIT="off", VH_TEST_HOOKS="1")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["info"] == [3, 0, 0, 0, 3], got["info"]                # three singles: a member that asked and has no kernel is no candidate
    assert got["passed"] == got["want"]
    for flags, kernel in zip(got["flags"], got["kernel"]):
        assert flags & BIT27 and not flags & BIT5 and not flags & BIT30 and kernel.startswith("scan_agg_planes_kernel<"), (hex(flags), kernel)


# ---- 8. background build mode: while the batch kernel is not at hand the members answer for themselves
@needs_jit
def test_on_a_background_table(host, monkeypatch):
    h = host
    # shapes no other test of this file puts into a batch, and member shapes no test of ANY file compiles — tests/test_gpu_plane_jit.py's
    # background case runs later in the same process and counts on ITS four-leaf shape (ne, le, gt, ne) being new to the process
    four = AND(REL(D2, "ne", 2), REL(D3, "ge", 100), REL(D4, "lt", 900), REL(D3, "ne", 7))
    members = [c3(h, four, metrics=("count",), label="count by d2"), c3(h, four, dims=(), metrics=("m0",), label="m0 in all"), c3(h, NO_FILTER, dims=(), metrics=("count",), label="count in all, no filter")]
    h.dt.set_build_mode(True)
    monkeypatch.setenv("VH_TEST_BUILD_HOLD", "start")
    try:
        res, info = h.dt.query_agg_batch([m.plan for m in members])          # the worker starts nothing: whatever has to be compiled is pending
        for r, m in zip(res, members):
            compare(r, m.want, m.label + " [held]")
            assert r.flags & BIT19 and not r.flags & BIT30 and r.flags & BIT27, (m.label, hex(r.flags), r.kernel)
            # its own compiled kernel where this process has it already, the pre-built plane kernel while that is pending too
            assert (r.kernel.startswith(COMPILED) and r.flags & BIT5) or (r.kernel.startswith("scan_agg_planes_kernel<") and not r.flags & BIT5), (hex(r.flags), r.kernel)
        assert info.compiled_groups == 0 and info.fused_groups == 0 and info.singles == 3
        monkeypatch.delenv("VH_TEST_BUILD_HOLD")
        fused = False
        for attempt in range(3):      # the members' own kernels first (if they were pending), then the batch kernel, which is asked for once those exist
            bi = h.dt.build_wait(120000)
            assert bi.jobs_queued == 0 and bi.jobs_running == 0 and bi.jobs_failed == 0, (bi.jobs_queued, bi.jobs_running, bi.jobs_failed)
            res, info = h.dt.query_agg_batch([m.plan for m in members])
            for r, m in zip(res, members):
                compare(r, m.want, m.label + f" [released, batch {attempt}]")
            fused = info.compiled_groups == 1
            if fused:
                break
            assert all(r.flags & BIT19 and r.flags & BIT5 and not r.flags & BIT30 and r.kernel.startswith(COMPILED) for r in res), [(hex(r.flags), r.kernel) for r in res]
        assert fused and attempt <= 1, attempt
        assert h.dt.build_info().inline_builds == 0
        run_batch(h.dt, members, [0, 0, 2], label="after the worker is done")
        assert not any(r.flags & BIT19 for r in res)
    finally:
        monkeypatch.delenv("VH_TEST_BUILD_HOLD", raising=False)
        h.dt.set_build_mode(False)


# ---- 9. a sync_batch of changed and appended rows between two batches of one shape
@needs_jit
def test_batches_follow_the_syncs(host):
    h = host

    def members():
        return [c3(h, C3F, label="C3"), c3(h, C3F, dims=(), label="C3 total"), c3(h, NO_FILTER, dims=(), label="total, no filter"), c3(h, NO_FILTER, metrics=("count",), label="count by d2, no filter")]
    want = [0, 0, 2, 2]
    before, _ = run_batch(h.dt, members(), want, label="before")
    h.change(1, 1000, 1500, flip=True)
    h.sync(1, 1000, 1500)
    h.append(2, 700)                                                # rows 5000 .. 5699: the word that held 8 rows fills up
    after, _ = run_batch(h.dt, members(), want, label="after 1500 changed and 700 appended rows")
    assert after[0].passed_recs != before[0].passed_recs and after[2].passed_recs == NSEG * ROWS + 700 == after[3].passed_recs
    assert after[0].kernel == before[0].kernel
