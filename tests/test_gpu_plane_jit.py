"""The aggregate ON the bit-sliced planes by a kernel COMPILED for the plan's shape (PLAN2_PLANE_JIT in vh_plan.flags2, or VH_PLANE_JIT=1 for a
process; the generator is viyadb_amd/csrc/vh_jit.hip, the frame vh_jit_planes.h; the rule: include/viya_hip.h, "Aggregates on the bit-sliced
planes, compiled").

Tables are those of tests/test_gpu_plane_agg.py — three segments of 5000 rows at capacity 8192: two whole 2048-row chunks, one of 904 rows and
a last plane word of 8 rows in every segment — and two of tests/plane_shapes.py.

Every case runs THREE queries: the plan with PLAN2_PLANE_JIT | PLAN_FORCE_JIT (plus PLAN2_PLANE_ROWS where the case has more than 64 ids),
twin 1 with PLAN_NO_JIT | PLAN2_PLANE_AGG (the pre-built plane kernel) and twin 2 with no flag at all. All three equal the oracle
(tests/parity.compare) and each other bit for bit: every state is an integer. Where the rule holds the flagged run has bits 27 and 5 with
bits 4 / 11 / 13, bits 0 / 1 / 26 clear, plane_sink 1 or 2 as the id count says, and the compiled kernel's name; where it does not, its flags
and kernel equal those of the same plan without PLAN2_PLANE_JIT."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import plane_shapes as S
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_agg_sliced import AND, REL, SET, agree
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from tests.test_gpu_plane_agg import (C3F, COUNT, EVERY_ROW, F, M0, METRIC, NO_FILTER, NSEG, ROWS, CAP, Small, sliced_layouts)
from tests.test_gpu_sync_batch import seg_columns
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
needs_jit = pytest.mark.skipif(JIT_OFF, reason="VH_JIT=off: no per-query kernel is compiled")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JIT2 = capi.PLAN2_PLANE_JIT
BIT27, BIT5 = capi.INFO_PLANE_AGG, capi.INFO_JIT
ON_PLANES = capi.INFO_ON_PLANES
OFF = capi.INFO_FAST | capi.INFO_LANES | capi.INFO_SLICED_PREBUILT      # bits 0, 1 and 26
SETS = capi.INFO_INSET | capi.INFO_INSET_SLICED
COMPILED = "viya_jit_scan_"
PREBUILT = "scan_agg_planes_"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _host(one=False):
    h = C3Host(NSEG, ROWS, CAP)
    if one:
        h.dt.predpack([D2, D3, M0, COUNT], sliced=True)       # V = F
    else:
        h.dt.predpack([D2, D3, D4], sliced=True)              # F
        h.dt.predpack([D2, M0, COUNT], sliced=True)           # V
    return h


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
    h = _host(one=True)
    yield h
    h.close()


@pytest.fixture(scope="module")
def small():
    t = Small()
    yield t
    t.close()


def run3(dt, plan, want, on, sets=False, rows2=0, label=""):
    """The flagged plan and its two twins -> the flagged run. on: 0 the rule does not hold, 1 the loop over ids, 2 the row sink."""
    base = dataclasses.replace(plan, flags=plan.flags & ~(capi.PLAN_NO_JIT | capi.PLAN_FORCE_JIT))
    forced = 0 if JIT_OFF else capi.PLAN_FORCE_JIT
    j = dt.query_agg(dataclasses.replace(base, flags=base.flags | forced, flags2=JIT2 | rows2))
    t1 = dt.query_agg(dataclasses.replace(base, flags=base.flags | capi.PLAN_NO_JIT, flags2=capi.PLAN2_PLANE_AGG | rows2))
    t2 = dt.query_agg(base)
    print(f"{label}: flags {j.flags:#x} / {t1.flags:#x} / {t2.flags:#x}, passed {j.passed_recs}, groups {j.ngroups}, kernel {j.kernel} / {t1.kernel} / {t2.kernel}")
    for res, who in ((j, "compiled on the planes"), (t1, "pre-built on the planes"), (t2, "no flag")):
        compare(res, want, f"{label} [{who}]")
    agree(j, t1, label)
    agree(j, t2, label)
    assert bool(t1.flags & BIT27) == bool(on) and not t1.flags & BIT5 and not t2.flags & BIT27, (label, hex(t1.flags), hex(t2.flags))
    if on and not JIT_OFF:
        assert j.flags & BIT27 and j.flags & BIT5 and j.jit and j.plane_agg and j.plane_jit, (label, hex(j.flags), j.kernel)
        assert j.flags & ON_PLANES == ON_PLANES and not j.flags & OFF, (label, hex(j.flags))
        assert j.flags & SETS == (SETS if sets else 0), (label, hex(j.flags))
        assert j.flags & ~BIT5 == t1.flags, (label, hex(j.flags), hex(t1.flags))                    # bit 27's word plus bit 5
        assert j.plane_sink == on == t1.plane_sink, (label, j.plane_sink, t1.plane_sink)
        assert j.kernel.startswith(COMPILED) and t1.kernel.startswith(PREBUILT), (label, j.kernel, t1.kernel)
    elif on:            # VH_JIT=off: the pre-built plane kernel answers the flag
        assert j.flags == t1.flags and j.kernel == t1.kernel and j.plane_sink == on, (label, hex(j.flags), j.kernel)
    else:               # the flag changes nothing: the same plan without it, run right before and right after (the table builds layouts unasked
        plain = dataclasses.replace(base, flags=base.flags | forced, flags2=rows2)      # after a few queries of one kind: a neighbour sees the same ones)
        w1, j2, w2 = dt.query_agg(plain), dt.query_agg(dataclasses.replace(plain, flags2=JIT2 | rows2)), dt.query_agg(plain)
        agree(j2, j, label)
        assert (j2.flags, j2.kernel) in ((w1.flags, w1.kernel), (w2.flags, w2.kernel)), (label, hex(j2.flags), hex(w1.flags), hex(w2.flags), j2.kernel, w1.kernel, w2.kernel)
        assert j.plane_sink == j2.plane_sink == 0 and not j.plane_agg and not j2.plane_agg, (label, hex(j.flags), hex(j2.flags))
    return j


def c3(h, filt, dims=(D2,), metrics=("m0", "count"), flags=0, seg_rows=None, on=1, sets=False, label=""):
    nodes, qfilter = filt
    q = {"type": "aggregate", "table": "synth", "dimensions": [f"d{c}" for c in dims], "metrics": list(metrics)}
    if qfilter is not None:
        q["filter"] = qfilter
    want = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    plan = AggPlan(filter=nodes, groups=[GroupSpec(c) for c in dims], metrics=[METRIC[m] for m in metrics], flags=flags, seg_rows=seg_rows)
    return run3(h.dt, plan, want, on, sets, label=f"{label} by={list(dims)} metrics={list(metrics)} snapshot={seg_rows}")


def small3(t, dims, metrics, flt=None, on=1, rows2=0, label=""):
    q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
    if flt is not None:
        q["filter"] = flt
    aq = vo.parse_query(t.tab, q)
    return run3(t.dt, plan_from_query(t.tab, aq), vo.scan_aggregate(aq), on, rows2=rows2, label=f"{label} by={list(dims)} metrics={list(metrics)}")


# ---- 1. totals and GROUP BY d2: no filter, C3's filter, every row; F != V and V = F
def test_forms_with_two_projections(shared):
    h = shared
    for dims in ((), (D2,)):
        a = c3(h, NO_FILTER, dims=dims, label="no filter")
        assert a.passed_recs == NSEG * ROWS
        a = c3(h, C3F, dims=dims, label="C3")
        assert 0.03 < a.passed_recs / a.scanned_recs < 0.08
        a = c3(h, EVERY_ROW, dims=dims, label="every row passes")
        assert a.passed_recs == a.scanned_recs == NSEG * ROWS


def test_forms_with_one_projection(one):
    h = one
    two = AND(REL(D2, "eq", 1), REL(D3, "lt", 447))
    for dims in ((), (D2,)):
        c3(h, NO_FILTER, dims=dims, label="V = F, no filter")
        a = c3(h, two, dims=dims, label="V = F")
        assert 0 < a.passed_recs < a.scanned_recs
        a = c3(h, EVERY_ROW, dims=dims, label="V = F, every row passes")
        assert a.passed_recs == NSEG * ROWS
    c3(h, C3F, on=0, label="V = F lacks d4: a filter column outside F")


# ---- 2. set leaves
def test_set_leaves(shared):
    h = shared
    held = np.unique(np.concatenate([seg["d"][D4][:ROWS] for seg in h.tab.segments]))
    values = [int(v) for v in held[::len(held) // 8][:8]]
    for equal in (True, False):
        a = c3(h, AND(SET(D4, values, equal, kind="inset"), REL(D2, "ne", 3)), sets=True, label=f"a set leaf on d4 (10-bit field), {'IN' if equal else 'NOT IN'}")
        assert 0 < a.passed_recs < a.scanned_recs


# ---- 3. the Small table: lo above 0, 64 and 65 ids, wrapping sums, MIN / MAX of every kind, AVG with the hidden count
def test_groups_and_the_two_sinks(small):
    a = small3(small, ["a"], ["lm"], label="a group column whose values start at 5")
    assert a.ngroups == 4 and sorted(a.keys[0].tolist()) == [5, 6, 7, 8]
    a = small3(small, ["a", "b"], ["um"], rows2=capi.PLAN2_PLANE_ROWS, label="64 ids with PLANE_ROWS: the last plan of the loop")
    assert a.ngroups == 4 * 15
    a = small3(small, ["a", "b"], ["um"], flt={"op": "and", "filters": [F("lt", "f", 500), F("ge", "a", 6)]}, label="64 ids under a filter on F = [a, b, f]")
    assert 0 < a.passed_recs < a.scanned_recs
    a = small3(small, ["c", "e"], ["im"], on=2, rows2=capi.PLAN2_PLANE_ROWS, label="65 ids with PLANE_ROWS: the first plan of the row sink")
    assert a.ngroups > 50
    small3(small, ["c", "e"], ["im"], on=0, label="65 ids without PLANE_ROWS")


def test_states(small):
    a = small3(small, [], ["us"], label="uint_sum of 31-bit values")
    exact = sum(int(seg["m"][0][:ROWS].astype(np.uint64).sum()) for seg in small.tab.segments)
    assert exact > 1 << 32 and int(a.states[0][0]) == exact % (1 << 32)
    a = small3(small, [], ["ls"], label="long_sum over 32-bit fields")
    assert int(a.states[0][0]) > 1 << 32
    small3(small, ["a", "b"], ["um"], label="uint_min")
    small3(small, ["a"], ["lm"], label="long_max")
    a = small3(small, ["c"], ["im", "zm", "av"], label="int_min, a uint_max of zeros, AVG with the hidden count")
    assert a.ngroups == 13 and a.hidden_count is not None and not a.states[1].any()
    a = small3(small, ["c", "e"], ["im", "zm", "av"], on=2, rows2=capi.PLAN2_PLANE_ROWS, label="the same states through the row sink")
    assert a.hidden_count is not None
    small3(small, ["a"], ["dd"], on=0, label="a double metric")


# ---- 4. other fields: one that ends at plane 31, a projection that is one 32-plane field, MIN / MAX kinds of byte and short sources
@pytest.mark.parametrize("shape", ["bytes", "long32"])
def test_fields_at_the_top_plane(shape):
    h = S.ShapeHost(shape)
    try:
        case = S.composite(shape, "and")
        want = h.want(case.query, (), ("v", "count"))
        plan = AggPlan(filter=case.nodes, groups=[], metrics=[h.index["v"], h.index["count"]])
        a = run3(h.dt, plan, want, 1, label=f"{shape}: {case.label}")
        assert 0 < a.passed_recs < a.scanned_recs
    finally:
        h.close()


def test_min_max_kinds_of_the_values_shape():
    h = S.ShapeHost("values")
    try:
        case = S.composite("values", "and")
        for dims, metrics in ((("g",), ("mx", "sm")), (("g",), ("lm",)), ((), ("mx", "sm"))):
            want = h.want(case.query, dims, metrics)
            plan = AggPlan(filter=case.nodes, groups=[GroupSpec(h.index[d]) for d in dims], metrics=[h.index[m] for m in metrics])
            run3(h.dt, plan, want, 1, label=f"values: {case.label} by={dims} metrics={metrics}")
    finally:
        h.close()


def test_the_min_max_kinds_no_other_table_has():
    """int_max, long_min, ulong_min and ulong_max (SOP_MAX_I32, SOP_MIN_I64, SOP_MIN_U64, SOP_MAX_U64) against the oracle: a table of its own,
    g of 4 values and four 7-bit metrics in ONE projection of 30 planes (V = F), totals and GROUP BY g, with no filter and under g != 0."""
    rng = np.random.default_rng(11)
    tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": "g", "type": "uint"}],
                    "metrics": [{"name": "ix", "type": "int_max"}, {"name": "ln", "type": "long_min"}, {"name": "un", "type": "ulong_min"},
                                {"name": "ux", "type": "ulong_max"}, {"name": "count", "type": "count"}]})
    for _ in range(NSEG):
        g_ = rng.integers(0, 4, CAP).astype(np.uint32)
        g_[0], g_[1] = 0, 3
        m = [rng.integers(1, 127, CAP).astype(dt) for dt in (np.int32, np.int64, np.uint64, np.uint64)]
        for col in m:
            col[0], col[1] = 127, 0                                # the recorded ranges give 7-bit fields; 0 and the top value are held
        tab.add_segment_arrays([g_], m + [rng.integers(1, 4, CAP).astype(np.uint32)], None, ROWS)
    dt = mirror_table(tab)
    try:
        dt.predpack([0, 1, 2, 3, 4], sliced=True)
        assert len(sliced_layouts(dt)) == 1
        for dims in ([], ["g"]):
            for flt in (None, F("ne", "g", 0)):
                q = {"type": "aggregate", "table": "t", "dimensions": dims, "metrics": ["ix", "ln", "un", "ux"]}
                if flt is not None:
                    q["filter"] = flt
                aq = vo.parse_query(tab, q)
                want = vo.scan_aggregate(aq)
                a = run3(dt, plan_from_query(tab, aq), want, 1, label=f"int_max, long_min, ulong_min, ulong_max by={dims} filter={flt}")
                assert a.ngroups == (1 if not dims else 4 if flt is None else 3)
    finally:
        dt.close()


# ---- 5. snapshots and skipped segments
@pytest.mark.parametrize("snap", [[ROWS, 0, ROWS], [1, 31, 33], [ROWS, 2049, 4097]], ids=lambda s: "-".join(map(str, s)))
def test_snapshots(shared, snap):
    c3(shared, C3F, seg_rows=snap, label="C3")
    a = c3(shared, NO_FILTER, dims=(), seg_rows=snap, label="no filter")
    assert a.passed_recs == sum(snap)


def test_a_segment_skipped_by_its_min_max(host):
    h = host
    seg = h.tab.segments[1]
    seg["d"][D3][:ROWS] = 500 + seg["d"][D3][:ROWS] % 500
    h.sync(1, 0, ROWS)
    a = c3(h, AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), label="segment 1 skipped")
    assert a.scanned_segments == 2 and a.passed_recs > 0


# ---- 6. coherence
def test_a_sync_that_leaves_v_stale(host):
    h = host
    c3(h, C3F, label="before")
    h.tab.segments[0]["m"][0][:100] += 1500             # m0 needs 11 bits, V's field has 10: V is dropped
    h.sync(0, 0, 100)
    c3(h, C3F, on=0, label="m0 outgrew its field")


def test_a_value_outside_the_planned_range():
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
        q = {"type": "aggregate", "table": "t", "dimensions": ["s"], "metrics": ["v", "count"], "filter": F("lt", "f", 800)}
        aq = vo.parse_query(tab, q)
        plan = plan_from_query(tab, aq)
        a = run3(dt, plan, vo.scan_aggregate(aq), 1, label="three codes, three ids")
        assert a.ngroups == 3
        dic.v2c["z"] = 3
        dic.c2v.append("z")
        seg = tab.segments[1]
        seg["d"][0][2048 + 31], seg["d"][1][2048 + 31] = 3, 0
        dt.sync_batch([(1, 2048 + 31, 1, ROWS, seg_columns(tab, seg), 0)])
        want = vo.scan_aggregate(vo.parse_query(tab, q))
        assert want.ngroups == 4
        forced = 0 if JIT_OFF else capi.PLAN_FORCE_JIT
        a = dt.query_agg(dataclasses.replace(plan, flags=forced, flags2=JIT2))      # the plan still says three ids: planned again
        compare(a, want, "a fourth code behind the plan's back")
        assert a.ngroups == 4 and not a.plane_agg
        a = run3(dt, plan_from_query(tab, vo.parse_query(tab, q)), want, 1, label="planned again with four ids")
        assert a.ngroups == 4
    finally:
        dt.close()


# ---- 7. one compile per shape: other literals, another lo
def _ranged(lo):
    """dims a (lo .. lo + 3, below 16: a 4-bit field whatever lo) and f, metrics v and count; F = [a, f], V = [a, v, count]."""
    rng = np.random.default_rng(lo)
    tab = vo.Table({"name": "t", "segment_size": CAP, "dimensions": [{"name": "a", "type": "uint"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "uint_sum"}, {"name": "count", "type": "count"}]})
    for _ in range(NSEG):
        a_ = rng.integers(lo, lo + 4, CAP).astype(np.uint32)
        a_[0], a_[1] = lo, lo + 3
        f_ = rng.integers(0, 1000, CAP).astype(np.uint32)
        f_[0], f_[1] = 0, 999
        v_ = rng.integers(0, 500, CAP).astype(np.uint32)
        v_[0], v_[1] = 0, 499
        tab.add_segment_arrays([a_, f_], [v_, rng.integers(1, 4, CAP).astype(np.uint32)], None, ROWS)
    dt = mirror_table(tab)
    dt.predpack([0, 1], sliced=True)
    dt.predpack([0, 2, 3], sliced=True)
    return tab, dt


@needs_jit
def test_one_kernel_per_shape(shared):
    names = set()
    for lit in (447, 100, 999):
        flt = AND(REL(D2, "eq", lit % 4), REL(D3, "lt", lit), REL(D4, "ge", 1000 - lit))
        names.add(c3(shared, flt, label=f"C3 with {lit}").kernel)
    assert len(names) == 1, names
    names = set()
    for lo, lit in ((8, 500), (9, 200), (12, 900)):          # a in 8 .. 11, 9 .. 12, 12 .. 15: four planes each, three values of lo
        tab, dt = _ranged(lo)
        try:
            aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": ["a"], "metrics": ["v", "count"], "filter": F("lt", "f", lit)})
            a = run3(dt, plan_from_query(tab, aq), vo.scan_aggregate(aq), 1, label=f"a from {lo} on, f < {lit}")
            assert a.ngroups == 4 and min(a.keys[0].tolist()) == lo
            names.add(a.kernel)
        finally:
            dt.close()
    assert len(names) == 1, names                             # lo, extent and the literal are data: one text, one kernel


# ---- 8. VH_JIT=off in a child, and the environment switch
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
res = h.dt.query_agg(AggPlan(filter=p.filter, groups=[GroupSpec(2)], metrics=p.metrics, flags={flags}, flags2={flags2}))
print("FLAGS", res.flags, res.passed_recs, res.plane_sink, res.kernel)
h.close()
"""


def child(env_set, flags, flags2):
    env = {k: v for k, v in os.environ.items() if k not in ("VH_PLANE_AGG", "VH_PLANE_JIT", "VH_JIT")}
    env.update(env_set)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, flags=flags, flags2=flags2)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("FLAGS ")][-1].split(None, 4)
    return int(line[1]), int(line[2]), int(line[3]), line[4]


def test_under_jit_off_the_prebuilt_kernel_answers(shared):
    here = shared.dt.query_agg(AggPlan(filter=C3F[0], groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=capi.PLAN_NO_JIT))
    flags, passed, sink, kernel = child({"VH_JIT": "off"}, 0, JIT2)
    assert passed == here.passed_recs
    assert flags & BIT27 and not flags & BIT5 and flags & ON_PLANES == ON_PLANES and not flags & OFF and sink == 1 and kernel.startswith(PREBUILT), (hex(flags), kernel)


@needs_jit
def test_the_environment_switch(shared):
    here = shared.dt.query_agg(AggPlan(filter=C3F[0], groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=capi.PLAN_NO_JIT))
    flags, passed, sink, kernel = child({"VH_PLANE_JIT": "1"}, capi.PLAN_FORCE_JIT, 0)
    assert passed == here.passed_recs
    assert flags & BIT27 and flags & BIT5 and not flags & OFF and sink == 1 and kernel.startswith(COMPILED), (hex(flags), kernel)


# ---- 9. a VH_BUILD_BACKGROUND table: pending first, compiled after the worker is done
@needs_jit
def test_on_a_background_table(host):
    h = host
    h.dt.set_build_mode(True)
    try:
        # a shape no other test of this file compiles: four leaves, SUM(count) alone
        nodes, qfilter = AND(REL(D2, "ne", 2), REL(D3, "le", 600), REL(D4, "gt", 300), REL(D4, "ne", 7))
        q = {"type": "aggregate", "table": "synth", "dimensions": ["d2"], "metrics": ["count"], "filter": qfilter}
        want = vo.scan_aggregate(vo.parse_query(h.tab, q))
        plan = AggPlan(filter=nodes, groups=[GroupSpec(D2)], metrics=[COUNT], flags=capi.PLAN_FORCE_JIT, flags2=JIT2)
        first = h.dt.query_agg(plan)
        compare(first, want, "pending")
        h.dt.build_wait(120000)
        second = h.dt.query_agg(plan)
        compare(second, want, "compiled")
        agree(first, second, "pending / compiled")
        # pending is decided at once: the lookup is of this process's kernels alone, and no other test of this file compiles this shape
        assert first.flags & capi.INFO_BUILD_PENDING, hex(first.flags)
        assert first.flags & BIT27 and not first.flags & BIT5 and first.kernel.startswith(PREBUILT) and first.plane_sink == 1, (hex(first.flags), first.kernel)
        assert second.flags & BIT27 and second.flags & BIT5 and second.kernel.startswith(COMPILED) and not second.flags & capi.INFO_BUILD_PENDING, (hex(second.flags), second.kernel)
    finally:
        h.dt.set_build_mode(False)


# ---- 10. in a batch: the member with the flag is answered singly, the others fuse as before
def test_in_a_batch(shared):
    h = shared
    forced = 0 if JIT_OFF else capi.PLAN_FORCE_JIT
    filters = [C3F, AND(REL(D2, "eq", 2), REL(D3, "lt", 600)), EVERY_ROW]
    plans = [AggPlan(filter=f[0], groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=capi.PLAN_NO_JIT, flags2=capi.PLAN2_PLANE_AGG) for f in filters]
    plans[1] = dataclasses.replace(plans[1], flags=forced, flags2=JIT2)
    got, info = h.dt.query_agg_batch(plans)
    singles = [h.dt.query_agg(p) for p in plans]
    for k, (a, b) in enumerate(zip(got, singles)):
        agree(a, b, f"member {k}")
        assert a.passed_recs == b.passed_recs and a.ngroups == b.ngroups
    assert got[0].batch_fused and got[2].batch_fused and not got[1].batch_fused, [hex(g.flags) for g in got]
    assert got[1].flags == singles[1].flags and got[1].kernel == singles[1].kernel and got[1].plane_agg
    assert got[1].jit == (not JIT_OFF)
    assert info.fused_members == 2 and info.singles == 1, (info.fused_members, info.singles)
