"""The readers of the bit-sliced predicate planes at fields other than C3's (tests/plane_shapes.py lists the tables and what each reaches):
1-, 2-, 4- and 8-byte sources, signed ones among them; fields of 1, 7, 8, 15, 16, 17, 31 and 32 planes, one ending at plane 31, one
projection that is a single 32-plane field; literals that wrap in a ubyte and a ushort, negative int and long literals, ulong literals from
2^63 on; group ids and metric values off fields of ubyte, ushort, int and long sources.

The six readers: the select kernels (select_count_sliced_kernel / select_emit_sliced_kernel), the pre-built aggregate scan
(scan_agg_sliced_kernel), the plane aggregate's loop sink (scan_agg_planes_kernel) and row sink (scan_agg_planes_rows_kernel), the fused
batch kernel (scan_agg_planes_batch_kernel) — all five over vh_bits_eval.h, under PLAN_NO_JIT, so they run under VH_JIT=off too — and the
compiled scan (vj_bits_rel / vj_bits_inset; skipped under VH_JIT=off).

Every case is compared three ways: against the oracle over the host's arrays (tests/parity.compare; oracle_select for selects), bit for bit
against its twin off the planes (every state here is an integer), and against the rule's what-ran bits. plane_shapes.DECLINED lists the kinds
of case the planner keeps off the planes: such a case still runs, its flags and kernel are the twin's and its answer the oracle's. Every
other case must report that it ran on the planes; none may leave them unlisted.

The plane aggregate's own fields (group ids, MIN / MAX / SUM values) are those of `values`. The other four shapes fill their filter
projection's 32 planes, so a metric cannot share it, not even a 1-plane one: there the aggregate reads the filter off F and the sums of v and
count off a projection V of their own.

From 15 % of the rows passing (VH_QPAY_MIN_SEL, by a probe of the data) the planner streams the payload records beside byte planes and the
compiled scan reads no bit-sliced plane at all; the literals here go up to every row passing, so the compiled reader's plans carry
PLAN_NO_QPAY beside PLAN_FORCE_JIT | PLAN_NO_LANES, as tests/test_gpu_cluster_shapes.py's do, and stay the scan whose vj_bits_rel is under
test. Below 15 % the flag changes nothing. The compiled scan compiles one kernel per plan shape — column types, field widths, relations —, literals are arguments: its sweeps on `l`
(32 planes) and `i` (31) are parametrised by relation so that a test function pays for one or two compiles."""
import dataclasses

import numpy as np
import pytest

from tests import plane_shapes as S
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.test_gpu_agg_sliced import BASE as PRE_BASE, PREBUILT, agree, expect_flags
from tests.test_gpu_batch import Member
from tests.test_gpu_batch_rows import run as run_members
from tests.test_gpu_batch_share import member_info
from tests.test_gpu_plane_rows import AGG, HOOK, ROWS2, run3
from tests.test_gpu_select import oracle_select
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
NO_SLICED = capi.PLAN_NO_SLICED
ON_PLANES, SLICED = capi.INFO_ON_PLANES, capi.INFO_SLICED
SETS = capi.INFO_INSET | capi.INFO_INSET_SLICED
NOJIT = capi.PLAN_NO_JIT
COMPILED = capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES | capi.PLAN_NO_QPAY
COLUMNS = [(sh, c) for sh in S.SHAPES for c in S.SHAPES[sh].filt]
RAGGED = ([S.CHUNK + 32 * 5 + 13, 0, S.ROWS], [1, 4991, 33])
COUNTS = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def hosts():
    """ShapeHost(name), one per shape for the cases that change nothing."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.ShapeHost(name)
        return made[name]
    yield get
    for h in made.values():
        h.close()
    print("cases per reader:", COUNTS)


def counted(reader):
    COUNTS[reader] = COUNTS.get(reader, 0) + 1


def rule(h, case, on):
    """What the rule says of the case: on the planes unless DECLINED lists its kind (`on`: a caller that knows better — the projection is gone)."""
    return (case is None or S.declined(h.name, case) is None) if on is None else on


def cases_of(shape, column, kinds=("rel", "in", "inset")):
    return [c for c in S.column_cases(shape, column) if c.kind in kinds]


def plan_of(h, case, dims, metrics, flags, seg_rows=None, flags2=0):
    return AggPlan(filter=case.nodes if case is not None else [], groups=[GroupSpec(h.index[d]) for d in dims], metrics=[h.index[m] for m in metrics],
                   flags=flags, flags2=flags2, seg_rows=seg_rows)


# ---- reader 1: the select kernels
def select_check(h, case, skip=0, limit=0, seg_rows=None, on=None):
    on = rule(h, case, on)
    cols = [h.index[case.column or h.shape.filt[0]], h.index["v"]]
    label = f"{case.label} [select] skip={skip} limit={limit} snapshot={seg_rows}"
    want, stats = oracle_select(h.tab, h.query(case.query), cols, skip, limit, seg_rows)
    got, info, path = h.dt.query_select_ex(case.nodes, cols, skip=skip, limit=limit, seg_rows=seg_rows)
    twin, tinfo, tpath = h.dt.query_select_ex(case.nodes, cols, skip=skip, limit=limit, seg_rows=seg_rows, flags=NO_SLICED)
    for res, i in ((got, info), (twin, tinfo)):
        assert (i.nrows, i.scanned_recs, i.scanned_segments, i.passed_recs) == \
               (stats["output_recs"], stats["scanned_recs"], stats["scanned_segments"], stats["passed_recs"]), (label, i.nrows, i.passed_recs, stats)
        for a, b in zip(res, want):
            assert len(a) == len(b) and (not len(b) or np.array_equal(a, b.astype(a.dtype))), label
    for a, b in zip(got, twin):
        assert a.dtype == b.dtype and np.array_equal(a, b), label
    assert not tpath & ON_PLANES, (label, hex(tpath))
    if on:
        assert path & SLICED and path & ON_PLANES == ON_PLANES, (label, hex(path))
        assert path & (SETS | capi.INFO_INSET_SEARCH) == (SETS if case.kind == "inset" else 0), (label, hex(path))
    else:
        assert path == tpath, (label, hex(path), hex(tpath))
    counted("select")
    return info


# ---- reader 2: the pre-built aggregate scan
def prebuilt_check(h, case, dims=("k",), flags=0, seg_rows=None, on=None):
    on = rule(h, case, on)
    label = f"{case.label} [pre-built] by={list(dims)} flags={flags:#x} snapshot={seg_rows}"
    want = h.want(case.query, dims, seg_rows=seg_rows)
    a, b = (h.dt.query_agg(plan_of(h, case, dims, ("v", "count"), PRE_BASE | flags | fl, seg_rows)) for fl in (PREBUILT, 0))
    compare(a, want, label + " [on the planes]")
    compare(b, want, label + " [twin]")
    agree(a, b, label)
    assert a.path == b.path, (label, a.path, b.path)
    expect_flags(a, b, on, on and case.kind == "inset", label)
    counted("pre-built scan")
    return a


# ---- readers 3 and 4: the plane aggregate's loop sink, and the same plan through its row sink (VH_TEST_PLANE_ROWS_MIN=1)
def planes_check(h, case, dims, metrics, monkeypatch, seg_rows=None, on=None):
    on = rule(h, case, on)
    label = f"{case.label if case is not None else h.name + ': no filter'} [plane aggregate] by={list(dims)} metrics={list(metrics)} snapshot={seg_rows}"
    want = h.want(case.query if case is not None else None, dims, metrics, seg_rows=seg_rows)
    plan = plan_of(h, case, dims, metrics, NOJIT, seg_rows)
    monkeypatch.delenv(HOOK, raising=False)
    loop = run3(h.dt, plan, want, 1 if on else 0, label + " [loop]", flags2=AGG)
    monkeypatch.setenv(HOOK, "1")
    rows = run3(h.dt, plan, want, 2 if on else 0, label + " [row sink]", flags2=ROWS2)
    monkeypatch.delenv(HOOK)
    agree(loop, rows, label)
    assert loop.returned == rows.returned
    counted("plane aggregate, loop sink")
    counted("plane aggregate, row sink")
    return loop


def rows_check(h, case, dims, metrics, seg_rows=None, on=None, sink=2):
    """PLAN2_PLANE_ROWS without the hook: a plan of more than 64 ids takes the row sink (`sink=1`: at most 64 ids, the loop)."""
    on = rule(h, case, on)
    label = f"{case.label if case is not None else h.name + ': no filter'} [row sink] by={list(dims)} snapshot={seg_rows}"
    want = h.want(case.query if case is not None else None, dims, metrics, seg_rows=seg_rows)
    a = run3(h.dt, plan_of(h, case, dims, metrics, NOJIT, seg_rows), want, sink if on else 0, label, flags2=ROWS2)
    counted("plane aggregate, row sink" if sink == 2 else "plane aggregate, loop sink")
    return a


# ---- reader 6: the compiled scan
def compiled_check(h, case, dims=("k",), on=None):
    on = rule(h, case, on)
    label = f"{case.label} [compiled]"
    want = h.want(case.query, dims)
    a = h.dt.query_agg(plan_of(h, case, dims, ("v", "count"), COMPILED))
    b = h.dt.query_agg(plan_of(h, case, dims, ("v", "count"), PRE_BASE))
    compare(a, want, label + " [on the planes]")
    compare(b, want, label + " [twin]")
    agree(a, b, label)
    assert a.jit and not b.jit and not b.sliced, (label, hex(a.flags), hex(b.flags))
    assert (a.predpack and a.sliced) if on else not a.sliced, (label, hex(a.flags), a.kernel)
    assert a.inset_sliced == (on and case.kind == "inset"), (label, hex(a.flags))
    counted("compiled scan")
    return a


def plane_metrics(h):
    """What the plane aggregate sums and by what it groups, per shape: on `values` the fields of V1 and V2, elsewhere v and count of V."""
    if h.name == "values":
        return [(("g",), ("mx", "sm")), (("g",), ("lm",)), ((), ("mx", "sm")), ((), ("lm",))]      # (a total per V: no projection holds mx, sm and lm)
    return [((), ("v", "count"))]


@pytest.mark.parametrize("reader", ["select", "prebuilt", "planes"])
@pytest.mark.parametrize("shape, column", COLUMNS, ids=lambda x: x)
def test_the_literal_sweep(hosts, monkeypatch, shape, column, reader):
    """Every literal of the column's set under the six relations, IN / NOT IN of three literals and the same lists as set leaves: the select
    and the pre-built scan take all of it; the plane aggregate takes every literal under `le` and `ne`, and the negative ones under `gt`, through
    both sinks."""
    h = hosts(shape)
    if reader == "planes":
        t = S.column(shape, column)[1]
        for case in [c for c in cases_of(shape, column, ("rel",)) if c.op in ("le", "ne") or (c.op == "gt" and S.as_held(t, c.lits[0]) < 0)]:
            for dims, metrics in plane_metrics(h):      # (`le` of a negative literal is settled by the segments' minima: `gt` of it reaches the kernel)
                planes_check(h, case, dims, metrics, monkeypatch)
        return
    verdicts = set()
    for case in cases_of(shape, column):
        r = select_check(h, case) if reader == "select" else prebuilt_check(h, case)
        verdicts.add("none" if r.passed_recs == 0 else "all" if r.passed_recs == S.NSEG * S.ROWS else "some")
    assert verdicts == {"none", "some", "all"}, verdicts


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_composites(hosts, monkeypatch, shape):
    """The flat AND over the shape's filter columns, the nest that needs the stack and, on long32, the AND no projection holds (DECLINED):
    every pre-built reader; the select's windows at the word's, the chunk's and the segment's survivor counts."""
    h = hosts(shape)
    conj = S.composite(shape, "and")
    for case in [c for c in S.filters(shape) if c.column is None]:
        info = select_check(h, case)
        assert 0 < info.passed_recs < info.scanned_recs
        prebuilt_check(h, case)
        for dims, metrics in plane_metrics(h):
            planes_check(h, case, dims, metrics, monkeypatch)
    m = h.mask(conj, 0)
    word, chunk, seg = int(m[:32].sum()), int(m[:S.CHUNK].sum()), int(m.sum())
    assert word < chunk < seg
    for skip, limit in [(0, 0)] + [(max(0, n + d), lim) for n in (word, chunk, seg) for d in (-1, 0, 1) for lim in (0, 2)]:
        select_check(h, conj, skip, limit)
    a = prebuilt_check(h, conj, dims=())
    assert a.path == "scalar"
    a = prebuilt_check(h, conj, flags=capi.PLAN_FORCE_HASH)
    assert a.path == "hash"
    for dims, metrics in plane_metrics(h):
        planes_check(h, None, dims, metrics, monkeypatch)


# ---- reader 4: plans of more than 64 ids
def test_the_row_sink_on_group_fields_of_byte_and_short_sources(hosts):
    h = hosts("values")
    for dims in (("g", "h"), ("h", "g")):
        a = rows_check(h, None, dims, ("mx", "sm"))
        assert a.path == "dense_lds" and a.ngroups > 2000 and a.passed_recs == S.NSEG * S.ROWS
        for which in ("and", "nest"):
            a = rows_check(h, S.composite("values", which), dims, ("mx", "sm"))
            assert 0 < a.passed_recs < a.scanned_recs
    for case in [c for c in cases_of("values", "f", ("rel",)) if c.op in ("le", "ne")]:
        rows_check(h, case, ("g", "h"), ("mx", "sm"))
    rows_check(h, S.composite("values", "and"), ("g",), ("lm",), sink=1)          # (7 ids with PLAN2_PLANE_ROWS: the loop)


# ---- reader 5: the fused batch kernel
def member(h, case, dims, metrics, flags2, fused=True, label=""):
    want = h.want(case.query if case is not None else None, dims, metrics)
    return Member(plan_of(h, case, dims, metrics, NOJIT, flags2=flags2), want, fused, False, f"{label} by={list(dims)} metrics={list(metrics)}")


def one_leaf(shape, column, op, lit):
    nodes, q = S._rel(shape, column, op, lit)
    return S.Case("rel", column, op, (lit,), [nodes], q, f"{shape}: {column} {op} {lit}")


def test_the_fused_batch(hosts):
    h = hosts("values")
    x, y = one_leaf("values", "f", "lt", "512"), one_leaf("values", "f", "lt", "513")
    members = [member(h, x, ("g",), ("mx", "sm"), ROWS2, label="f < 512"), member(h, x, (), ("mx", "sm"), ROWS2, label="f < 512, a total"),
               member(h, y, ("g",), ("sm",), ROWS2, label="f < 513"), member(h, x, ("g", "h"), ("mx", "sm"), ROWS2, label="f < 512, the row member")]
    assert members[0].want.passed_recs != members[2].want.passed_recs          # (the planted rows with f == 512)
    res, _ = run_members(h.dt, members, [True], label="values: four members, two masks")
    assert [member_info(r) for r in res] == [(1, 0, 0, 4, 0, 2), (1, 0, 1, 4, 0, 2), (1, 0, 2, 4, 2, 2), (1, 0, 3, 4, 0, 2)]      # vh_batch_share: one class per filter
    assert [r.plane_sink for r in res] == [1, 1, 1, 2] and all(r.batch_fused for r in res)
    counted("fused batch")
    h = hosts("long32")
    lits = (("lt", str(2 ** 31)), ("le", str(2 ** 32 + 5)), ("gt", "-1"))
    members = [member(h, one_leaf("long32", "l", op, lit), (), ("v", "count"), AGG, label=f"l {op} {lit}") for op, lit in lits]
    assert 0 < members[0].want.passed_recs < S.NSEG * S.ROWS and members[1].want.passed_recs == members[2].want.passed_recs == S.NSEG * S.ROWS
    res, _ = run_members(h.dt, members, [False], label="long32: three literals on l")
    assert [member_info(r) for r in res] == [(1, 0, i, 3, i, 3) for i in range(3)]
    assert all(r.batch_fused and r.plane_sink == 1 for r in res)
    counted("fused batch")


# ---- reader 6
@pytest.mark.skipif(JIT_OFF, reason="the compiled scan is switched off")
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_the_compiled_scan_on_the_composites(hosts, shape):
    h = hosts(shape)
    for case in [c for c in S.filters(shape) if c.kind in ("and", "across")]:
        a = compiled_check(h, case)
        assert 0 < a.passed_recs < a.scanned_recs


@pytest.mark.skipif(JIT_OFF, reason="the compiled scan is switched off")
@pytest.mark.parametrize("op", list(S.OPS) + ["sets"])
@pytest.mark.parametrize("shape, column", [("long32", "l"), ("int31", "i")], ids=lambda x: x)
def test_the_compiled_scan_sweeps_32_and_31_planes(hosts, shape, column, op):
    """vj_bits_rel<32, OP> and <31, OP> under every literal of the set; "sets": IN / NOT IN as lists (on the planes) and as set leaves (a
    field wider than VH_INSET_TRUTH_BITS: DECLINED)."""
    h = hosts(shape)
    cases = [c for c in cases_of(shape, column) if (c.op == op if op != "sets" else c.kind != "rel")]
    assert len(cases) >= 4
    verdicts = set()
    for case in cases:
        a = compiled_check(h, case)
        verdicts.add("none" if a.passed_recs == 0 else "all" if a.passed_recs == S.NSEG * S.ROWS else "some")
    assert "some" in verdicts and (op == "sets" or len(verdicts) >= 2), verdicts


# ---- after a sync: a value that outgrows `a`'s 7 planes drops the projection, and every reader falls back
def test_after_a_sync_that_outgrows_a_field(monkeypatch):
    h = S.ShapeHost("bytes")
    try:
        conj, leaf = S.composite("bytes", "and"), one_leaf("bytes", "a", "le", "64")
        batch = [member(h, c, (), ("v", "count"), AGG, label=c.label) for c in (conj, leaf)]
        for on in (None, False):
            if on is False:
                arr = h.named(0)["a"]
                assert arr[0] == 127
                arr[0] = 128                                                    # 8 bits: beyond the field; predpack_usable drops F
                h.sync(0, 0, 1)
                batch = [dataclasses.replace(member(h, c, (), ("v", "count"), AGG, label=c.label), fused=False) for c in (conj, leaf)]
            for case in (conj, leaf):
                select_check(h, case, on=on)
                prebuilt_check(h, case, on=on)
                planes_check(h, case, (), ("v", "count"), monkeypatch, on=on)
                if not JIT_OFF:
                    compiled_check(h, case, on=on)
            run_members(h.dt, batch, [False] if on is None else [], label="bytes: two totals")
            assert len(h.sliced_layouts()) == (2 if on is None else 1)          # V stays
        info = select_check(h, one_leaf("bytes", "a", "ge", "128"), on=False)
        assert info.passed_recs == 1
    finally:
        h.close()


# ---- ragged snapshots: the word that straddles seg_rows is masked, a segment of no rows, a segment of one
@pytest.mark.parametrize("snap", RAGGED, ids=lambda s: "-".join(map(str, s)))
def test_ragged_snapshots(hosts, monkeypatch, snap):
    h = hosts("int31")
    for case in (S.composite("int31", "and"), one_leaf("int31", "i", "le", str(2 ** 30)), one_leaf("int31", "i", "gt", "-1"), one_leaf("int31", "b", "ne", "256")):
        select_check(h, case, seg_rows=snap)
        a = prebuilt_check(h, case, seg_rows=snap)
        planes_check(h, case, (), ("v", "count"), monkeypatch, seg_rows=snap)
        if case.op == "gt":
            assert a.passed_recs == sum(snap)
    h = hosts("values")
    rows_check(h, S.composite("values", "and"), ("g", "h"), ("mx", "sm"), seg_rows=snap)
    a = rows_check(h, None, ("h", "g"), ("mx", "sm"), seg_rows=snap)
    assert a.passed_recs == sum(snap)
