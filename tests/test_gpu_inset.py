"""VH_F_INSET — an IN / NOT IN list evaluated as one set lookup per row (include/viya_hip.h, viyadb_amd/csrc/vh_inset.h) — against
the oracle on the typed table of tests/test_gpu_typed.py (3 x 40 000 rows). Every plan comes from plan_from_query with its "in"
tuples rewritten to "inset" and goes through compare(), which holds keys, states and every counter exactly: a set leaf must give
exactly what the VH_F_IN leaf with the same fields gives. On top: which lookup form ran (vh_result_info.reserved bits 22 / 23),
which kernels and layouts serve such a plan, the refusals, and that a list's length or form never changes the code object."""
import dataclasses

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query, storage_index
from tests.test_gpu_typed import NOW, F, typed_table
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan

pytestmark = pytest.mark.gpu

NO_FAST, FORCE_HASH, FORCE_JIT, SET_SEARCH = capi.PLAN_NO_FAST, capi.PLAN_FORCE_HASH, capi.PLAN_FORCE_JIT, capi.PLAN_SET_SEARCH
COLUMNS = ["d_ubyte", "d_ushort", "d_int", "d_uint", "d_long", "d_ulong", "s8", "s16", "s32", "flag", "ts", "uts", "id"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def typed():
    tab = typed_table()
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


def to_inset(plan):
    """The same plan with every "in" leaf of the scan filter as a set leaf."""
    return dataclasses.replace(plan, filter=[("inset",) + tuple(f[1:]) if f[0] == "in" else f for f in plan.filter])


def set_spans(tab, plan):
    """largest - smallest member of every set leaf, in the column's own type."""
    cols = list(tab.dims) + list(tab.metrics)
    out = []
    for f in plan.filter:
        if f[0] != "inset":
            continue
        dtype = np.dtype(cols[f[1]].num_type.dtype)
        vals = [int(np.frombuffer(bytes(a), dtype=dtype, count=1)[0]) for a in f[3]]
        out.append(max(vals) - min(vals))
    return out


def run(tab, dt, q, flags=0, st=None, seg_rows=None):
    """-> (result of the set plan, oracle state). The oracle's state is computed once per query and shared between the flags."""
    q = dict({"type": "aggregate", "table": "t"}, **q)
    aq = vo.parse_query(tab, q)
    if st is None:
        st = vo.scan_aggregate(aq, now=NOW, seg_rows=seg_rows)
    plan = to_inset(plan_from_query(tab, aq, now=NOW, flags=flags, seg_rows=seg_rows))
    assert any(f[0] == "inset" for f in plan.filter)
    res = dt.query_agg(plan)
    compare(res, st, f"{q.get('filter')} flags={flags:#x}")
    assert res.inset, "vh_result_info.reserved bit 22"
    want_search = bool(flags & SET_SEARCH) or any(s >= 2 ** 20 for s in set_spans(tab, plan))
    assert res.inset_search == want_search, (res.flags, set_spans(tab, plan))
    return res, st


def members(tab, col, present=40, absent=5):
    """Literal texts for a filter on `col`: up to `present` distinct values the column holds, then `absent` it does not."""
    c = tab.column(col)
    held = np.unique(np.concatenate([seg["d"][c.index][:seg["size"]] for seg in tab.segments]))
    rng = np.random.default_rng(len(col))
    picked = rng.choice(held, size=min(present, len(held)), replace=False)
    if c.dim_type == "string":
        dic = tab.dicts[col]
        return [dic.c2v[int(v)] for v in picked if int(v) < len(dic.c2v)] + ["nowhere%d" % k for k in range(absent)]
    if c.dim_type == "boolean":
        return ["true", "false"]
    top = int(held.max())
    return [str(int(v)) for v in picked] + [str(top + 7 + 3 * k) for k in range(absent)]


def in_filter(col, values, equal=True):
    f = {"op": "in", "column": col, "values": values}
    return f if equal else {"op": "not", "filter": f}


# ---- 1. every column type, both polarities, every kernel that serves a set leaf
@pytest.mark.parametrize("equal", [True, False], ids=["in", "not_in"])
@pytest.mark.parametrize("col", COLUMNS)
def test_every_column_type(typed, col, equal):
    tab, dt = typed
    q = {"dimensions": ["s8"], "metrics": ["count", "long_sum"], "filter": in_filter(col, members(tab, col), equal)}
    st = None
    for flags in (0, NO_FAST, FORCE_JIT, FORCE_JIT | SET_SEARCH, FORCE_HASH | FORCE_JIT):
        res, st = run(tab, dt, q, flags=flags, st=st)
        from tests.conftest import JIT_OFF
        if flags & FORCE_JIT and not JIT_OFF:
            assert res.jit and res.kernel.startswith("viya_jit_scan_"), (flags, res.kernel)
        if flags & NO_FAST:
            assert not res.fast
    assert 0 < st.passed_recs < st.scanned_recs or col == "flag"


# ---- 2. edges
@pytest.mark.parametrize("col,values,search", [
    ("id", ["0"], False), ("id", ["119999"], False), ("id", ["31", "32", "33", "63", "64"], False),
    ("id", ["5", str(5 + 2 ** 20 - 1)], False),         # span 2^20 - 1: still a bitmap
    ("id", ["5", str(5 + 2 ** 20)], True),              # span 2^20: the sorted array
    ("d_long", [str(-2 ** 63), "-60", "-1", "0", "59", str(2 ** 63 - 1)], True),
    ("d_ulong", ["0", "60", str(2 ** 63), str(2 ** 64 - 1)], True),
    ("s32", ["v17", "v4999", "not in the dictionary"], True)])      # a missing string decodes to UINT32_MAX: the array form
def test_edges(typed, col, values, search):
    tab, dt = typed
    for equal in (True, False):
        st = None
        for flags in (0, FORCE_JIT):
            res, st = run(tab, dt, {"dimensions": ["flag"], "metrics": ["count", "int_sum"], "filter": in_filter(col, values, equal)}, flags=flags, st=st)
            assert res.inset_search == search
        assert st.passed_recs > 0


# ---- 3. a composite filter: sets beside ordinary leaves, nested
def test_composite_filter(typed):
    tab, dt = typed
    s16 = ["v%d" % v for v in range(0, 3000, 10)]
    flt = {"op": "or", "filters": [{"op": "and", "filters": [in_filter("s16", s16), F("lt", "d_uint", "30")]},
                                   in_filter("d_int", [str(v) for v in range(-60, 45, 3)], equal=False)]}
    assert len(s16) == 300 and len(flt["filters"][1]["filter"]["values"]) == 35
    st = None
    for flags in (0, NO_FAST, FORCE_JIT, FORCE_JIT | SET_SEARCH, FORCE_HASH | FORCE_JIT, FORCE_HASH | FORCE_JIT | capi.PLAN_FORCE_HPART):      # (the last: hashed partitioning)
        res, st = run(tab, dt, {"dimensions": ["s8", "flag"], "metrics": ["count", "long_sum", "double_max"], "filter": flt}, flags=flags, st=st)
    assert 0 < st.passed_recs < st.scanned_recs


# ---- 4. set counts
def test_four_sets_answer_five_are_refused(typed):
    tab, dt = typed
    leaves = [in_filter("d_int", [str(v) for v in range(-50, 50)]), in_filter("d_uint", [str(v) for v in range(0, 55)]),
              in_filter("s8", ["v%d" % v for v in range(120)]), in_filter("d_long", ["-3", "4", "5"], equal=False),
              in_filter("d_ushort", [str(v) for v in range(2, 58)])]
    for flags in (0, FORCE_JIT):
        run(tab, dt, {"dimensions": ["s8"], "metrics": ["count"], "filter": {"op": "and", "filters": leaves[:4]}}, flags=flags)
    aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": ["s8"], "metrics": ["count"], "filter": {"op": "and", "filters": leaves}})
    with pytest.raises(capi.VhError) as e:
        dt.query_agg(to_inset(plan_from_query(tab, aq, now=NOW)))
    assert e.value.code == -4, e.value       # VH_E_UNSUPPORTED


# ---- 5. refusals (on code without the feature every one of these is VH_E_INVALID: "kind 5")
def test_refusals(typed):
    tab, dt = typed
    col = lambda name: storage_index(tab, tab.column(name))
    s8 = AggPlan(groups=plan_from_query(tab, vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": ["s8"], "metrics": ["count"]}), now=NOW).groups,
                 metrics=[col("count")])
    with pytest.raises(capi.VhError) as e:
        dt.query_agg(dataclasses.replace(s8, filter=[("inset", col("d_float"), True, [1.5, 2.5])]))
    assert e.value.code == -4, e.value       # a floating column: VH_E_UNSUPPORTED, the caller keeps VH_F_IN
    with pytest.raises(capi.VhError) as e:
        dt.query_agg(dataclasses.replace(s8, filter=[("inset", col("double_max"), True, [1.5])]))
    assert e.value.code == -4, e.value
    with pytest.raises(capi.VhError) as e:
        dt.query_agg(dataclasses.replace(s8, having=[("inset", 0, True, [3, 4])]))
    assert e.value.code == -1, e.value       # a set in HAVING: VH_E_INVALID
    with pytest.raises(capi.VhError) as e:
        dt.query_agg(dataclasses.replace(s8, filter=[("inset", col("d_int"), True, [])]))
    assert e.value.code == -1, e.value       # count = 0: VH_E_INVALID
    # ... and the same leaves as VH_F_IN / with a member answer
    dt.query_agg(dataclasses.replace(s8, filter=[("in", col("d_float"), True, [1.5, 2.5])]))
    assert dt.query_agg(dataclasses.replace(s8, filter=[("inset", col("d_int"), True, [3])])).inset


# ---- 6. a ragged size() snapshot
def test_ragged_snapshot(typed):
    tab, dt = typed
    q = {"dimensions": ["s8"], "metrics": ["count", "long_sum"], "filter": in_filter("id", [str(v) for v in range(0, 120000, 7)])}
    st = None
    for flags in (FORCE_JIT, 0):
        res, st = run(tab, dt, q, flags=flags, st=st, seg_rows=[40000, 1234, 0])
    assert res.scanned_recs == 41234 and 0 < st.passed_recs < 41234


# ---- 7. segment skipping: the verdict of the VH_F_IN loop, found by binary search
def test_segment_skipping():
    n, nseg = 20000, 6
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "time", "type": "ulong"}, {"name": "k", "type": "ubyte"}],
                    "metrics": [{"name": "count", "type": "count"}]})
    rng = np.random.default_rng(5)
    for s in range(nseg):
        tab.add_segment_arrays([np.arange(s * n, (s + 1) * n, dtype=np.uint64), rng.integers(0, 9, n).astype(np.uint8)], [np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        for values, equal, want in (([str(n + 1), str(3 * n)], True, 2), ([str(n + 1)], False, 1), ([str(7 * n)], True, 0),
                                    ([str(v) for v in range(2 * n - 40, 2 * n + 40)] + [str(5 * n + 5)], True, 3)):
            q = {"type": "aggregate", "table": "t", "dimensions": ["k"], "metrics": ["count"], "filter": in_filter("time", values, equal)}
            aq = vo.parse_query(tab, q)
            st = vo.scan_aggregate(aq, now=NOW)
            plan = plan_from_query(tab, aq, now=NOW)
            as_in, as_set = dt.query_agg(plan), dt.query_agg(to_inset(plan))
            compare(as_set, st, str(values[:3]))
            assert as_set.scanned_segments == as_in.scanned_segments == st.scanned_segments == want
    finally:
        dt.close()


# ---- 8 / 9. derived layouts: narrow copies and byte planes serve a set plan, bit-sliced planes never do
def test_narrow_copies_and_byte_planes_not_sliced_planes():
    from tests.conftest import JIT_OFF
    J = not JIT_OFF      # (without compiled kernels the interpreting scan answers from the arenas: the rows are still the oracle's, no layout is read)
    tab = typed_table()
    dt = mirror_table(tab)
    try:
        # s16 in 12 bits, d_uint in 6, flag in 1: three bytes of planes per row where the narrowest copies take four (a projection that saves nothing is not built)
        flt = {"op": "and", "filters": [in_filter("s16", ["v%d" % v for v in range(0, 3000, 150)]), F("lt", "d_uint", "30"), in_filter("flag", ["false"], equal=False)]}
        q = {"dimensions": ["s8"], "metrics": ["count", "long_sum"], "filter": flt}
        cols = [storage_index(tab, tab.column(c)) for c in ("s16", "d_uint", "flag")]
        res, st = run(tab, dt, q, flags=FORCE_JIT)
        assert res.jit == J and not res.narrow and not res.predpack
        dt.narrow(cols)
        res, _ = run(tab, dt, q, flags=FORCE_JIT, st=st)
        assert res.jit == J and res.narrow == J and not res.predpack and not res.sliced      # d_uint: values below 61 -> a one-byte copy
        dt.predpack(cols, sliced=False)
        res, _ = run(tab, dt, q, flags=FORCE_JIT, st=st)
        assert res.jit == J and res.predpack == J and not res.sliced
        # ... a filter on the same columns with VH_F_IN leaves is what the layouts were built for: it still reads them (a short list: the
        # bit-serial form of a long one is a text of its own length)
        short = dict(flt, filters=[in_filter("s16", ["v30", "v300", "v2999"])] + flt["filters"][1:])
        aq = vo.parse_query(tab, dict({"type": "aggregate", "table": "t"}, **dict(q, filter=short)))
        assert dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=FORCE_JIT)).predpack == J
        # 9. with the bit-sliced planes present too, the set plan keeps to the byte planes; without them, to the narrow copies
        dt.predpack(cols, sliced=True)
        assert dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=FORCE_JIT)).predpack == J      # (the VH_F_IN plan reads one or the other)
        res, _ = run(tab, dt, q, flags=FORCE_JIT, st=st)
        assert res.jit == J and res.predpack == J and not res.sliced
    finally:
        dt.close()
    dt = mirror_table(tab)
    try:
        dt.predpack(cols, sliced=True)           # only the bit-sliced planes
        res, _ = run(tab, dt, q, flags=FORCE_JIT, st=st)
        assert res.jit == J and not res.sliced and not res.predpack
        for _ in range(4):                       # ... and the automatic builder never answers such a plan with planes it cannot read
            res, _ = run(tab, dt, q, flags=FORCE_JIT, st=st)
            assert not res.sliced
    finally:
        dt.close()


# ---- 10. one code object per shape
def test_one_code_object_whatever_the_list(typed):
    from tests.conftest import JIT_OFF
    tab, dt = typed
    kernels = set()
    for values, search in (([str(v) for v in range(0, 400, 3)], False), ([str(v) for v in range(100, 120000, 37)], False),
                           (["5"], False), (["5", str(5 + 2 ** 20)], True), ([str(v) for v in range(0, 2 ** 31, 2 ** 22)], True)):
        res, _ = run(tab, dt, {"dimensions": ["s8"], "metrics": ["count"], "filter": {"op": "and", "filters": [in_filter("id", values), F("ge", "d_int", "-70")]}}, flags=FORCE_JIT)
        assert res.jit == (not JIT_OFF) and res.inset_search == search
        kernels.add(res.kernel)
    assert len(kernels) == 1, kernels


def test_a_set_larger_than_the_literal_pool(typed):
    """70 000 members — more than the 65 535 literals a filter's REL / IN leaves may carry — beside an ordinary leaf: `id IN {0 .. 69999}` is
    `id < 70000`, which is what the oracle is asked."""
    tab, dt = typed
    q = {"type": "aggregate", "table": "t", "dimensions": ["flag"], "metrics": ["count", "long_sum"],
         "filter": {"op": "and", "filters": [F("lt", "id", "70000"), F("ge", "d_int", "-40")]}}
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=NOW)
    for flags in (0, FORCE_JIT):
        plan = plan_from_query(tab, aq, now=NOW, flags=flags)
        flt = [("inset", f[1], True, list(range(70000))) if f[0] == "rel" and f[1] == storage_index(tab, tab.column("id")) else f for f in plan.filter]
        assert sum(f[0] == "inset" for f in flt) == 1
        res = dt.query_agg(dataclasses.replace(plan, filter=flt))
        compare(res, st, "a set of 70 000 members")
        assert res.inset and not res.inset_search and 0 < res.passed_recs < res.scanned_recs


# ---- 11. select, and the host shim's rewrite of long lists
def test_select_with_a_set_filter(typed):
    from tests.test_gpu_select import oracle_select
    tab, dt = typed
    cols = [storage_index(tab, tab.column(c)) for c in ("id", "s16", "d_long")]
    for flt in (in_filter("id", [str(v) for v in range(3, 120000, 1111)]), in_filter("d_ubyte", [str(v) for v in range(1, 60)], equal=False)):
        q = {"type": "aggregate", "table": "t", "filter": flt}
        plan = to_inset(plan_from_query(tab, vo.parse_query(tab, dict(q, dimensions=[], metrics=["count"])), now=NOW))
        for skip, limit in ((0, 0), (5, 40)):
            got, info = dt.query_select(plan.filter, cols, skip=skip, limit=limit)
            want, stats = oracle_select(tab, q, cols, skip, limit)
            assert info.nrows == stats["output_recs"] > 0 and info.passed_recs == stats["passed_recs"] and info.scanned_segments == stats["scanned_segments"]
            for a, b in zip(got, want):
                assert np.array_equal(a, b.astype(a.dtype))


def test_host_shim_turns_long_lists_into_sets():
    from viyadb_amd import hostdb
    tconf = {"name": "t", "segment_size": 3000, "dimensions": [{"name": "country"}, {"name": "k", "type": "uint"}, {"name": "x", "type": "double"}],
             "metrics": [{"name": "count", "type": "count"}, {"name": "v", "type": "long_sum"}]}
    rnd = np.random.default_rng(3)
    rows = [[["US", "IL", "KZ", "DE"][int(rnd.integers(0, 4))], str(int(rnd.integers(0, 200))), str(int(rnd.integers(0, 200)) / 4), str(int(rnd.integers(-50, 50)))] for _ in range(7000)]
    gdb, odb = hostdb.Database({"tables": [tconf]}), vo.Database({"tables": [tconf]})
    try:
        gdb.load("t", rows, now=NOW)
        odb.table("t").load(rows, now=NOW)
        for flt, want_set in (
                ({"op": "and", "filters": [in_filter("k", [str(v) for v in range(0, 120, 3)]), F("eq", "country", "US")]}, True),       # 40 values + 1: over the limit
                ({"op": "and", "filters": [in_filter("k", [str(v) for v in range(0, 30, 3)]), F("eq", "country", "US")]}, False),       # 10 values: the plan of old
                ({"op": "and", "filters": [in_filter("x", [str(v / 4) for v in range(0, 120, 3)]), F("eq", "country", "US")]}, False),  # a double column keeps VH_F_IN
                ({"op": "and", "filters": [in_filter("x", [str(v / 4) for v in range(0, 120, 3)]), in_filter("k", ["3", "4", "5"])]}, False),           # ... and no set can bring that filter under the limit: its plan stays as it was
                ({"op": "or", "filters": [in_filter("k", [str(v) for v in range(0, 200, 5)], equal=False), in_filter("country", ["IL", "XX"])]}, True)):
            q = {"type": "aggregate", "table": "t", "dimensions": ["country", "k"], "metrics": ["count", "v"], "filter": flt}
            got, gst = gdb.query(q, now=NOW)
            want, _ = odb.query(q, now=NOW)
            assert sorted(map(tuple, got)) == sorted(map(tuple, want)) and len(got) > 0
            assert bool(gst["device_flags"] & capi.INFO_INSET) == want_set, (flt["op"], gst["device_flags"])
    finally:
        gdb.close()
