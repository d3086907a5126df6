"""HIP path vs oracle on typed random tables: every element type as predicate / key / metric,
time rollups, wide keys, hash regrow, segment skipping, size() snapshots, count-distinct."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query

pytestmark = pytest.mark.gpu
NOW = 1496570140


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _rand(rng, dtype, n, small=False):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (rng.integers(-2000, 2000, n) / 8.0).astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = (max(info.min, -60), min(info.max, 60)) if small else (max(info.min, -(2 ** 20)), min(info.max, 2 ** 20))
    return rng.integers(lo, hi, n, endpoint=True).astype(dtype)


TYPES = ["byte", "ubyte", "short", "ushort", "int", "uint", "long", "ulong", "float", "double"]


def typed_table(nseg=3, rows=40_000, seg_size=50_000, seed=7):
    rng = np.random.default_rng(seed)
    dims = [{"name": "d_" + t, "type": t} for t in TYPES]
    dims += [{"name": "s8", "cardinality": 200}, {"name": "s16", "cardinality": 60000}, {"name": "s32"},
             {"name": "flag", "type": "boolean"}, {"name": "ts", "type": "time"}, {"name": "uts", "type": "microtime"},
             {"name": "id", "type": "uint"}]
    mets = [{"name": "count", "type": "count"}]
    for t in TYPES:
        for a in ("sum", "min", "max", "avg"):
            mets.append({"name": f"{t}_{a}", "type": f"{t}_{a}"})
    tab = vo.Table({"name": "t", "segment_size": seg_size, "dimensions": dims, "metrics": mets})
    for nm, card in (("s8", 150), ("s16", 3000), ("s32", 5000)):
        dic = tab.dicts[nm]
        for i in range(card):
            dic.v2c["v%d" % i] = len(dic.c2v)
            dic.c2v.append("v%d" % i)
    for s in range(nseg):
        d = [_rand(rng, vo.NUMERIC_TYPES[t][0], rows, small=True) for t in TYPES]
        d.append(rng.integers(0, 151, rows).astype(np.uint8))
        d.append(rng.integers(0, 3001, rows).astype(np.uint16))
        d.append(rng.integers(0, 5001, rows).astype(np.uint32))
        d.append(rng.integers(0, 2, rows).astype(np.uint8))
        d.append(rng.integers(NOW - 2 * 365 * 86400, NOW, rows).astype(np.uint32))
        d.append((rng.integers(NOW - 400 * 86400, NOW, rows).astype(np.uint64) * np.uint64(1000000) + rng.integers(0, 10 ** 6, rows).astype(np.uint64)))
        d.append(np.arange(s * rows, (s + 1) * rows, dtype=np.uint32))
        m = [rng.integers(1, 4, rows).astype(np.uint32)]
        for t in TYPES:
            for a in ("sum", "min", "max", "avg"):
                m.append(_rand(rng, vo.NUMERIC_TYPES[t][0], rows, small=(a in ("sum", "avg") and t in ("byte", "ubyte", "short", "ushort"))))
        tab.add_segment_arrays(d, m, None, rows)
    return tab


@pytest.fixture(scope="module")
def typed():
    tab = typed_table()
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


def run(tab, dt, q, flags=0, now=NOW, groups_hint=0, seg_rows=None):
    q = dict({"type": "aggregate", "table": "t"}, **q)
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=now, seg_rows=seg_rows)
    res = dt.query_agg(plan_from_query(tab, aq, now=now, flags=flags, groups_hint=groups_hint, seg_rows=seg_rows))
    compare(res, st, str(q))
    return res, st


def F(op, col, val):
    return {"op": op, "column": col, "value": str(val)}


@pytest.mark.parametrize("t", [x for x in TYPES if x not in ("byte", "short")])
@pytest.mark.parametrize("op", ["eq", "ne", "lt", "le", "gt", "ge"])
def test_predicate_on_every_type(typed, t, op):
    tab, dt = typed
    val = "3.5" if t in ("float", "double") else "7"
    q = {"dimensions": ["s8"], "metrics": ["count", "long_sum"], "filter": F(op, "d_" + t, val)}
    r0, _ = run(tab, dt, q)
    run(tab, dt, q, flags=8)


def test_fast_kernel_is_taken_when_eligible(typed):
    """4-byte predicate columns (u32 / i32 / f32 / time) take the register-resident kernel; others do not."""
    tab, dt = typed
    q4 = {"dimensions": ["s8"], "metrics": ["count"], "filter": {"op": "and", "filters": [
        F("lt", "d_uint", "40"), F("gt", "d_int", "-40"), F("ne", "d_float", "1.5"), F("gt", "ts", "1000")]}}
    for flags, want in ((0, True), (8, False)):
        aq = vo.parse_query(tab, dict({"type": "aggregate", "table": "t"}, **q4))
        res = dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=flags))
        compare(res, vo.scan_aggregate(aq, now=NOW), "fast=%s" % want)
        assert res.fast == want
    # (an 8-byte predicate column: register-resident only in a kernel compiled for the plan, which a table this small does not get unasked)
    from viyadb_amd import capi
    aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": ["s8"], "metrics": ["count"], "filter": F("lt", "d_ulong", "5")})
    assert dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=capi.PLAN_NO_JIT)).fast is False
    res = dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=capi.PLAN_FORCE_JIT))
    compare(res, vo.scan_aggregate(aq, now=NOW), "u64 predicate, compiled kernel")
    from tests.conftest import JIT_OFF
    assert JIT_OFF or (res.fast and res.jit and res.kernel.startswith("viya_jit_scan_"))


@pytest.mark.parametrize("t", [x for x in TYPES if x not in ("byte", "short")])
def test_metric_predicates(typed, t):
    tab, dt = typed
    run(tab, dt, {"dimensions": ["flag"], "metrics": ["count"], "filter": {"op": "and", "filters": [
        F("gt", t + "_max", "-5"), {"op": "or", "filters": [F("lt", t + "_min", "100"), F("eq", "count", "2")]}]}})


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("flags", [0, 1, 8, 9, 16, 48, 64])
def test_all_aggregations_per_type(typed, t, flags):
    tab, dt = typed
    run(tab, dt, {"dimensions": ["s8", "flag"], "metrics": ["count"] + [f"{t}_{a}" for a in ("sum", "min", "max", "avg")],
                  "filter": F("lt", "d_uint", "20")}, flags=flags)


@pytest.mark.parametrize("t", TYPES)
def test_avg_without_count_uses_hidden_count(t):
    rng = np.random.default_rng(3)
    tab = vo.Table({"name": "t", "segment_size": 20000, "dimensions": [{"name": "k", "type": "ushort"}],
                    "metrics": [{"name": "a", "type": t + "_avg"}]})
    for _ in range(2):
        n = 15000
        tab.add_segment_arrays([rng.integers(0, 300, n).astype(np.uint16)], [_rand(rng, vo.NUMERIC_TYPES[t][0], n, small=True)],
                               rng.integers(1, 5, n).astype(np.uint64), n)
    dt = mirror_table(tab)
    try:
        res, st = run(tab, dt, {"dimensions": ["k"], "metrics": ["a"]})
        assert res.hidden_count is not None
    finally:
        dt.close()


@pytest.mark.parametrize("dims", [["d_byte", "d_float", "d_double"], ["d_ulong", "d_long"], ["s8", "s16", "s32", "flag", "d_short"],
                                  ["d_ubyte"], ["id"], ["d_int", "d_uint", "d_ushort", "d_ubyte", "d_byte", "d_short", "d_long", "d_ulong"]])
@pytest.mark.parametrize("flags", [0, 1])
def test_group_key_shapes(typed, dims, flags):
    """Narrow, 64-bit-packed and wide (multi-word, incl. float/double) keys."""
    tab, dt = typed
    run(tab, dt, {"dimensions": dims, "metrics": ["count", "int_sum", "double_max"], "filter": F("ge", "d_int", "-30")}, flags=flags)


@pytest.mark.parametrize("flags", [0, 16, 64, 48])
def test_partitioned_aggregation_shapes(typed, flags):
    """Group-id spaces of 10K-150K ids with 1-4 metrics of mixed widths (tuple packing), through the
    radix-partitioned path and, for comparison, direct global atomics."""
    tab, dt = typed
    for dims, mets in ((["s16", "flag"], ["count"]), (["s16", "d_ubyte"], ["long_sum", "count", "int_min", "double_max"]),
                       (["s32", "flag"], ["float_sum", "uint_max", "short_sum"]), (["s16"], ["ulong_min", "long_max"]),
                       (["s8", "s16"], ["int_avg", "count"])):
        res, _ = run(tab, dt, {"dimensions": dims, "metrics": mets, "filter": F("lt", "d_uint", "45")}, flags=flags)
        assert res.path in ("dense_part", "dense_global", "dense_lds", "hash")


def test_partition_buffer_regrows():
    """Every row survives: the tuple extents planned for 1/8 of the rows overflow and the query is re-run."""
    rng = np.random.default_rng(21)
    n = 60000
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}]})
    for _ in range(3):
        tab.add_segment_arrays([rng.integers(0, 300, n).astype(np.uint32), rng.integers(0, 200, n).astype(np.uint32)],
                               [rng.integers(-1000, 1000, n).astype(np.int64), np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("ge", "a", "0")})
        assert res.path == "dense_global"        # ~100 % pass, but 180 K rows do not pay for the second phase: direct atomics
        import os
        for flags, lanes in ((64 | 128, False), (64, True)):   # compacting and lanes form of phase 1
            os.environ["VH_TEST_PART_EXTENTS"] = "40"          # first attempt runs out of tuple extents -> re-run with more room
            try:
                res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("ge", "a", "0")}, flags=flags)
            finally:
                del os.environ["VH_TEST_PART_EXTENTS"]
            assert res.path == "dense_part" and res.retries >= 1 and res.lanes == lanes
            res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("ge", "a", "0")}, flags=flags)
            assert res.path == "dense_part" and res.retries == 0 and res.lanes == lanes
        # skew: everything lands in one partition
        res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("eq", "a", "7")}, flags=64)
        res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("lt", "a", "3")})
        assert res.path == "dense_global"        # ~1 %: direct atomics
    finally:
        dt.close()


def test_two_level_partitioning():
    """Group-id spaces of more than 64 LDS-sized ranges: phase 1 partitions coarsely, part_split_kernel splits every partition 64
    ways, phase 2 aggregates up to 4096 ranges in LDS. Compacting and lanes form of phase 1, both pools overflowing, skew (one
    coarse partition, one sub-partition), sparse occupancy, against the oracle and the direct-atomics plan."""
    import os
    from viyadb_amd import capi
    rng = np.random.default_rng(33)
    n = 400000
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "uint"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}, {"name": "lo", "type": "int_min"}, {"name": "hi", "type": "uint_max"}]})
    for _ in range(3):
        tab.add_segment_arrays([rng.integers(0, 3000, n).astype(np.uint32), rng.integers(0, 700, n).astype(np.uint32), rng.integers(0, 100, n).astype(np.uint32)],
                               [rng.integers(-10**12, 10**12, n).astype(np.int64), rng.integers(1, 4, n).astype(np.uint32),
                                rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), rng.integers(0, 2**32 - 1, n).astype(np.uint32)], None, n)
    dt = mirror_table(tab)
    q = {"dimensions": ["a", "b"], "metrics": ["v", "count"], "filter": F("lt", "f", "50")}
    try:
        res, _ = run(tab, dt, q)
        assert res.path == "dense_global"                       # 0.6 M survivors do not pay for two more passes
        for flags, lanes in ((64 | 128, False), (64, False), (64 | 256, True)):
            qq = dict(q, filter=F("ge", "f", "0") if lanes else F("lt", "f", "30"))
            res, _ = run(tab, dt, qq, flags=flags)
            assert res.path == "dense_part" and "part_split_" in res.kernel and res.lanes == lanes and res.retries == 0, (res.path, res.kernel, res.lanes)
            if not lanes:       # two unsigned group columns, SUM(long) + SUM(uint): the pre-built specialised drain, the generic one on request,
                                # and phase 1 compiled for the plan (the split and phase 2 do not care who wrote the tuples)
                if not res.jit:
                    assert "scan_agg_shape_kernel" in res.kernel, res.kernel
                res, _ = run(tab, dt, qq, flags=flags | capi.PLAN_NO_SHAPE | capi.PLAN_NO_JIT)
                assert res.path == "dense_part" and "scan_agg_fast_kernel" in res.kernel, res.kernel
                res, _ = run(tab, dt, qq, flags=flags | capi.PLAN_FORCE_JIT)
                from tests.conftest import JIT_OFF
                assert res.path == "dense_part" and (res.jit or JIT_OFF) and ("viya_jit_scan_" in res.kernel or JIT_OFF) and "part_split_" in res.kernel, res.kernel
            res, _ = run(tab, dt, qq, flags=flags | capi.PLAN_NO_PART2)
            assert res.path == "dense_global"
        # the specialised drain's other forms: metrics in the other order, one group column, narrow unsigned keys elsewhere in the suite
        res, _ = run(tab, dt, dict(q, metrics=["count", "v"]), flags=64 | 128)
        assert "scan_agg_shape_kernel<4, 256, 4, 1, 2>" in res.kernel, res.kernel
        res, _ = run(tab, dt, {"dimensions": ["a"], "metrics": ["v", "count"], "filter": F("lt", "f", "50")}, flags=64 | 128)
        assert res.path != "dense_part" or "scan_agg_shape_kernel" in res.kernel, (res.path, res.kernel)
        # four metrics (wide tuples), MIN / MAX states
        res, _ = run(tab, dt, dict(q, metrics=["v", "count", "lo", "hi"]), flags=64)
        assert "part_split_" in res.kernel
        # one- and two-word tuples are split through the ring writer (extents by position + the slices' overflow regions, no barriers); wider tuples
        # (four metrics above) tuple by tuple
        res, _ = run(tab, dt, q, flags=64 | 128)
        assert "part_split_ring_kernel" in res.kernel and res.retries == 0, (res.kernel, res.retries)
        res, _ = run(tab, dt, dict(q, metrics=["v", "count", "lo", "hi"]), flags=64)
        assert "part_split_kernel<256>" in res.kernel, res.kernel
        # either pool too small at first: the query re-plans with more room
        for var in ("VH_TEST_PART_EXTENTS", "VH_TEST_PART_EXTENTS2"):
            os.environ[var] = "50"
            try:
                res, _ = run(tab, dt, q, flags=64 | 128)
            finally:
                del os.environ[var]
            assert res.path == "dense_part" and res.retries >= 1 and "part_split_ring_kernel" in res.kernel, (var, res.retries, res.kernel)      # (the re-run: a bigger pool, the same writer)
        # ... and with few or no positional extents every tuple of both pools goes through the overflow regions (what a hot key does to one stream)
        for levels in ("0", "1"):
            os.environ["VH_TEST_POS_LEVELS"] = levels
            try:
                for qq in (q, dict(q, filter=F("lt", "a", "5")), dict(q, filter={"op": "and", "filters": [F("eq", "a", "2999"), F("eq", "b", "699")]})):
                    res, _ = run(tab, dt, qq, flags=64 | 128 | capi.PLAN_FORCE_JIT)
                    assert res.path == "dense_part" and res.retries == 0 and "part_split_ring_kernel" in res.kernel, (levels, res.retries, res.kernel)
            finally:
                del os.environ["VH_TEST_POS_LEVELS"]
        # skew: one coarse partition; one single group
        run(tab, dt, dict(q, filter=F("lt", "a", "5")), flags=64)
        run(tab, dt, dict(q, filter={"op": "and", "filters": [F("eq", "a", "2999"), F("eq", "b", "699")]}), flags=64)
        run(tab, dt, dict(q, filter=F("gt", "f", "1000")), flags=64)      # nothing survives
    finally:
        dt.close()
    # one group column through the specialised drain (the host gives it a second digit that counts for nothing)
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "k", "type": "uint"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}]})
    for _ in range(2):
        tab.add_segment_arrays([rng.integers(0, 200000, n).astype(np.uint32), rng.integers(0, 100, n).astype(np.uint32)],
                               [rng.integers(-10**12, 10**12, n).astype(np.int64), rng.integers(1, 4, n).astype(np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        for mets in (["v", "count"], ["count", "v"]):
            res, _ = run(tab, dt, {"dimensions": ["k"], "metrics": mets, "filter": F("lt", "f", "40")}, flags=64 | 128)
            assert res.path == "dense_part" and "scan_agg_shape_kernel" in res.kernel, (res.path, res.kernel)
            run(tab, dt, {"dimensions": ["k"], "metrics": mets, "filter": F("lt", "f", "40")}, flags=64 | 128 | capi.PLAN_NO_SHAPE)
    finally:
        dt.close()
    # 1.5 M groups, three out of four empty (a dense table is planned up to 4 groups per row)
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "uint"}],
                    "metrics": [{"name": "count", "type": "count"}]})
    tab.add_segment_arrays([rng.integers(0, 2000, n).astype(np.uint32), rng.integers(0, 750, n).astype(np.uint32)], [np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        res, _ = run(tab, dt, {"dimensions": ["a", "b"], "metrics": ["count"]}, flags=64)
        assert res.path == "dense_part" and "part_split_" in res.kernel, (res.path, res.kernel)
    finally:
        dt.close()


def test_few_partitions_every_row_passing_through_the_ring_writer():
    """Three LDS-sized ranges and no filter: every drain of 64 survivors puts ~21 tuples into each of three partitions — more than the two waiting lines
    per partition hold — so lanes of one call take their ring places in rounds, a line's owner flushes while later lanes of the same call still wait,
    and four waves of a block do so at once (vh_ring_add_tb's `gen` / `done` counters at their busiest). One-word and two-word tuples, compiled kernel."""
    from tests.conftest import JIT_OFF
    if JIT_OFF:
        pytest.skip("the ring writer lives in the compiled kernels")
    import os
    from viyadb_amd import capi
    rng = np.random.default_rng(77)
    n = 500_000
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "uint"}],
                    "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}]})
    for _ in range(2):
        tab.add_segment_arrays([rng.integers(0, 150, n).astype(np.uint32), rng.integers(0, 150, n).astype(np.uint32)],
                               [rng.integers(0, 1000, n).astype(np.int64), np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    q = {"dimensions": ["a", "b"], "metrics": ["v", "count"]}
    try:
        for flags in (capi.PLAN_FORCE_PART | capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES, capi.PLAN_FORCE_PART | capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES | capi.PLAN_NO_NARROW_TUPLES):
            res, st = run(tab, dt, q, flags=flags)
            assert res.path == "dense_part" and res.jit and res.retries == 0 and res.ngroups == st.ngroups == 22500, (res.path, res.kernel, res.retries, res.ngroups)
    finally:
        dt.close()


def test_two_level_on_typed_shapes(typed):
    """The typed table's group spaces are small; with 1 KB LDS tables (VH_PART_TABLE_KB) they still split into hundreds of ranges,
    so every state type (float / double SUM, MIN / MAX of every width, AVG, narrow sums) goes through both partition levels."""
    import os
    tab, dt = typed
    os.environ["VH_PART_TABLE_KB"] = "1"
    try:
        two = 0
        for dims, mets in ((["s16", "d_ubyte"], ["count", "long_sum"]), (["s16", "d_ushort"], ["double_sum", "float_max", "count"]),
                           (["d_ushort", "flag", "s8"], ["int_min", "uint_max", "long_max", "count"]), (["s16", "s8"], ["int_avg", "count", "double_min"]),
                           (["d_uint"], ["short_sum", "byte_max", "count"]), (["d_ushort", "d_ubyte"], ["ulong_sum"])):
            for flags in (64, 64 | 128):
                for flt in (F("lt", "d_uint", "45"), F("ge", "d_uint", "0")):
                    try:
                        res, _ = run(tab, dt, {"dimensions": dims, "metrics": mets, "filter": flt}, flags=flags)
                    except vo.Unsupported:
                        continue
                    two += "part_split_" in res.kernel
        assert two >= 8, two
    finally:
        del os.environ["VH_PART_TABLE_KB"]


def test_in_and_not_in(typed):
    tab, dt = typed
    for flt in ({"op": "in", "column": "s8", "values": ["v1", "v7", "v9", "nope"]},
                {"op": "not", "filter": {"op": "in", "column": "d_ubyte", "values": ["1", "2", "3", "40"]}},
                {"op": "or", "filters": [{"op": "in", "column": "d_long", "values": ["5", "-5"]}, F("eq", "flag", "true")]}):
        run(tab, dt, {"dimensions": ["s16"], "metrics": ["count"], "filter": flt})


@pytest.mark.parametrize("gran", ["year", "month", "day", "hour", "minute", "second"])
@pytest.mark.parametrize("col", ["ts", "uts"])
def test_query_granularity(typed, gran, col):
    tab, dt = typed
    run(tab, dt, {"select": [{"column": col, "granularity": gran}, {"column": "count"}], "filter": F("lt", "d_ubyte", "30")})


@pytest.mark.parametrize("micro", [False, True])
def test_rollup_rules_at_query_time(micro):
    rng = np.random.default_rng(11)
    n = 30000
    rules = [{"granularity": "hour", "after": "1 days"}, {"granularity": "day", "after": "1 weeks"}, {"granularity": "month", "after": "1 years"}]
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "ts", "type": "microtime" if micro else "time", "rollup_rules": rules},
                                                                    {"name": "u", "type": "uint"}],
                    "metrics": [{"name": "count", "type": "count"}]})
    for _ in range(2):
        ts = rng.integers(NOW - 3 * 365 * 86400, NOW, n).astype(np.uint64)
        if micro:
            ts = ts * np.uint64(1000000) + rng.integers(0, 10 ** 6, n).astype(np.uint64)
        tab.add_segment_arrays([ts.astype(np.uint64 if micro else np.uint32), rng.integers(0, 5, n).astype(np.uint32)],
                               [rng.integers(1, 3, n).astype(np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        run(tab, dt, {"dimensions": ["ts", "u"], "metrics": ["count"]})
        run(tab, dt, {"select": [{"column": "ts", "granularity": "month"}, {"column": "count"}]})
    finally:
        dt.close()


@pytest.mark.parametrize("flags", [0, 1, 64, 1 | (1 << 18) | (1 << 20)])      # (the last: hashed partitioning where the plan allows it — its groups then go through the list of records, not straight into the output columns)
def test_having_on_device(typed, flags):
    """HAVING evaluated by the group-emission kernel. Keys, SUM, AVG (raw sum), MIN/MAX, IN, nested and/or."""
    from tests.having import apply_keep, having_nodes, keep_mask
    tab, dt = typed
    cases = [
        ({"dimensions": ["s8", "flag"], "metrics": ["count", "long_sum", "double_max", "int_avg"]},
         {"op": "and", "filters": [F("gt", "count", "300"), {"op": "or", "filters": [F("lt", "long_sum", "0"), F("ge", "double_max", "200")]}]}),
        ({"dimensions": ["s16"], "metrics": ["int_avg", "count"]}, F("gt", "int_avg", "5")),
        ({"dimensions": ["d_int", "d_float"], "metrics": ["ushort_min"]}, {"op": "or", "filters": [F("lt", "d_int", "-10"), F("eq", "d_float", "2.5")]}),
        ({"dimensions": ["s8"], "metrics": ["count"]}, {"op": "in", "column": "s8", "values": ["v3", "v4", "zzz"]}),
        ({"dimensions": ["s8"], "metrics": ["count"]}, {"op": "not", "filter": {"op": "in", "column": "s8", "values": ["v3", "v4"]}}),
    ]
    for sel, hv in cases:
        q = dict({"type": "aggregate", "table": "t", "filter": F("lt", "d_uint", "50"), "having": hv}, **sel)
        aq = vo.parse_query(tab, q)
        st = vo.scan_aggregate(aq, now=NOW)
        total = st.ngroups
        # oracle side: the same ComparisonBuilder semantics on the aggregated tuples (post_agg.cc:77-83) — tests/having.py
        keep = keep_mask(tab, aq, st)
        apply_keep(st, keep)
        plan = plan_from_query(tab, aq, now=NOW, flags=flags)
        plan.having = having_nodes(tab, aq)
        res = dt.query_agg(plan)
        assert res.ngroups == total and res.returned == int(keep.sum()), (q, res.ngroups, total, res.returned, int(keep.sum()))
        res.ngroups = res.returned
        compare(res, st, str(q))


def test_hash_table_regrows(typed):
    tab, dt = typed
    res, _ = run(tab, dt, {"dimensions": ["id", "d_double"], "metrics": ["count"]}, flags=1, groups_hint=1)
    assert res.retries >= 1 and res.ngroups == 120000
    res, _ = run(tab, dt, {"dimensions": ["id"], "metrics": ["count", "long_sum", "int_min", "double_max"]}, flags=1 | 2048, groups_hint=1)
    assert res.retries >= 1 and res.path == "hash"       # single-word key: the table of records regrows as well


def test_segment_skipping_and_snapshot():
    n, nseg = 20000, 6
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "time", "type": "ulong"}, {"name": "k", "type": "ubyte"}],
                    "metrics": [{"name": "count", "type": "count"}]})
    rng = np.random.default_rng(5)
    for s in range(nseg):
        tab.add_segment_arrays([np.arange(s * n, (s + 1) * n, dtype=np.uint64), rng.integers(0, 9, n).astype(np.uint8)],
                               [np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        res, st = run(tab, dt, {"dimensions": ["k"], "metrics": ["count"], "filter": F("gt", "time", 4 * n + 5)})
        assert res.scanned_segments == 2 and res.scanned_recs == n * nseg
        res, _ = run(tab, dt, {"dimensions": ["k"], "metrics": ["count"], "filter": {"op": "in", "column": "time", "values": [str(n + 1), str(3 * n)]}})
        assert res.scanned_segments == 2
        # NOT IN takes the same min/max expression in the reference (equal() is ignored): quirk kept
        res, _ = run(tab, dt, {"dimensions": ["k"], "metrics": ["count"], "filter": {"op": "not", "filter": {"op": "in", "column": "time", "values": [str(n + 1)]}}})
        assert res.scanned_segments == 1
        # size() snapshot smaller than what is mirrored: later rows are invisible
        snap = [n, n - 17, 5, 0, n, 1]
        res, _ = run(tab, dt, {"dimensions": ["k"], "metrics": ["count"]}, seg_rows=snap)
        assert res.scanned_recs == sum(snap)
    finally:
        dt.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("flags", [0, 1, 1 | 2048])      # dense table; hash table as arrays; hash table as records
def test_count_distinct(wide, flags):
    rng = np.random.default_rng(9)
    n = 8000
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "c", "type": "ushort"}, {"name": "x", "type": "uint"}],
                    "metrics": [{"name": "users", "type": "bitset", "max": 2 ** 40 if wide else 2 ** 31},
                                {"name": "count", "type": "count"}]})
    for _ in range(3):
        sets = [set(int(v) for v in rng.integers(0, 500 if not wide else 2 ** 36, rng.integers(0, 4))) for _ in range(n)]
        tab.add_segment_arrays([rng.integers(0, 40, n).astype(np.uint16), rng.integers(0, 100, n).astype(np.uint32)],
                               [sets, np.ones(n, dtype=np.uint32)], None, n)
    dt = mirror_table(tab)
    try:
        run(tab, dt, {"dimensions": ["c"], "metrics": ["users", "count"], "filter": F("lt", "x", "60")}, flags=flags)
        run(tab, dt, {"dimensions": [], "metrics": ["users"]}, flags=flags)
        # the bitset metric in the FILTER: the predicate compares the row's own cardinality (filter.cc:216,235)
        res, st = run(tab, dt, {"dimensions": ["c"], "metrics": ["users", "count"], "filter": F("ge", "users", "2")}, flags=flags)
        assert 0 < st.passed_recs < st.scanned_recs
        run(tab, dt, {"dimensions": ["c"], "metrics": ["count"],
                      "filter": {"op": "and", "filters": [{"op": "in", "column": "users", "values": ["1", "3"]}, F("lt", "x", "80")]}}, flags=flags)
        run(tab, dt, {"dimensions": ["c"], "metrics": ["count"], "filter": {"op": "not", "filter": {"op": "in", "column": "users", "values": ["0", "2"]}}}, flags=flags)
    finally:
        dt.close()


def _ref_sort_key(v, dtype):
    """The reference's sort order of a formatted value: INTEGER columns compare (length, text) (src/util/string.h:28-49),
    FLOAT columns compare stod of the "%.15g" / "%g" text."""
    if np.dtype(dtype).kind == "f":
        return float(("%g" if np.dtype(dtype) == np.float32 else "%.15g") % float(v))
    s = str(int(v))
    return (len(s), s)


@pytest.mark.parametrize("metric", ["long_max", "int_min", "ulong_sum", "uint_max", "short_sum", "float_sum", "double_min", "count"])
@pytest.mark.parametrize("desc", [True, False])
def test_device_top_n_keeps_a_superset(typed, metric, desc):
    """sort + limit on a numeric column. The device must return every group that ties with or beats
    the k-th in the REFERENCE's order (string length first for integers, so -5 > 3), and far fewer than all groups."""
    import dataclasses
    tab, dt = typed
    q = {"type": "aggregate", "table": "t", "dimensions": ["id"], "metrics": [metric, "count"], "filter": F("ge", "d_int", "-50")}
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=NOW)
    assert st.ngroups > 100_000
    vals = st.states[0]
    keys = [_ref_sort_key(v, vals.dtype) for v in vals]
    for k in (1, 10, 1000):
        plan = dataclasses.replace(plan_from_query(tab, aq, now=NOW), top=(1, desc, k))
        res = dt.query_agg(plan)
        assert res.ngroups == st.ngroups
        order = sorted(range(len(keys)), key=lambda i: keys[i], reverse=desc)
        kth = keys[order[k - 1]]
        required = {int(st.keys[0][i]) for i in range(len(keys)) if (keys[i] >= kth if desc else keys[i] <= kth)}
        got = {int(x) for x in res.keys[0]}
        assert required <= got, (metric, desc, k, len(required - got))
        assert res.returned == len(got) and len(got) <= len(required) + 3000, (metric, desc, k, len(got), len(required))
        # the kept rows carry their true states
        pos = {int(x): i for i, x in enumerate(st.keys[0])}
        idx = np.array([pos[int(x)] for x in res.keys[0]])
        assert np.array_equal(res.states[0], vals[idx]) and np.array_equal(res.states[1], st.states[1][idx])


@pytest.mark.parametrize("dims,metrics,eligible", [
    (["d_int"], ["long_sum", "int_min"], True), (["d_long"], ["float_sum", "double_max"], True),
    (["d_uint"], ["uint_max", "ulong_min"], True), (["d_ulong"], ["count", "int_avg"], True),
    (["d_int"], ["double_sum"], True), (["d_uint"], ["long_max", "float_min"], True),
    (["d_int"], ["short_sum", "long_sum"], False),       # 2-byte payload column
    (["d_int", "flag"], ["long_sum"], False),            # 1-byte group column
    (["d_int"], ["long_sum", "int_min", "count"], False)])  # 3 metrics
def test_lanes_kernel_matches_oracle(typed, dims, metrics, eligible):
    """The no-compaction kernel (high selectivity, LDS table): every 4/8-byte element type as group / metric column,
    segment tails, the fall-back to the compacting kernel when the plan is not eligible, and the probe-driven choice."""
    tab, dt = typed
    many, few = F("ge", "d_int", "-30"), F("lt", "d_uint", "3")      # ~75 % / ~5 % of the rows pass
    for flt in (many, few):
        q = {"dimensions": dims, "metrics": metrics, "filter": flt}
        res, _ = run(tab, dt, q, flags=256)       # forced whenever eligible
        assert res.path == "dense_lds" and res.lanes == eligible, (dims, metrics)
        res, _ = run(tab, dt, q, flags=128)       # never
        assert not res.lanes
        res, _ = run(tab, dt, q)                  # by the selectivity probe
        assert res.lanes == (eligible and flt is many)
    # no filter at all: every row passes, no predicate column is loaded, still the register-resident kernels
    res, _ = run(tab, dt, {"dimensions": dims, "metrics": metrics})
    assert res.fast and res.lanes == eligible


@pytest.mark.parametrize("sel,eligible", [
    ([{"column": "ts", "granularity": "day"}, {"column": "count"}, {"column": "long_sum"}], True),
    ([{"column": "uts", "granularity": "month"}, {"column": "double_max"}], True),
    ([{"column": "d_float"}, {"column": "count"}, {"column": "float_min"}], True),
    ([{"column": "ts", "granularity": "hour"}, {"column": "d_uint"}, {"column": "int_sum"}, {"column": "ulong_max"}], True),
    ([{"column": "d_double"}, {"column": "d_int"}, {"column": "count"}], False),          # 96-bit key: two words, no LDS front table
    ([{"column": "ts", "granularity": "day"}, {"column": "flag"}, {"column": "count"}], False)])   # 1-byte group column
def test_lanes_kernel_on_the_hash_path(typed, sel, eligible):
    """Time buckets / float keys with most rows passing: the no-compaction kernel over the LDS front table, rows that
    find no LDS slot falling through to the HBM table; against the oracle, forced on, forced off, and by the probe."""
    tab, dt = typed
    many, few = F("ge", "d_int", "-30"), F("lt", "d_uint", "3")
    for flt in (many, few, None):
        q = {"select": sel}
        if flt:
            q["filter"] = flt
        res, st = run(tab, dt, q, flags=256)
        small = st.ngroups <= 2000      # the host skips the front table once it has seen far more groups than it holds
        assert res.path == "hash" and (res.lanes == eligible or not small), sel
        assert not run(tab, dt, q, flags=128)[0].lanes
        assert not run(tab, dt, q, flags=512)[0].lanes        # no LDS front table -> nothing for the lanes kernel to use
        res = run(tab, dt, q)[0]         # probe-driven: only when (nearly) every row passes; 75 % is too close to call
        if small and flt is not many:
            assert res.lanes == (eligible and flt is None)


@pytest.mark.parametrize("seed", list(range(int(__import__("os").environ.get("VH_FUZZ_SEEDS", "8")))))   # VH_FUZZ_SEEDS=300: bug hunt
def test_random_plans_against_oracle(typed, seed):
    """Seeded random queries over the typed table — random group columns (dict codes of three widths, every numeric type,
    bool, time with a random granularity), random metrics, random filter trees (rel / in / not / and / or, two levels),
    random plan flags — each compared with the oracle. Catches interactions no hand-written case thought of."""
    import random
    rnd = random.Random(1000 + seed)
    tab, dt = typed
    dims_pool = ["s8", "s16", "s32", "flag", "d_ubyte", "d_short", "d_ushort", "d_int", "d_uint", "d_long", "d_ulong", "d_float", "d_double", "id"]
    metric_pool = ["count"] + [f"{t}_{a}" for t in TYPES for a in ("sum", "min", "max", "avg")]
    filt_cols = [("d_int", lambda: rnd.randrange(-60, 61)), ("d_uint", lambda: rnd.randrange(0, 61)), ("d_long", lambda: rnd.randrange(-60, 61)),
                 ("d_ulong", lambda: rnd.randrange(0, 61)), ("d_float", lambda: rnd.randrange(-200, 200) / 8.0), ("d_double", lambda: rnd.randrange(-200, 200) / 8.0),
                 ("d_ubyte", lambda: rnd.randrange(0, 61)), ("d_ushort", lambda: rnd.randrange(0, 61)), ("s8", lambda: "v%d" % rnd.randrange(0, 160)),
                 ("flag", lambda: rnd.choice(["true", "false"])), ("ts", lambda: NOW - rnd.randrange(0, 2 * 365 * 86400)),
                 ("count", lambda: rnd.randrange(1, 4)), ("int_sum", lambda: rnd.randrange(-2 ** 19, 2 ** 19)), ("double_max", lambda: rnd.randrange(-200, 200) / 8.0)]

    def leaf():
        col, gen = rnd.choice(filt_cols)
        if rnd.random() < 0.2:
            return {"op": "in", "column": col, "values": [str(gen()) for _ in range(rnd.randrange(1, 5))]}
        op = rnd.choice(["eq", "ne", "lt", "le", "gt", "ge"]) if col not in ("s8", "flag") else rnd.choice(["eq", "ne"])
        return F(op, col, gen())

    def tree(depth):
        r = rnd.random()
        if depth == 0 or r < 0.35:
            f = leaf()
        else:
            f = {"op": rnd.choice(["and", "or"]), "filters": [tree(depth - 1) for _ in range(rnd.randrange(2, 4))]}
        return {"op": "not", "filter": f} if rnd.random() < 0.15 else f

    flag_pool = [0, 0, 0, 1, 2, 8, 9, 16, 48, 64, 128, 256, 512, 64 | 256, 1 | 512, 8 | 64, 1 | 2048, 9 | 2048, 1 | 2048 | 512, 2048,
                 8192, 8192 | 1, 8192 | 8, 8192 | 64, 8192 | 2, 8192 | 128, 8192 | 1 | 2048,      # 8192: gather from a payload projection
                 64 | 32768, 64 | 16384, 64 | 8192 | 32768, 65536, 65536 | 64, 65536 | 1,                                 # 32768 / 16384 / 65536: no specialised drain / no second partition level / no narrow predicate copies
                 1 | (1 << 18) | (1 << 20), 1 | (1 << 18) | (1 << 20), 1 | (1 << 18) | (1 << 20) | 8192]                      # hashed partitioning where the plan allows it (one key word, a payload of <= 64 bits)
    done = 0
    for _ in range(40):
        sel = []
        for d in rnd.sample(dims_pool, rnd.randrange(0, 4)):
            sel.append({"column": d})
        if rnd.random() < 0.3:
            sel.append({"column": "ts", "granularity": rnd.choice(["year", "month", "day", "hour", "minute"])})
        ms = rnd.sample(metric_pool, rnd.randrange(1, 5))
        if any(m.endswith("_avg") for m in ms) and "count" not in ms:
            ms.append("count")        # an AVG without the table's COUNT does not compile in the reference
        for m in ms:
            sel.append({"column": m})
        rnd.shuffle(sel)
        q = {"select": sel}
        if rnd.random() < 0.85:
            q["filter"] = tree(2)
        flags = rnd.choice(flag_pool)
        try:
            run(tab, dt, q, flags=flags)
            done += 1
        except vo.Unsupported:     # e.g. a filter on a byte / short column
            continue
    assert done >= 30


def test_result_handles_own_their_state(typed):
    """A vh_result owns an execution context (device scratch + pinned staging) from launch to vh_result_free: other queries
    on the table in between must not disturb it — launched handles finalise later, finalised ones keep their rows and
    can still be regrouped on the device. Bad table descriptors and segment indices are rejected."""
    import ctypes as C
    from viyadb_amd import capi
    tab, dt = typed
    q = dict({"type": "aggregate", "table": "t"}, dimensions=["s8"], metrics=["count", "long_sum"])
    q2 = dict({"type": "aggregate", "table": "t"}, dimensions=["s16", "flag"], metrics=["count", "int_max"])
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=NOW)
    plan = plan_from_query(tab, aq, now=NOW)
    plan2 = plan_from_query(tab, vo.parse_query(tab, q2), now=NOW)
    launched = [dt.query_launch(plan) for _ in range(3)]    # three partials in flight on one table
    for _ in range(3):
        dt.query_agg(plan2)                                 # ... and other queries run to completion meanwhile
    for h in reversed(launched):
        compare(dt.finalize(h, plan), st, "launched handle finalised late")
    kept = dt.query_agg_keep(plan)
    try:
        first = dt.collect(kept, plan)
        for _ in range(3):
            dt.query_agg(plan2)
        compare(dt.collect(kept, plan), st, "host view after later queries")
        offs, bufs = dt.partition(kept, 2)                  # device-side rows are still there
        assert int(offs[-1]) == first.ngroups and len(bufs) == 3
    finally:
        dt.discard(kept)
    lib, h = capi.load(), C.c_void_p()
    bad = (capi.ColDesc * 2)(capi.ColDesc(capi.DIM_NUMERIC, capi.U32), capi.ColDesc(capi.METRIC_SUM, capi.BITSET32))
    assert lib.vh_table_create(bad, 2, 1000, 1, C.byref(h)) == -1 and b"bad kind" in lib.vh_last_error()
    bad = (capi.ColDesc * 1)(capi.ColDesc(7, capi.U32))
    assert lib.vh_table_create(bad, 1, 1000, 1, C.byref(h)) == -1
    with pytest.raises(capi.VhError, match="out of range"):
        dt.sync_segment(1 << 30, [None] * len(dt.cols), 0)


def test_limits_the_reference_does_not_have(typed):
    """IN lists of hundreds of values (one comparison per value in the reference, filter.cc:223-241), more group columns
    and more metrics than one pass of the kernels carries: answers, not VH_E_UNSUPPORTED."""
    tab, dt = typed
    vals = [str(v) for v in range(-60, 61, 2)] + [str(1000 + v) for v in range(600)]
    for flags in (0, 8, 1):
        res, st = run(tab, dt, {"dimensions": ["s8"], "metrics": ["count", "long_sum"], "filter": {"op": "in", "column": "d_int", "values": vals}}, flags=flags)
        assert 0 < st.passed_recs < st.scanned_recs
        run(tab, dt, {"dimensions": ["flag"], "metrics": ["count"],
                      "filter": {"op": "and", "filters": [{"op": "not", "filter": {"op": "in", "column": "d_uint", "values": vals}}, F("lt", "d_long", "30")]}}, flags=flags)
    run(tab, dt, {"dimensions": ["s8"], "metrics": ["count"], "filter": {"op": "or", "filters": [F("eq", "d_int", str(v)) for v in range(-60, 60)]}})   # 120 operands, 120 literals
    # 11 group columns (49-byte key), then every metric of the table at once: 41 states per group, several passes joined on the key
    dims = ["s8", "s16", "flag", "d_ubyte", "d_short", "d_ushort", "d_int", "d_uint", "d_float", "d_long", "d_double"]
    run(tab, dt, {"dimensions": dims, "metrics": ["count", "int_sum"], "filter": F("lt", "d_uint", "12")})
    allm = ["count"] + [f"{t}_{a}" for t in TYPES for a in ("sum", "min", "max", "avg")]
    for flags in (0, 1):
        res, _ = run(tab, dt, {"dimensions": ["s8", "flag"], "metrics": allm, "filter": F("lt", "d_uint", "30")}, flags=flags)
        assert len(res.states) == 41
    noc = [m for m in allm if m != "count"][:30]          # AVG without COUNT: the hidden count travels with one of the passes
    if tab.has_hidden_count:
        res, _ = run(tab, dt, {"dimensions": ["s8"], "metrics": noc}, flags=0)
