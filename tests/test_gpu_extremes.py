"""HIP paths vs the oracle at the limits of the types (tests/extremes.py): predicates with edge literals (segment skipping at degenerate
stats included), extreme group keys, SUM / MIN / MAX / AVG at the extremes (float sums against the exact-sum bound), and the packed forms
on both sides of every width where one form switches to the next — asserting which form ran, not only the answer."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import extremes as X
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query, storage_index
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
NOW = 1496570140
PRED_FLAGS = [0, capi.PLAN_NO_FAST, capi.PLAN_NO_JIT, capi.PLAN_FORCE_JIT]
PATH_FLAGS = [0, capi.PLAN_FORCE_GLOBAL, capi.PLAN_FORCE_HASH, capi.PLAN_FORCE_PART, capi.PLAN_FORCE_LANES,
              capi.PLAN_NO_JIT, capi.PLAN_FORCE_JIT | capi.PLAN_FORCE_PART]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def edge():
    tab = X.edge_table()
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


def run(tab, dt, q, flags=0, label=""):
    q = dict({"type": "aggregate", "table": tab.name}, **q)
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=NOW)
    res = dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=flags))
    label = f"{label} {q} flags={flags}"
    pos = X.float_sum_positions(aq)
    if pos:
        cache = tab.__dict__.setdefault("_addends", {})              # (kept on the table: it lives exactly as long as the rows it sums)
        if str(q) not in cache:
            cache[str(q)] = X.group_addends(tab, aq, NOW)
        compare(X._without(res, pos), X._without(st, pos), label)
        X.check_float_sums(res.keys, res.states, aq, cache[str(q)], label, pos)
    else:
        compare(res, st, label)
    return res, st


# ------------------------------------------------------------------------------------------------------------------- (a) predicates
@pytest.mark.parametrize("op", X.OPS)
@pytest.mark.parametrize("t", X.FILTERABLE)
def test_edge_literals(edge, t, op):
    """Every edge literal (and the stoul-wrapped "256" / "-1") through the flag sets; scanned_segments matches the oracle's skipping at
    the one-value segments (all minimum, all maximum / all -0.0, all +inf, all +0.0)."""
    tab, dt = edge
    for lits in X.pred_literal_sets(t, op):
        for flags in PRED_FLAGS:
            run(tab, dt, X.pred_query(t, op, lits), flags)


@pytest.mark.parametrize("t", ["float", "double"])
def test_signed_zero_literals_at_one_value_segments(edge, t):
    """Segment 3 holds only +0.0, segment 1 only -0.0: IEEE says -0.0 == +0.0, the order key says -0.0 < +0.0. Skipping must follow IEEE
    (the reference compares the stats as floats), so `le -0.0` / `eq -0.0` / `ge +0.0` scan both and pass every row of both."""
    tab, dt = edge
    for op, lit, segs in (("le", "-0.0", 3), ("eq", "-0.0", 3), ("eq", "0.0", 3), ("lt", "-0.0", 3), ("ge", "0.0", 4), ("gt", "-0.0", 4)):
        for flags in PRED_FLAGS:
            res, st = run(tab, dt, {"dimensions": ["g"], "metrics": ["count"], "filter": X.F(op, "d_" + t, lit)}, flags)
            assert st.scanned_segments == res.scanned_segments == segs, (op, lit, st.scanned_segments)    # (all +inf: skipped, its min is FLT_MAX)
            if op in ("le", "eq"):
                assert res.passed_recs >= 2 * X.SEG_ROWS


def _narrow_table(amax, bmax=255, n=40_000, nseg=2):
    """Unsigned 32-bit filter columns a (recorded max exactly amax, the uint edge values up to it) and b (max bmax), a group column g and
    two metrics: the kind of column vh_table_narrow copies and vh_table_predpack packs."""
    rng = np.random.default_rng(amax)
    e = np.array([v for v in X.int_edges("uint") if v <= amax] + [amax], dtype=np.uint32)
    tab = vo.Table({"name": "w", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "b", "type": "uint"},
                                                                   {"name": "g", "type": "ushort"}],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "v", "type": "long_sum"}]})
    for s in range(nseg):
        a = np.where(np.arange(n) % 3 == 0, e[np.arange(n) % len(e)], rng.integers(0, amax + 1, n)).astype(np.uint32)
        b = rng.integers(0, bmax + 1, n).astype(np.uint32)
        b[0] = bmax
        tab.add_segment_arrays([a, b, (np.arange(n) % 16).astype(np.uint16)],
                               [np.ones(n, dtype=np.uint32), rng.integers(-1000, 1000, n).astype(np.int64)], None, n)
    return tab


def _narrow_query(op, lits):
    f = X.pred_filter("uint", op, lits)
    (f["filter"] if op == "not in" else f)["column"] = "a"
    return {"dimensions": ["g"], "metrics": ["count", "v"], "filter": f}


NARROW_FLAGS = capi.PLAN_NO_JIT | capi.PLAN_NO_LANES | capi.PLAN_NO_PACK      # the pre-built compacting kernels: what reads the copies


@pytest.mark.parametrize("amax", [255, 65535])
def test_edge_literals_on_narrow_copies(amax):
    """Every uint edge literal (2^32 - 1, "-1", 256, 65536, ... beyond the copy's range) against a column held as a 1- or 2-byte copy."""
    tab = _narrow_table(amax)
    dt = mirror_table(tab)
    try:
        dt.narrow([storage_index(tab, tab.dimension("a"))])
        for op in X.OPS:
            for lits in X.pred_literal_sets("uint", op):
                res, _ = run(tab, dt, _narrow_query(op, lits), NARROW_FLAGS)
                assert res.narrow, (op, lits, res.flags)
                run(tab, dt, _narrow_query(op, lits))
    finally:
        dt.close()


# the compiled compacting kernel (the lanes kernel reads the 4-byte arenas); byte planes: not the bit-sliced form built unasked beside them
PREDPACK_FLAGS = {True: capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES, False: capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES | capi.PLAN_NO_SLICED}


@pytest.mark.parametrize("sliced", [True, False])
def test_edge_literals_on_a_predicate_projection(sliced):
    """The same literals against 4-bit fields of a predicate projection, bit-sliced or in byte planes."""
    if JIT_OFF:
        pytest.skip("predicate projections are read by the compiled kernels")
    tab = _narrow_table(15, bmax=15)
    dt = mirror_table(tab)
    try:
        dt.predpack([storage_index(tab, tab.dimension(c)) for c in ("a", "b")], sliced=sliced)
        for op in X.OPS:
            for lits in X.pred_literal_sets("uint", op):
                res, _ = run(tab, dt, _narrow_query(op, lits), PREDPACK_FLAGS[sliced])
                assert res.predpack and res.sliced == sliced, (op, lits, res.flags)
    finally:
        dt.close()


# ------------------------------------------------------------------------------------------------------------------- (b) group keys
@pytest.mark.parametrize("flags", PATH_FLAGS)
@pytest.mark.parametrize("dims", X.KEY_SETS, ids=lambda d: "+".join(d))
def test_extreme_keys(edge, dims, flags):
    tab, dt = edge
    res, st = run(tab, dt, X.key_query(dims), flags)
    if res.path == "hash" and not res.hpart:      # the LDS front table takes one-word keys only (packed by element width, vhh_plan.h)
        assert bool(res.flags & capi.INFO_LDS_HASH) == (X.key_words(tab, dims) == 1), (dims, res.flags)
    if dims in (["d_long"], ["d_ulong"], ["d_float"], ["d_double"]) and not flags & capi.PLAN_FORCE_GLOBAL:
        assert res.path == "hash", (dims, res.path)      # INT64_MIN..INT64_MAX / a u64 range past 2^63: the digit extent overflows


def test_float_key_signed_zero_is_one_group(edge):
    tab, dt = edge
    for flags in (0, capi.PLAN_FORCE_HASH, capi.PLAN_NO_JIT):
        res, _ = run(tab, dt, X.key_query(["d_double"]), flags)
        assert np.sum(res.keys[0] == 0) == 1


# ------------------------------------------------------------------------------------------------------------------- (c) metrics
@pytest.mark.parametrize("flags", PATH_FLAGS + [capi.PLAN_NO_FAST])
@pytest.mark.parametrize("t", X.TYPES)
def test_edge_metrics(edge, t, flags, monkeypatch):
    """Wrapping long / ulong / uint sums, identity-only groups, negative-only floats (MAX: FLT_MIN), subnormal-only groups, infinities;
    float SUM / AVG within the exact-sum bound on every path's float atomics."""
    tab, dt = edge
    monkeypatch.setenv("VH_PART_TABLE_KB", "8")        # phase 2's LDS ranges: 8 KB, so that 4096 groups make many of them
    res, _ = run(tab, dt, X.metric_query(t), flags)                 # 16 groups: one LDS table unless a path is forced
    assert res.path == METRIC_PATHS_SMALL.get(flags & (capi.PLAN_FORCE_GLOBAL | capi.PLAN_FORCE_HASH), "dense_lds"), (flags, res.path)
    res, _ = run(tab, dt, X.metric_query(t, dims=["g", "d_ubyte"], filt=X.F("ne", "d_uint", "7"), aggs=("sum", "min", "max")), flags)
    want = METRIC_PATHS_WIDE.get(flags)        # 4096 groups x four states (the fast kernels' most): beyond one block's LDS table
    assert want is None or res.path == want, (flags, res.path, res.kernel)
    assert res.path in ("dense_global", "dense_part", "hash"), res.path


METRIC_PATHS_SMALL = {capi.PLAN_FORCE_GLOBAL: "dense_global", capi.PLAN_FORCE_HASH: "hash"}
# (DENSE_PART takes a fast scan kernel, and those gather at most four metric columns: hence four states in the wide query)
METRIC_PATHS_WIDE = {capi.PLAN_FORCE_GLOBAL: "dense_global", capi.PLAN_FORCE_HASH: "hash", capi.PLAN_FORCE_PART: "dense_part",
                     capi.PLAN_FORCE_JIT | capi.PLAN_FORCE_PART: "dense_part"}


# ------------------------------------------------------------------------------------------------------------ (d) packed widths
def _pack_table(maxes, elem="uint", n=20_000, nseg=2, neg=False, lows=None):
    """Columns a0..ak (dimensions of type `elem`) whose recorded max is exactly maxes[i] (min 0, or -1 with neg), a selective filter
    column f and a COUNT."""
    rng = np.random.default_rng(len(maxes) * 31 + int(neg))
    dt_ = X.np_type(elem)
    dims = [{"name": f"a{i}", "type": elem} for i in range(len(maxes))] + [{"name": "f", "type": "uint"}, {"name": "n", "type": "byte"}]
    tab = vo.Table({"name": "p", "segment_size": n, "dimensions": dims, "metrics": [{"name": "count", "type": "count"}]})
    for s in range(nseg):
        cols = []
        for i, mx in enumerate(maxes):
            lo = lows[i] if lows else -1 if elem in ("short", "int", "long") else 0
            c = np.array([int(v) for v in rng.integers(0, max(min(mx, 2 ** 62), 0) + 1, n, dtype=np.uint64)], dtype=object)
            c = (c % 7) if s == 0 else c                      # small values in segment 0, the extreme in segment 1
            c[0] = mx if s == 1 else 0
            c[1] = lo
            cols.append(c.astype(dt_))
        cols.append(rng.integers(0, 100, n).astype(np.uint32))
        cols.append(np.full(n, -1 if neg else 1, dtype=np.int8))     # (in the projection with neg: a negative value keeps byte fields)
        tab.add_segment_arrays(cols, [np.ones(n, dtype=np.uint32)], None, n)
    return tab


def _packed_run(tab, maxes, compressed=True, neg=False):
    dt = mirror_table(tab)
    try:
        cols = [storage_index(tab, tab.dimension(f"a{i}")) for i in range(len(maxes))] + [storage_index(tab, tab.metric("count"))]   # (what the query gathers)
        dt.pack(cols + [storage_index(tab, tab.dimension("n"))] if neg else cols, compressed=compressed)
        res, _ = run(tab, dt, {"dimensions": [f"a{i}" for i in range(len(maxes))], "metrics": ["count"], "filter": X.F("lt", "f", "5")},
                     capi.PLAN_FORCE_PACK | capi.PLAN_FORCE_JIT)
        assert res.packed and res.packed_compressed == compressed, (res.packed, res.packed_compressed)
        return res
    finally:
        dt.close()


@pytest.mark.parametrize("maxes,elem,neg,rec", [
    ([255] * 6, "uint", True, 8), ([255] * 5 + [256], "uint", True, 16),                    # + COUNT + the byte -1 (byte fields): 8 vs 9 bytes
    ([65535] * 3, "uint", True, 8), ([65535, 65535, 65536], "uint", True, 16),
    ([2 ** 32 - 1, 255], "ulong", True, 8), ([2 ** 32, 255], "ulong", True, 16),
    ([127] * 7, "int", False, 8), ([127] * 6 + [128], "int", False, 16)])                   # (signed: -1 in every column; + COUNT)
def test_compressed_byte_widths(maxes, elem, neg, rec):
    if JIT_OFF:
        pytest.skip("compressed records are read by the compiled kernels")
    res = _packed_run(_pack_table(maxes, elem, neg=neg), maxes, neg=neg)
    assert not res.pack_bits and res.pack_rec_bytes == rec, (res.pack_bits, res.pack_rec_bytes)


@pytest.mark.parametrize("lows,maxes,elem,rec", [
    ([-128] + [-1] * 6, [127] * 7, "int", 8), ([-129] + [-1] * 6, [127] * 7, "int", 16),      # the negative side of one byte
    ([-1] * 4, [32767] * 3 + [127], "int", 8), ([-1] * 4, [32767, 32767, 32768, 127], "int", 16),          # 2 vs 4 bytes
    ([-1] * 4 + [-32768], [127] * 5, "int", 8), ([-1] * 4 + [-32769], [127] * 5, "int", 16),            # ... from below
    ([-1] * 3, [2 ** 31 - 1, 127, 127], "long", 8), ([-1] * 3, [2 ** 31, 127, 127], "long", 16),         # 4 vs 8 bytes
    ([-(2 ** 31), -1, -1], [127] * 3, "long", 8), ([-(2 ** 31) - 1, -1, -1], [127] * 3, "long", 16)])
def test_compressed_signed_widths(lows, maxes, elem, rec):
    """Signed columns at the width steps from both sides: the recorded min counts as much as the max."""
    if JIT_OFF:
        pytest.skip("compressed records are read by the compiled kernels")
    res = _packed_run(_pack_table(maxes, elem, lows=lows), maxes)
    assert not res.pack_bits and res.pack_rec_bytes == rec, (res.pack_bits, res.pack_rec_bytes)


@pytest.mark.parametrize("maxes,bits,rec", [
    ([255, 255, 255, 127], True, 4), ([255] * 4, False, 8),                                   # + COUNT's bit: 32 bits, a 4-byte record; 33: 8 bytes, no smaller
    ([2 ** 20 - 1, 2 ** 20 - 1, 2 ** 23 - 1], True, 8), ([2 ** 20 - 1, 2 ** 20 - 1, 2 ** 23], False, 16),   # 64 bits in 8 vs bytes in 16; 65: bytes
    ([255] * 7, False, 8)])                                                                  # 57 bits, but the byte record is 8 too: bytes kept
def test_bit_field_records(maxes, bits, rec):
    if JIT_OFF:
        pytest.skip("compressed records are read by the compiled kernels")
    elem = "uint"
    res = _packed_run(_pack_table(maxes, elem), maxes)
    assert res.pack_bits == bits and res.pack_rec_bytes == rec, (res.pack_bits, res.pack_rec_bytes)


def _tuple_table(vbits, gbits=16, nseg=8, n=150_000):
    """G = 2^gbits dense groups, COUNT (1 bit) and a SUM whose recorded max is 2^vbits - 1: gid + values = gbits + 1 + vbits."""
    rng = np.random.default_rng(vbits)
    tab = vo.Table({"name": "u", "segment_size": n, "dimensions": [{"name": "a", "type": "uint"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "v", "type": "ulong_sum"}]})
    for s in range(nseg):
        a = rng.integers(0, 2 ** gbits, n).astype(np.uint32)
        a[:2] = (0, 2 ** gbits - 1)
        v = rng.integers(0, 2 ** vbits, n, dtype=np.uint64)
        v[0] = 2 ** vbits - 1
        tab.add_segment_arrays([a, rng.integers(0, 100, n).astype(np.uint32)], [np.ones(n, dtype=np.uint32), v], None, n)
    return tab


TUPLE_Q = {"dimensions": ["a"], "metrics": ["count", "v"], "filter": X.F("lt", "f", "90")}


@pytest.mark.parametrize("total,one_word,four", [(32, True, True), (33, True, False), (63, True, False), (64, False, False)])
def test_dense_part_tuple_widths(total, one_word, four):
    """gid bits + value bits = 32: four-byte tuples; 33: eight-byte one-word; 63: one-word; 64: two words."""
    if JIT_OFF:
        pytest.skip("packed tuples need the compiled kernels")
    tab = _tuple_table(total - 17)
    dt = mirror_table(tab)
    try:
        res, _ = run(tab, dt, TUPLE_Q, capi.PLAN_FORCE_PART | capi.PLAN_FORCE_JIT)
        assert res.path == "dense_part" and res.retries == 0, (res.path, res.retries)
        assert bool(res.flags & capi.INFO_TUPLE1) == one_word and res.tuple4 == four, (total, res.flags, res.kernel)
    finally:
        dt.close()


@pytest.mark.parametrize("vbits", [20, 21])
def test_hp_packed_tuple_widths(vbits):
    """Hashed partitioning: two 20-bit ids + COUNT (1) + a SUM of `vbits`: pbits + 2 * idbits = 61 packs, 62 does not."""
    if JIT_OFF:
        pytest.skip("the hashed partitioning needs the compiled kernels")
    rng = np.random.default_rng(vbits)
    n = 20_000
    tab = vo.Table({"name": "h", "segment_size": n, "dimensions": [{"name": "c", "type": "ushort"}, {"name": "x", "type": "uint"}],
                    "metrics": [{"name": "users", "type": "bitset", "max": 2 ** 31}, {"name": "count", "type": "count"}, {"name": "v", "type": "uint_sum"}]})
    for s in range(2):
        sets = [set(int(v) for v in rng.integers(2 ** 20 - 3000, 2 ** 20, k)) for k in rng.integers(0, 4, n)]
        v = rng.integers(0, 2 ** vbits, n).astype(np.uint32)
        v[0] = 2 ** vbits - 1
        tab.add_segment_arrays([rng.integers(0, 40, n).astype(np.uint16), rng.integers(0, 100, n).astype(np.uint32)],
                               [sets, np.ones(n, dtype=np.uint32), v], None, n)
    dt = mirror_table(tab)
    try:
        res, _ = run(tab, dt, {"dimensions": ["c", "x"], "metrics": ["users", "count", "v"]},
                     capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HPART | capi.PLAN_FORCE_JIT)
        assert res.path == "hash" and res.hpart and res.retries == 0, (res.path, res.kernel)
        assert res.hp_packed == (1 + vbits + 40 <= 61), (vbits, res.kernel)
    finally:
        dt.close()


# ------------------------------------------------------------------------------------------------------ (e) outgrown widths after a sync
@pytest.mark.parametrize("value,grows", [(2 ** 23 - 1, False), (2 ** 23, True)])
def test_bit_field_records_outgrown_by_a_sync(value, grows):
    """A bit-field projection (20 + 20 + 23 + COUNT's 1 bit, 8-byte records) gets a synced value of exactly 2^23 (one bit past its field:
    rebuilt as byte fields, 16-byte records) or 2^23 - 1 (still fits: kept)."""
    if JIT_OFF:
        pytest.skip("compressed records are read by the compiled kernels")
    maxes = [2 ** 20 - 1, 2 ** 20 - 1, 2 ** 23 - 1]
    tab = _pack_table(maxes, "uint")
    dt = mirror_table(tab)
    q = {"dimensions": ["a0", "a1", "a2"], "metrics": ["count"], "filter": X.F("lt", "f", "5")}
    flags = capi.PLAN_FORCE_PACK | capi.PLAN_FORCE_JIT
    try:
        dt.pack([storage_index(tab, tab.dimension(f"a{i}")) for i in range(3)] + [storage_index(tab, tab.metric("count"))], compressed=True)
        res, _ = run(tab, dt, q, flags)
        assert res.pack_bits and res.pack_rec_bytes == 8
        seg = tab.segments[0]
        f = tab.dimension("f").index
        seg["d"][f][11] = 0                                               # the row passes the filter
        seg["d"][tab.dimension("a2").index][11] = value
        d2 = tab.dimension("a2").index
        seg["dmax"][d2] = max(seg["d"][d2].max(), seg["dmax"][d2])
        dt.sync_batch([(0, 11, 1, seg["size"], list(seg["d"]) + [seg["m"][0]], 0)])
        res, _ = run(tab, dt, q, flags, label="after sync")
        assert res.packed and res.pack_bits != grows and res.pack_rec_bytes == (16 if grows else 8), (res.pack_bits, res.pack_rec_bytes)
    finally:
        dt.close()


def _sync_value(tab, dt, seg_i, col, row, value):
    """One row's value of dimension `col` changed in place through vh_table_sync_batch, the oracle's copy and its stats alike."""
    seg = tab.segments[seg_i]
    d = tab.dimension(col).index
    seg["d"][d][row] = value
    seg["dmax"][d] = max(seg["d"][d].max(), seg["dmax"][d])
    seg["dmin"][d] = min(seg["d"][d].min(), seg["dmin"][d])
    dt.sync_batch([(seg_i, row, 1, seg["size"], list(seg["d"]) + list(seg["m"]), 0)])


@pytest.mark.parametrize("amax,value", [(255, 255), (255, 256), (65535, 65535), (65535, 65536)])
def test_narrow_copies_outgrown_by_a_sync(amax, value):
    """A 1-byte copy (max 255) gets 255 or 256, a 2-byte copy (max 65535) gets 65535 or 65536. What still fits keeps the copy (same
    device bytes); 256 drops the 1-byte copy (a 2-byte one may be built in its place: more device bytes); 65536 drops the copy for good."""
    tab = _narrow_table(amax)
    dt = mirror_table(tab)
    q = _narrow_query("lt", [str(amax // 2)])
    try:
        dt.narrow([storage_index(tab, tab.dimension("a"))])
        res, _ = run(tab, dt, q, NARROW_FLAGS)
        assert res.narrow
        before = dt.info()[2]
        _sync_value(tab, dt, 1, "a", 17, value)
        res, _ = run(tab, dt, q, NARROW_FLAGS, label="after sync")
        after = dt.info()[2]
        for lits in ([str(value)], [str(value - 1)], [str(value + 1)]):
            run(tab, dt, _narrow_query("eq", lits), NARROW_FLAGS, label="after sync")
        if value == amax:
            assert res.narrow and after == before, (res.flags, before, after)
        elif value == 65536:
            assert not res.narrow and after < before, (res.flags, before, after)
        else:
            assert (not res.narrow and after < before) or (res.narrow and after > before), (res.flags, before, after)
    finally:
        dt.close()


@pytest.mark.parametrize("sliced", [True, False])
@pytest.mark.parametrize("value", [15, 16])
def test_predicate_projection_outgrown_by_a_sync(sliced, value):
    """4-bit fields (max 15) get 15 (kept) or 16, one bit past the field: predpack_usable drops the projection; the answers stay the
    oracle's and the query that follows reads the column elsewhere (or from a projection built again, wider: more device bytes)."""
    if JIT_OFF:
        pytest.skip("predicate projections are read by the compiled kernels")
    tab = _narrow_table(15, bmax=15)
    dt = mirror_table(tab)
    q = _narrow_query("lt", ["3"])
    try:
        dt.predpack([storage_index(tab, tab.dimension(c)) for c in ("a", "b")], sliced=sliced)
        res, _ = run(tab, dt, q, PREDPACK_FLAGS[sliced])
        assert res.predpack and res.sliced == sliced
        before = dt.info()[2]
        _sync_value(tab, dt, 0, "a", 5, value)
        res, _ = run(tab, dt, q, PREDPACK_FLAGS[sliced], label="after sync")
        after = dt.info()[2]
        run(tab, dt, _narrow_query("eq", [str(value)]), PREDPACK_FLAGS[sliced], label="after sync")
        if value == 15:
            assert res.predpack and res.sliced == sliced and after == before, (res.flags, before, after)
        else:
            assert not res.predpack or after != before, (res.flags, before, after)
    finally:
        dt.close()


@pytest.mark.parametrize("value,rec", [(255, 8), (256, 16)])
def test_compressed_byte_fields_outgrown_by_a_sync(value, rec):
    """Byte-field records of 8 bytes (six 1-byte columns, COUNT, a negative byte) get 255 (kept) or 256 (a 2-byte field: rebuilt, 16)."""
    if JIT_OFF:
        pytest.skip("compressed records are read by the compiled kernels")
    maxes = [255] * 6
    tab = _pack_table(maxes, "uint", neg=True)
    dt = mirror_table(tab)
    q = {"dimensions": [f"a{i}" for i in range(6)] + ["n"], "metrics": ["count"], "filter": X.F("lt", "f", "5")}   # (n: a projection
    flags = capi.PLAN_FORCE_PACK | capi.PLAN_FORCE_JIT                                                                # built again holds it too)
    try:
        cols = [storage_index(tab, tab.dimension(f"a{i}")) for i in range(6)] + [storage_index(tab, tab.metric("count")),
                                                                                  storage_index(tab, tab.dimension("n"))]
        dt.pack(cols, compressed=True)
        res, _ = run(tab, dt, q, flags)
        assert not res.pack_bits and res.pack_rec_bytes == 8
        tab.segments[0]["d"][tab.dimension("f").index][11] = 0              # the row passes the filter
        _sync_value(tab, dt, 0, "a5", 11, value)
        res, _ = run(tab, dt, q, flags, label="after sync")
        assert res.packed and not res.pack_bits and res.pack_rec_bytes == rec, (res.pack_bits, res.pack_rec_bytes)
    finally:
        dt.close()


# ----------------------------------------------------------------------------------------- (f) one-word tuples that meet a wider value
def test_one_word_tuples_recover_from_a_wide_value(monkeypatch):
    """VH_TEST_TUPLE_BITS=k records k bits too few for the first metric: the kernel meets values wider than their field (VH_ERR_HP_WIDE)
    and the query is planned again without one-word tuples — the oracle's answer, retries >= 1."""
    if JIT_OFF:
        pytest.skip("packed tuples need the compiled kernels")
    tab = _tuple_table(15)
    dt = mirror_table(tab)
    q = dict(TUPLE_Q, metrics=["v", "count"])                     # (the hook narrows the FIRST metric)
    try:
        res, _ = run(tab, dt, q, capi.PLAN_FORCE_PART | capi.PLAN_FORCE_JIT)
        assert res.tuple4 and res.retries == 0
        for k in ("1", "3"):
            monkeypatch.setenv("VH_TEST_TUPLE_BITS", k)
            res, _ = run(tab, dt, q, capi.PLAN_FORCE_PART | capi.PLAN_FORCE_JIT, label="tuple bits -" + k)
            monkeypatch.delenv("VH_TEST_TUPLE_BITS")
            assert res.retries >= 1 and not res.flags & capi.INFO_TUPLE1 and not res.tuple4, (res.retries, res.flags)
    finally:
        dt.close()
