"""The three kernels that regroup a partial result by owner for the multi-GPU exchange — partition_groups_kernel, partition_pairs_kernel
and hp_partition_pairs_kernel (csrc/vh_small_kernels.h) — through vh_result_partition and vh_result_partition_pairs on one finalised
result, for every nparts the sharded protocol can ask for. No communicator is involved.

The reference owner is include/viya_hip.h's `mix(key columns) % world`, restated here: h = 0x9E3779B97F4A7C15; per key column
h = splitmix64(h ^ v), v the EMITTED key value zero-extended from the column's width; owner = h % nparts. The group kernel reads the
emitted columns, the pair kernels rebuild the key from a dense group id, a hash table's key words or a tuple's mixed key: a group's pairs
must land with the group's states whatever the key's sign, width, word count — or when the key is the hash table's empty marker.

Checked for every case and nparts: the offsets' shape, element types and merge ops; the partitioned rows are a permutation of the rows
the host view holds (all columns of a row together, as bytes); every row sits in its reference owner's slice; the (key, id) pairs are the
oracle's set (without duplicates and as many as the cardinalities add up to, unless the hashed partitioning delivered them), each in the
slice of its key's reference owner."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import extremes as X
from tests.planner import mirror_table, plan_from_query
from viyadb_amd import capi
from viyadb_amd.executor import device_read

pytestmark = pytest.mark.gpu
NOW = 1496570140
NPARTS = (1, 2, 3, 4, 7, 8, 63, 64)
HASH = capi.PLAN_FORCE_HASH
RECORDS = capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HASH_RECORDS
HP = capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HPART | capi.PLAN_FORCE_JIT
GLOBAL, PART = capi.PLAN_FORCE_GLOBAL, capi.PLAN_FORCE_PART
MERGE_OP = {"sum": 0, "avg": 0, "count": 0, "min": 1, "max": 2, "bitset": -2}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def F(op, col, val):
    return {"op": op, "column": col, "value": str(val)}


# ------------------------------------------------------------------------------------------------------------ the reference owner
def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def bits(a):
    """A key column as the kernels see it: its bytes, zero-extended to 64 bits."""
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize).astype(np.uint64)


def ref_owner(key_bits, nparts):
    n = len(key_bits[0])
    h = np.full(n, 0x9E3779B97F4A7C15, dtype=np.uint64)
    for v in key_bits:
        h = splitmix64(h ^ v)
    return (h % np.uint64(nparts)).astype(np.int64)


def test_reference_owner_against_python_integers():
    """The numpy restatement against plain Python integers, on one- and three-column keys of every width."""
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    cols = [np.array([-1, -128, 0, 127], dtype=np.int8), np.array([-1, 2 ** 31 - 1, -2 ** 31, 7], dtype=np.int32),
            np.array([2 ** 64 - 1, 2 ** 63, 0, 5], dtype=np.uint64)]
    for keys in ([cols[0]], [cols[2]], cols):
        for nparts in (3, 8, 63):
            want = []
            for i in range(4):
                h = 0x9E3779B97F4A7C15
                for c in keys:
                    h = mix(h ^ (int(c[i]) & ((1 << (8 * c.dtype.itemsize)) - 1)))
                want.append(h % nparts)
            assert ref_owner([bits(c) for c in keys], nparts).tolist() == want


# ------------------------------------------------------------------------------------------------------------ the checks
def row_bytes(cols):
    """The rows of a set of columns as sorted byte strings: all columns of a row together."""
    n = len(cols[0])
    raw = np.concatenate([np.ascontiguousarray(c).view(np.uint8).reshape(n, c.dtype.itemsize) for c in cols], axis=1) if n else np.zeros((0, 1), np.uint8)
    flat = np.ascontiguousarray(raw).view(np.dtype((np.void, raw.shape[1]))).ravel()
    return np.sort(flat)


def read_partition(offs, bufs, nparts, count, dtypes, ops, what):
    assert len(offs) == nparts + 1 and int(offs[0]) == 0 and int(offs[nparts]) == count, (what, nparts, offs, count)
    assert (np.diff(offs.astype(np.int64)) >= 0).all(), (what, nparts, offs)
    assert len(bufs) == len(dtypes), (what, len(bufs), len(dtypes))
    cols = []
    for (ptr, n, elem, op), dt, want_op in zip(bufs, dtypes, ops):
        assert n == count and np.dtype(capi.ELEM_NP[elem]) == dt and op == want_op, (what, nparts, n, count, elem, dt, op, want_op)
        cols.append(device_read(ptr, n, dt))
    return cols


def slice_of(offs, nparts):
    return np.repeat(np.arange(nparts, dtype=np.int64), np.diff(offs.astype(np.int64)))


def pair_rows(key_cols, ids):
    return np.stack([bits(k) for k in key_cols] + [ids.astype(np.uint64)], axis=1) if len(ids) else np.zeros((0, len(key_cols) + 1), np.uint64)


def oracle_pairs(st, res, j):
    """(key bits ..., id) of every passing row's ids under its group key — the oracle's sets of metric j, one row per member."""
    sizes = np.array([len(s) for s in st.bitsets[j]], dtype=np.int64)
    keys = [np.repeat(k.astype(r.dtype), sizes) for k, r in zip(st.keys, res.keys)]
    ids = np.array([i for s in st.bitsets[j] for i in sorted(s)], dtype=np.uint64)
    return pair_rows(keys, ids)


def check_result(tab, dt, q, flags, path=None, hpart=None, nparts_list=NPARTS, label=""):
    """One query, kept; vh_result_partition and vh_result_partition_pairs for every nparts. -> (AggResult, {nparts: (group key bits ->
    slice, pair key bits -> slice)}) for the cases that compare owners between tables."""
    q = dict({"type": "aggregate", "table": tab.name}, **q)
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq, now=NOW)
    plan = plan_from_query(tab, aq, now=NOW, flags=flags)
    kept = dt.query_agg_keep(plan)
    owners = {}
    try:
        res = dt.collect(kept, plan)
        what = "%s flags=%d path=%s hpart=%s" % (label or q.get("dimensions") or q.get("select"), flags, res.path, res.hpart)
        print("PARTITION CASE", what, "groups", res.ngroups)
        if path is not None:
            assert res.path == path or (path == "dense" and res.path.startswith("dense")), what
        if hpart is not None:
            assert res.hpart == hpart, what
        assert res.ngroups == st.ngroups == res.returned, (what, res.ngroups, st.ngroups)
        nk = len(res.keys)
        host_cols = res.keys + res.states + ([res.hidden_count] if res.hidden_count is not None else [])
        assert (res.hidden_count is not None) == (st.hidden_count is not None), what
        ops = [-1] * nk + [MERGE_OP[oc.col.agg] for oc in aq.metric_cols] + ([0] if res.hidden_count is not None else [])
        want_rows = row_bytes(host_cols)
        bitset_js = [j for j, oc in enumerate(aq.metric_cols) if oc.col.agg == "bitset"]
        for nparts in nparts_list:
            offs, bufs = dt.partition(kept, nparts)
            cols = read_partition(offs, bufs, nparts, res.ngroups, [c.dtype for c in host_cols], ops, what)
            got_rows = row_bytes(cols)
            assert got_rows.tobytes() == want_rows.tobytes(), (what, nparts, "the partitioned rows are no permutation of the result's rows")
            where = slice_of(offs, nparts)
            kb = [bits(c) for c in cols[:nk]]
            bad = np.nonzero(ref_owner(kb, nparts) != where)[0] if res.ngroups else []
            assert len(bad) == 0, (what, nparts, "%d groups outside their owner's slice, first: keys %r in slice %d" % (
                len(bad), [c[bad[0]] for c in cols[:nk]], where[bad[0]]))
            gmap = {tuple(int(k[i]) for k in kb): int(where[i]) for i in range(res.ngroups)}
            pmap = {}
            for j in bitset_js:
                poffs, pbufs = dt.partition_pairs(kept, j, nparts)
                id_dt = np.dtype(capi.ELEM_NP[pbufs[-1][2]])
                assert id_dt in (np.dtype(np.uint32), np.dtype(np.uint64)), what
                pcols = read_partition(poffs, pbufs, nparts, int(poffs[nparts]), [k.dtype for k in res.keys] + [id_dt], [-1] * (nk + 1), what + " pairs")
                got = pair_rows(pcols[:nk], pcols[nk])
                want = oracle_pairs(st, res, j)
                uniq = np.unique(got, axis=0)
                assert uniq.shape == want.shape and np.array_equal(uniq, np.unique(want, axis=0)), (
                    what, nparts, "pairs differ from the oracle's sets: %d distinct delivered, %d wanted" % (len(uniq), len(want)))
                if not res.hpart:                      # the device-wide set holds every pair once; the tuple pool may repeat them
                    assert len(got) == len(uniq) == int(res.states[j].astype(np.uint64).sum()), (what, nparts, len(got), len(uniq))
                pwhere = slice_of(poffs, nparts)
                pkb = [got[:, c] for c in range(nk)]
                pbad = np.nonzero(ref_owner(pkb, nparts) != pwhere)[0] if len(got) else []
                assert len(pbad) == 0, (what, nparts, "%d pairs outside their key's owner's slice, first: %r in slice %d" % (
                    len(pbad), got[pbad[0]].tolist() if len(pbad) else None, pwhere[pbad[0]] if len(pbad) else -1))
                for i in range(len(got)):               # ... which is the slice its group's states went to
                    assert gmap[tuple(int(x) for x in got[i, :nk])] == int(pwhere[i]), (what, nparts, got[i].tolist())
                pmap.update({tuple(int(x) for x in got[i, :nk]): int(pwhere[i]) for i in range(len(got))})
            owners[nparts] = (gmap, pmap)
        return res, owners
    finally:
        dt.discard(kept)


# ------------------------------------------------------------------------------------------------------------ key types
@pytest.fixture(scope="module")
def E():
    tab = X.edge_table(nseg=3)
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


KEY_FAMILIES = [["d_byte", "d_short"],                  # negatives at 1 and 2 bytes
                ["d_int", "d_long"],                    # the extremes of both; 96 bits: two key words
                ["d_ubyte", "d_ushort", "d_uint"],
                ["d_ulong"],                            # from 2^63 up, and 2^64 - 1: the empty marker as a key
                ["d_long"],                             # -1: the empty marker again
                ["d_float", "d_double"],
                ["d_ulong", "d_byte"]]                  # 72 bits: the smallest two-word key


@pytest.mark.parametrize("flags", [0, HASH, RECORDS])
@pytest.mark.parametrize("dims", KEY_FAMILIES, ids=lambda d: "+".join(d))
def test_key_types(E, dims, flags):
    tab, dt = E
    res, _ = check_result(tab, dt, X.key_query(dims), flags, path="hash" if flags else None)
    if dims == ["d_ulong"]:
        assert (res.keys[0] == np.uint64(2 ** 64 - 1)).any() and (res.keys[0] >= np.uint64(2 ** 63)).sum() >= 3
    if dims == ["d_long"]:
        assert (res.keys[0] == -1).any() and (res.keys[0] == np.iinfo(np.int64).min).any()
    if dims == ["d_byte", "d_short"]:
        assert (res.keys[0] < 0).any() and (res.keys[1] < 0).any()


@pytest.fixture(scope="module")
def S():
    """A string, a boolean and a time dimension."""
    rng = np.random.default_rng(31)
    tab = vo.Table({"name": "s", "segment_size": 6000,
                    "dimensions": [{"name": "s", "cardinality": 200}, {"name": "flag", "type": "boolean"}, {"name": "ts", "type": "time"},
                                   {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "v", "type": "long_sum"}]})
    dic = tab.dicts["s"]
    for i in range(150):
        dic.v2c["v%d" % i] = len(dic.c2v)
        dic.c2v.append("v%d" % i)
    for n in (6000, 3111):
        tab.add_segment_arrays([rng.integers(0, 151, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8),
                                rng.integers(NOW - 30 * 86400, NOW, n).astype(np.uint32), rng.integers(0, 100, n).astype(np.uint32)],
                               [rng.integers(1, 4, n).astype(np.uint32), rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)], None, n)
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


@pytest.mark.parametrize("flags", [0, HASH, RECORDS])
def test_string_boolean_and_day_keys(S, flags):
    tab, dt = S
    q = {"select": [{"column": "ts", "granularity": "day"}, {"column": "s"}, {"column": "flag"}, {"column": "count"}, {"column": "v"}],
         "filter": F("lt", "f", 90)}
    res, _ = check_result(tab, dt, q, flags, path="hash" if flags else None, label="day+string+boolean")
    assert res.ngroups > 4096 and (res.keys[0] % 86400 == 0).all()


# ------------------------------------------------------------------------------------------------------------ metrics and organisations
METRICS = ["count", "ls", "us", "fs", "ds", "bmin", "hmax", "imin", "umax", "lmax"]


@pytest.fixture(scope="module")
def M():
    """Every state width at once; (a) is 40 group ids, (a, b) 16 000 — several LDS-sized ranges of the partitioned dense organisation."""
    rng = np.random.default_rng(32)
    tab = vo.Table({"name": "m", "segment_size": 8192,
                    "dimensions": [{"name": "a", "type": "ushort"}, {"name": "b", "type": "uint"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "ls", "type": "long_sum"}, {"name": "us", "type": "uint_sum"},
                                {"name": "fs", "type": "float_sum"}, {"name": "ds", "type": "double_sum"}, {"name": "bmin", "type": "byte_min"},
                                {"name": "hmax", "type": "ushort_max"}, {"name": "imin", "type": "int_min"}, {"name": "umax", "type": "uint_max"},
                                {"name": "lmax", "type": "ulong_max"}]})
    for n in (8192, 5001, 7777):
        tab.add_segment_arrays(
            [rng.integers(0, 40, n).astype(np.uint16), rng.integers(0, 400, n).astype(np.uint32), rng.integers(0, 100, n).astype(np.uint32)],
            [rng.integers(1, 4, n).astype(np.uint32), rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64), rng.integers(0, 1000, n).astype(np.uint32),
             (rng.integers(-2000, 2000, n) / 8.0).astype(np.float32), rng.integers(-2000, 2000, n) / 8.0, rng.integers(-128, 128, n).astype(np.int8),
             rng.integers(0, 2 ** 16, n).astype(np.uint16), rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
             rng.integers(0, 2 ** 32, n).astype(np.uint32), rng.integers(0, 2 ** 64, n, dtype=np.uint64)], None, n)
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


def _needs_jit(flags):
    from tests.conftest import JIT_OFF
    if flags == HP and JIT_OFF:
        pytest.skip("VH_JIT=off: the hashed partitioning needs the scan kernel compiled for the plan")


@pytest.mark.parametrize("dims,metrics,flags,path,hpart", [
    (["a"], METRICS, 0, "dense_lds", False), (["a", "b"], METRICS, GLOBAL, "dense_global", False),
    (["a", "b"], ["count", "ls", "fs", "lmax"], PART, "dense_part", False), (["a", "b"], ["ds", "bmin", "hmax", "umax"], PART, "dense_part", False),
    (["a", "b"], METRICS, HASH, "hash", False), (["a", "b"], METRICS, RECORDS, "hash", False), (["a", "b"], ["count", "us"], HP, "hash", True)],
    ids=["dense_lds", "dense_global", "dense_part", "dense_part_others", "hash", "records", "hpart"])
def test_every_state_width_on_every_organisation(M, dims, metrics, flags, path, hpart):
    """All ten states at once where the organisation takes them; the partitioned dense one holds at most four (VH_FAST_COLS), so it gets the
    ten in two plans, and the hashed partitioning 64 bits of them."""
    _needs_jit(flags)
    tab, dt = M
    check_result(tab, dt, {"dimensions": dims, "metrics": metrics, "filter": F("lt", "f", 70)}, flags, path=path, hpart=hpart)


@pytest.mark.parametrize("flags", [0, HASH, RECORDS])
def test_avg_travels_with_its_hidden_count(flags):
    rng = np.random.default_rng(33)
    tab = vo.Table({"name": "h", "segment_size": 6000, "dimensions": [{"name": "k", "type": "ushort"}],
                    "metrics": [{"name": "a", "type": "double_avg"}, {"name": "v", "type": "long_sum"}]})
    for n in (6000, 4500):
        tab.add_segment_arrays([rng.integers(0, 5000, n).astype(np.uint16)], [rng.integers(-2000, 2000, n) / 8.0, rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64)],
                               rng.integers(1, 5, n).astype(np.uint64), n)
    dt = mirror_table(tab)
    try:
        res, _ = check_result(tab, dt, {"dimensions": ["k"], "metrics": ["a", "v"]}, flags, path="hash" if flags else None)
        assert res.hidden_count is not None and res.ngroups > 4096
    finally:
        dt.close()


# ------------------------------------------------------------------------------------------------------------ count-distinct pairs
def pairs_table(wide):
    """Keys with negatives at two widths, exactly one key word together (16 + 32 + 16 bits); kl holds the empty marker. Ids of 32 bits, or
    up to 2^40 (the VH_U64 id column)."""
    rng = np.random.default_rng(34 + wide)
    tab = vo.Table({"name": "p", "segment_size": 6000,
                    "dimensions": [{"name": "ks", "type": "short"}, {"name": "ki", "type": "int"}, {"name": "ku", "type": "ushort"},
                                   {"name": "kl", "type": "ulong"}, {"name": "f", "type": "uint"}],
                    "metrics": [{"name": "users", "type": "bitset", "max": 2 ** 40 if wide else 2 ** 31}, {"name": "count", "type": "count"}]})
    top = 2 ** 40 if wide else 2 ** 31
    for n in (6000, 4097):
        sets = [set(int(v) for v in np.where(rng.random(k) < 0.5, rng.integers(top - 3000, top, k), rng.integers(0, 3000, k))) for k in rng.integers(0, 4, n)]
        tab.add_segment_arrays([rng.integers(-20, 20, n).astype(np.int16), rng.integers(-5, 5, n).astype(np.int32), rng.integers(0, 4, n).astype(np.uint16),
                                np.array([2 ** 64 - 1, 2 ** 63, 5], dtype=np.uint64)[rng.integers(0, 3, n)], rng.integers(0, 100, n).astype(np.uint32)],
                               [sets, np.ones(n, dtype=np.uint32)], None, n)
    return tab


@pytest.fixture(scope="module", params=[False, True], ids=["ids32", "ids40"])
def P(request):
    tab = pairs_table(request.param)
    dt = mirror_table(tab)
    yield tab, dt, request.param
    dt.close()


@pytest.mark.parametrize("dims,flags,path", [(["ks"], 0, "dense_global"), (["ks", "ki", "ku"], 0, "dense_global"), (["ks", "ki", "ku"], HASH, "hash"),
                                             (["ks", "ki", "ku"], RECORDS, "hash"), (["ks", "ki", "ku"], HP, "hash")],
                         ids=["dense_40_ids", "dense_global", "hash", "records", "hpart"])
def test_pairs_of_negative_keys_on_every_organisation(P, dims, flags, path):
    """Every organisation that takes a count-distinct metric: the dense table in LDS and the partitioned dense one do not, so 40 group ids
    and 1 640 alike are a dense table in global memory. The hashed partitioning carries 32-bit
    ids only: with ids up to 2^40 the planner answers from the plain hash table."""
    _needs_jit(flags)
    tab, dt, wide = P
    res, _ = check_result(tab, dt, {"dimensions": dims, "metrics": ["users", "count"], "filter": F("lt", "f", 80)}, flags,
                          path=path, hpart=(flags == HP and not wide))
    assert all((k < 0).any() for k in res.keys[:2]) and int(res.states[0].max()) > 3
    assert res.ngroups == 40 if len(dims) == 1 else res.ngroups > 1000


@pytest.mark.parametrize("flags", [HASH, RECORDS])
def test_the_sentinel_group_has_pairs(P, flags):
    """kl = 2^64 - 1 is the hash table's empty marker: its group lives in the reserved slot, and its pairs must still find its owner."""
    tab, dt, wide = P
    res, _ = check_result(tab, dt, {"dimensions": ["kl"], "metrics": ["users", "count"], "filter": F("lt", "f", 80)}, flags, path="hash")
    at = np.nonzero(res.keys[0] == np.uint64(2 ** 64 - 1))[0]
    assert res.ngroups == 3 and len(at) == 1 and int(res.states[0][at[0]]) > 100


# ------------------------------------------------------------------------------------------------------------ block edges
EDGE_N = (1, 255, 4095, 4096, 4097, 8193)               # a block of the partition kernels covers 16 x 256 = 4096 rows


@pytest.fixture(scope="module")
def B():
    """For every N a uint column with exactly N distinct values: s<N> sparse ones, d<N> 0 .. N - 1."""
    rng = np.random.default_rng(35)
    dims = [{"name": "%s%d" % (p, n), "type": "uint"} for n in EDGE_N for p in "sd"] + [{"name": "f", "type": "uint"}]
    tab = vo.Table({"name": "b", "segment_size": 4096, "dimensions": dims,
                    "metrics": [{"name": "count", "type": "count"}, {"name": "v", "type": "long_sum"}]})
    for s in range(3):
        row = np.arange(s * 4096, (s + 1) * 4096, dtype=np.uint64)
        cols = []
        for n in EDGE_N:
            cols += [((row % n) * np.uint64(2654435761) % np.uint64(2 ** 32)).astype(np.uint32), (row % n).astype(np.uint32)]
        cols.append(rng.integers(0, 100, 4096).astype(np.uint32))
        tab.add_segment_arrays(cols, [np.ones(4096, dtype=np.uint32), rng.integers(-10 ** 9, 10 ** 9, 4096).astype(np.int64)], None, 4096)
    dt = mirror_table(tab)
    yield tab, dt
    dt.close()


@pytest.mark.parametrize("n", EDGE_N)
def test_block_edges(B, n):
    tab, dt = B
    res, _ = check_result(tab, dt, {"dimensions": ["s%d" % n], "metrics": ["count", "v"]}, HASH, path="hash")
    assert res.ngroups == n
    res, _ = check_result(tab, dt, {"dimensions": ["d%d" % n], "metrics": ["count", "v"]}, 0, path="dense")
    assert res.ngroups == n


@pytest.mark.parametrize("flags", [0, HASH])
def test_a_filter_that_passes_nothing(B, flags):
    tab, dt = B
    for nparts in NPARTS:
        res, owners = check_result(tab, dt, {"dimensions": ["d4097"], "metrics": ["count", "v"], "filter": F("gt", "f", 1000)}, flags, nparts_list=(nparts,))
        assert res.ngroups == 0 and owners[nparts] == ({}, {})


# ------------------------------------------------------------------------------------------------------------ one owner function for all
def test_one_owner_function_whatever_the_table_records():
    """The same 300 key tuples in two tables whose other rows give the key columns different recorded ranges — a different `glo` and
    extent for the dense pair kernel, key words for the hash one: the owner of every common key is the same in both, for groups and pairs."""
    rng = np.random.default_rng(36)
    common = [(s, i) for s in range(-15, 15) for i in range(-5, 5)]
    assert len(common) == 300

    def table(far):
        tab = vo.Table({"name": "o", "segment_size": 4000, "dimensions": [{"name": "ks", "type": "short"}, {"name": "ki", "type": "int"}],
                        "metrics": [{"name": "users", "type": "bitset", "max": 2 ** 31}, {"name": "count", "type": "count"}]})
        for n in (4000, 2500):
            pick = np.array(common)[rng.integers(0, 300, n)]
            ks, ki = pick[:, 0].astype(np.int16), pick[:, 1].astype(np.int32)
            if far:                                     # other rows, far out: the recorded ranges (and with them glo, extents, the organisation) differ
                out = rng.random(n) < 0.2
                ks = np.where(out, rng.choice(np.array([-32768, 32767, 30000], dtype=np.int16), n), ks).astype(np.int16)
                ki = np.where(out, rng.choice(np.array([-2 ** 31, 2 ** 31 - 1, 10 ** 9], dtype=np.int64), n), ki).astype(np.int32)
            ks[:300], ki[:300] = np.array(common)[:, 0], np.array(common)[:, 1]      # every common tuple is there
            sets = [set(int(v) for v in rng.integers(0, 500, 1 + k)) for k in rng.integers(0, 3, n)]
            tab.add_segment_arrays([ks, ki], [sets, np.ones(n, dtype=np.uint32)], None, n)
        return tab
    near, far = table(False), table(True)
    assert near.segments[0]["dmin"][0] != far.segments[0]["dmin"][0] and near.segments[0]["dmax"][1] != far.segments[0]["dmax"][1]
    q = {"dimensions": ["ks", "ki"], "metrics": ["users", "count"]}
    got = []
    for tab, flags, path in ((near, 0, "dense"), (far, HASH, "hash")):
        dt = mirror_table(tab)
        try:
            got.append(check_result(tab, dt, q, flags, path=path, nparts_list=(3, 8))[1])
        finally:
            dt.close()
    keys = [(int(np.int16(s).view(np.uint16)), int(np.int32(i).view(np.uint32))) for s, i in common]
    for nparts in (3, 8):
        (g0, p0), (g1, p1) = got[0][nparts], got[1][nparts]
        for k in keys:
            assert g0[k] == g1[k] == p0[k] == p1[k], (nparts, k, g0[k], g1[k], p0[k], p1[k])
        assert len(set(g0[k] for k in keys)) == nparts


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(M):
    tab, dt = M
    aq = vo.parse_query(tab, {"type": "aggregate", "table": "m", "dimensions": ["a", "b"], "metrics": ["count", "us"], "filter": F("lt", "f", 70)})

    def code(plan, call):
        kept = dt.query_agg_keep(plan)
        try:
            with pytest.raises(capi.VhError) as e:
                call(kept)
            return e.value.code
        finally:
            dt.discard(kept)
    plain = plan_from_query(tab, aq, now=NOW, flags=HASH)
    assert code(plain, lambda h: dt.partition(h, 0)) == -1                    # VH_E_INVALID
    assert code(plain, lambda h: dt.partition(h, 65)) == -1
    assert code(plain, lambda h: dt.partition_pairs(h, 0, 0)) == -1
    assert code(plain, lambda h: dt.partition_pairs(h, 0, 65)) == -1
    assert code(plain, lambda h: dt.partition_pairs(h, 0, 3)) == -1           # `count` is no bitset metric
    assert code(plain, lambda h: dt.partition_pairs(h, 2, 3)) == -1           # and there is no third metric
    having = plan_from_query(tab, aq, now=NOW, flags=HASH)
    having.having = [("rel", 2, capi.OP_GT, 1)]
    assert code(having, lambda h: dt.partition(h, 3)) == -4                   # VH_E_UNSUPPORTED: HAVING applies to merged groups
    top = plan_from_query(tab, aq, now=NOW, flags=HASH)
    top.top = (2, True, 5)
    assert code(top, lambda h: dt.partition(h, 3)) == -4                      # ... and so does top-N
