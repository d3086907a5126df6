"""Device time truncation and rollup at calendar and width edges (tests/time_edges.py): every unit on every path that carries a time
key, two time keys at once, rows sitting exactly on rollup boundaries, boundaries handed straight to the C ABI, ragged snapshots, packed
record forms through a sync, an 8-byte non-micro time column, and the host shim. Every result is the oracle's bit for bit
(tests.parity.compare); where the oracle's schema cannot say the case, the expected groups come from time_edges.truth and numpy.

Each case prints the path it took (pytest -s shows it): `path kernel fast jit hpart lanes packed`.

Flag sets. Section a runs the eight sets the issue lists and four more: with no filter and one key word, NO_JIT and FORCE_JIT alone both end in
the pre-built no-compaction kernel, so PREBUILT and JIT add VH_PLAN_NO_LANES to pin the compacting pre-built and the compiled kernel, PACK_NL
does the same for the projection, and LANES asks for the no-compaction kernel outright. Eight of the twelve run pre-built kernels.

Compile budget. Granularity, rule units, element type and the hashed-partitioning form are compile-time constants of the compiled scan;
boundaries, snapshots and projections' contents are not. Distinct code objects the file compiles, counted from a run: a 22 (7 granularities x 2
column kinds — FORCE_JIT, JIT and a refused HPART share one — plus 2 x 2 x 2 hashed-partitioning forms), b 2, c 32 (2 rule sets x 2 kinds x 4
queries, each as a scan and as a hashed-partitioning scan), d 4, e 0 (a's), f 5, g 6: 67 after sharing. The whole file takes ~30 s on an MI355X."""
import dataclasses

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import time_edges as te
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.planner import mirror_table, plan_from_query
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, DeviceTable, GroupSpec

pytestmark = pytest.mark.gpu
NOW = te.NOW
GRANS = te.UNITS + [None]
INTERP = capi.PLAN_NO_FAST | capi.PLAN_NO_JIT
NO_JIT = capi.PLAN_NO_JIT
PREBUILT = capi.PLAN_NO_JIT | capi.PLAN_NO_LANES      # the pre-built compacting hash kernel; NO_JIT alone may take the pre-built lanes kernel
FORCE_JIT = capi.PLAN_FORCE_JIT
JIT = capi.PLAN_FORCE_JIT | capi.PLAN_NO_LANES        # the compiled kernel; FORCE_JIT alone gives way to the pre-built lanes kernel where that one is eligible
HPART = capi.PLAN_FORCE_JIT | capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HPART
RECORDS = capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HASH_RECORDS
PART = capi.PLAN_FORCE_PART
PACK = capi.PLAN_FORCE_PACK
PACK_NL = capi.PLAN_FORCE_PACK | capi.PLAN_NO_LANES
LANES = capi.PLAN_FORCE_LANES
FLAG_SETS = [0, INTERP, NO_JIT, PREBUILT, FORCE_JIT, JIT, HPART, RECORDS, PART, PACK, PACK_NL, LANES]
UNIT = {"year": capi.T_YEAR, "month": capi.T_MONTH, "day": capi.T_DAY, "hour": capi.T_HOUR, "minute": capi.T_MINUTE, "second": capi.T_SECOND,
        None: capi.T_NONE}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


class Mirrors:
    """One device mirror per table, made on first use and kept for the module."""

    def __init__(self):
        self.held = {}

    def get(self, name, make):
        if name not in self.held:
            tab = make()
            self.held[name] = (tab, mirror_table(tab))
        return self.held[name]

    def close(self):
        for _, dt in self.held.values():
            dt.close()


@pytest.fixture(scope="module")
def mirrors():
    m = Mirrors()
    yield m
    m.close()


def edge(mirrors, kind):
    return mirrors.get("edge_" + kind, lambda: te.edge_table(kind))


def boundary(mirrors, kind, name):
    return mirrors.get(f"boundary_{kind}_{name}", lambda: te.boundary_table(kind, te.RULE_SETS[name]))


def note(label, flags, res):
    print(f"[time-edges] {label} flags={flags:#x}: {res.path} {res.kernel} fast={res.fast} jit={res.jit} hpart={res.hpart} lanes={res.lanes} "
          f"packed={res.packed} bits={res.pack_bits} rec={res.pack_rec_bytes} groups={res.ngroups}")


def select(gran, dims=("k",), metrics=("count", "long_sum"), col="ts"):
    first = {"column": col, "granularity": gran} if gran else {"column": col}
    return {"select": [first] + [{"column": c} for c in dims] + [{"column": m} for m in metrics]}


def run(tab, dt, q, flags=0, st=None, seg_rows=None, label=""):
    """-> (device result, oracle state); the oracle's state is computed once per query and shared between the flag sets."""
    q = dict({"type": "aggregate", "table": "t"}, **q)
    aq = vo.parse_query(tab, q)
    if st is None:
        st = vo.scan_aggregate(aq, now=NOW, seg_rows=seg_rows)
    res = dt.query_agg(plan_from_query(tab, aq, now=NOW, flags=flags, seg_rows=seg_rows))
    note(label or str(q.get("select") or q.get("dimensions")), flags, res)
    compare(res, st, f"{label} {q} flags={flags:#x}")
    return res, st


def key_words(tab, cols):
    """64-bit words the hash path packs these key columns into: by element width, in query order, a column never straddling two words."""
    words, used = 1, 0
    for c in cols:
        bits = tab.dimension(c).num_type.size * 8
        if used + bits > 64:
            words, used = words + 1, 0
        used += bits
    return words


def front_table_slots(state_bytes):
    """Slots of the LDS front table of a one-word hash key (vhh_plan.h, choose_organisation): 2048, halved while slots x (8 key bytes + the
    states) exceed 24 KB. The host keeps using it — and with it the no-compaction kernel — while the groups it has seen for the plan's shape
    are at most four times the slots."""
    slots = 2048
    while slots > 256 and slots * (8 + state_bytes) > 24 * 1024:
        slots //= 2
    return slots


LANES_K, FAST_K, INTERP_K, JIT_K = "scan_agg_lanes_kernel<", "scan_agg_fast_kernel<", "scan_agg_kernel<", "viya_jit_scan_"


def check_path(res, flags, timey, one_word, state_bytes, ngroups):
    """Which kernel carried the time key, by the scan kernel's name. Every query here is unfiltered (every row passes) and lands in the hash
    organisation: a truncated time key has no dense group-id space, so VH_PLAN_FORCE_PART is answered from the hash table (asserted).
      VH_PLAN_NO_FAST                      the interpreting scan, scan_agg_kernel
      one key word, few groups             the pre-built no-compaction kernel over the LDS front table, scan_agg_lanes_kernel — unless
                                           VH_PLAN_NO_LANES forbids it or hashed partitioning runs. VH_PLAN_FORCE_JIT gives way to it too (there
                                           is no compiled form of it: the refusal is asserted), and so does VH_PLAN_FORCE_HASH_RECORDS
      VH_PLAN_FORCE_JIT otherwise          the compiled scan, viya_jit_scan_<hash>
      everything else                      the pre-built compacting kernel, scan_agg_fast_kernel
    Hashed partitioning (VH_PLAN_FORCE_HPART) takes one key word and at most 64 bits of states; the planner refuses it otherwise (asserted)."""
    k = res.kernel
    jit_asked = bool(flags & capi.PLAN_FORCE_JIT) and not JIT_OFF
    hpart = flags == HPART and jit_asked and one_word and state_bytes <= 8
    lanes_can = one_word and not hpart and not flags & (capi.PLAN_NO_LANES | capi.PLAN_NO_FAST)
    # (past four times the front table's slots the answer depends on what the mirror has seen before: either kernel is right)
    lanes = res.lanes if lanes_can and ngroups > 4 * front_table_slots(state_bytes) else lanes_can
    want = INTERP_K if flags & capi.PLAN_NO_FAST else LANES_K if lanes else JIT_K if jit_asked else FAST_K
    assert k.startswith(want), (flags, want, k)
    assert res.path == "hash" or not timey, (flags, res.path)
    assert res.lanes == lanes and res.jit == (want == JIT_K) and res.fast == (want != INTERP_K), (flags, k, res.flags)
    assert res.hpart == hpart and ("_hpagg" in k and "scatter_kernel" in k) == hpart, (flags, k)
    if flags == PACK_NL or (flags == PACK and not lanes):        # the lanes kernels read column ranges, never records
        assert res.packed, (flags, res.flags)
    elif not jit_asked:                                          # no filter: nothing to gather for, whatever projections earlier cases left behind
        assert not res.packed, (flags, res.flags)


# ---- a. every unit on every path
@pytest.mark.parametrize("gran", GRANS, ids=lambda g: g or "none")
@pytest.mark.parametrize("kind", ["time", "microtime"])
def test_every_unit_on_every_path(mirrors, kind, gran):
    tab, dt = edge(mirrors, kind)
    micro = kind == "microtime"
    want_keys = {te.truth_value(v, micro, gran) for v in te.table_values(tab)}
    one_word = key_words(tab, ["ts", "k"]) == 1
    st = None
    for flags in FLAG_SETS:
        res, st = run(tab, dt, select(gran), flags=flags, st=st, label=f"a {kind} {gran}")
        check_path(res, flags, gran is not None, one_word, 4 + 8, st.ngroups)
        assert {int(x) for x in res.keys[0]} == want_keys, (kind, gran, flags)
    if gran in ("month", "second") and not JIT_OFF:
        # COUNT and SUM(long) together are 96 bits of payload: hashed partitioning was refused above. One 64-bit state: it runs (one key word only)
        res, _ = run(tab, dt, select(gran, metrics=("long_sum",)), flags=HPART, label=f"a {kind} {gran} hpart")
        check_path(res, HPART, True, one_word, 8, res.ngroups)
        res, _ = run(tab, dt, select(gran, dims=(), metrics=("long_sum",)), flags=HPART, label=f"a {kind} {gran} hpart, ts alone")
        check_path(res, HPART, True, True, 8, res.ngroups)
        assert {int(x) for x in res.keys[0]} == want_keys


# ---- b. two time keys at once
@pytest.mark.parametrize("grans", [("month", "hour"), ("year", "second")], ids=lambda g: "_".join(g))
def test_two_time_keys(mirrors, grans):
    tab, dt = edge(mirrors, "both")
    assert key_words(tab, ["ts", "uts"]) == 2
    q = {"select": [{"column": "ts", "granularity": grans[0]}, {"column": "uts", "granularity": grans[1]}, {"column": "count"}, {"column": "long_sum"}]}
    a, st = run(tab, dt, q, flags=JIT, label=f"b {grans}")
    b, _ = run(tab, dt, q, flags=INTERP, st=st, label=f"b {grans}")
    check_path(a, JIT, True, False, 12, st.ngroups)
    check_path(b, INTERP, True, False, 12, st.ngroups)
    pa, pb = np.lexsort(a.keys[::-1]), np.lexsort(b.keys[::-1])
    for x, y in zip(a.keys + a.states, b.keys + b.states):
        assert x.dtype == y.dtype and np.array_equal(x[pa], y[pb])
    assert {int(x) for x in a.keys[0]} == {te.truth(v, grans[0]) for v in te.table_values(tab, "ts")}
    assert {int(x) for x in a.keys[1]} == {te.truth_value(v, True, grans[1]) for v in te.table_values(tab, "uts")}


# ---- c. rule boundaries
@pytest.mark.parametrize("gran", [None, "hour", "day", "month"], ids=lambda g: g or "rules_alone")
@pytest.mark.parametrize("kind", ["time", "microtime"])
@pytest.mark.parametrize("name", sorted(te.RULE_SETS))
def test_rows_on_rule_boundaries(mirrors, name, kind, gran):
    tab, dt = boundary(mirrors, kind, name)
    micro = kind == "microtime"
    rules = te.named_rules(tab.column("ts"))
    want_keys = {te.rule_chain(v, micro, rules, gran) for v in te.table_values(tab)}
    q = select(gran, metrics=("count",)) if gran else {"dimensions": ["ts", "k"], "metrics": ["count"]}
    # NO_JIT without NO_LANES: what a plain query of this shape runs — on the 4-byte column the no-compaction kernel over the LDS front table
    # (a few hundred groups: check_path asserts it ran), the third place the rollup chain is restated in vh_kernels.h
    st = None
    for flags in (INTERP, NO_JIT, PREBUILT, JIT, HPART):
        res, st = run(tab, dt, q, flags=flags, st=st, label=f"c {name} {kind} {gran}")
        check_path(res, flags, True, not micro, 4, st.ngroups)
        assert {int(x) for x in res.keys[0]} == want_keys, (name, kind, gran, flags)
    if micro:      # (ts, k) is two key words on a microtime column: hashed partitioning and the lanes kernel were refused above; the time key alone is one
        q1 = select(gran, dims=(), metrics=("count",)) if gran else {"dimensions": ["ts"], "metrics": ["count"]}
        st = None
        for flags in (NO_JIT, HPART):
            res, st = run(tab, dt, q1, flags=flags, st=st, label=f"c {name} {kind} {gran} ts alone")
            check_path(res, flags, True, True, 4, st.ngroups)
            assert {int(x) for x in res.keys[0]} == want_keys, (name, kind, gran, flags)


# ---- d. boundaries handed straight to the C ABI
def groups_of(res):
    return {tuple(int(k[i]) for k in res.keys): tuple(int(s[i]) for s in res.states) for i in range(res.returned)}


def numpy_groups(keys, metrics):
    """{key tuple: (sum of every metric column)} by numpy.unique over the rows."""
    rows = np.stack([np.asarray(k).astype(np.uint64) for k in keys], axis=1)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    sums = []
    for m in metrics:
        acc = np.zeros(len(uniq), dtype=np.int64)
        np.add.at(acc, np.asarray(inv).ravel(), np.asarray(m).astype(np.int64))
        sums.append(acc)
    return {tuple(int(x) for x in u): tuple(int(s[i]) for s in sums) for i, u in enumerate(uniq)}


def mapped(col, fn):
    uniq, inv = np.unique(col, return_inverse=True)
    out = np.array([fn(int(u)) for u in uniq], dtype=object).astype(np.uint64)
    return out[np.asarray(inv).ravel()]


def columns_of(tab, names):
    out = []
    for n in names:
        c = tab.column(n)
        out.append(np.concatenate([(s["d"] if c.is_dim else s["m"])[c.index][:s["size"]] for s in tab.segments]))
    return out


U64_MAX = (1 << 64) - 1
ORDER = [capi.T_MONTH, capi.T_DAY, capi.T_HOUR]      # the nested rule set in the reference's order (longest `after` first)


@pytest.mark.parametrize("kind,bounds", [("time", [0, 0, 0]), ("time", [1, 1, 1]), ("time", [1 << 32] * 3), ("time", [(1 << 32) + 5] * 3),
                                         ("time", [0, 1, (1 << 32) + 5]), ("time", [1, 1 << 31, 1 << 32]),
                                         ("microtime", [U64_MAX] * 3), ("microtime", [0, (1 << 32) * 1000000, U64_MAX]), ("microtime", [1, 1 << 32, (1 << 32) + 5])],
                         ids=lambda v: v if isinstance(v, str) else "_".join(hex(x) for x in v))
@pytest.mark.parametrize("gran", [None, "day"], ids=lambda g: g or "rules_alone")
def test_boundaries_straight_through_the_c_abi(mirrors, kind, bounds, gran):
    """2^32 and 2^32 + 5 on a 4-byte column: every row lies before the boundary (compared in 32 bits it would be none, or the five values below
    5). UINT64_MAX on a microtime column: every row. 0: none; 1: the value 0 alone."""
    tab, dt = edge(mirrors, kind)
    micro = kind == "microtime"
    base = plan_from_query(tab, vo.parse_query(tab, dict({"type": "aggregate", "table": "t"}, **select(gran, metrics=("count",)))), now=NOW)
    rules_o = list(zip([vo.MONTH, vo.DAY, vo.HOUR], bounds))
    ts, k, cnt = columns_of(tab, ["ts", "k", "count"])
    want = numpy_groups([mapped(ts, lambda v: vo.rollup_ts(v, micro, rules_o, None if gran is None else te.UNIT_CODE[gran])), k], [cnt])
    if kind == "time" and min(bounds) > te.U32_MAX and gran is None:      # every row before the first boundary: all of them truncated to the month
        assert {key[0] for key in want} == {te.truth(v, "month") for v in te.table_values(tab)}
    got = {}
    for flags in (INTERP, NO_JIT, PREBUILT, JIT):      # (NO_JIT: on the 4-byte column the no-compaction kernel, as in c)
        plan = dataclasses.replace(base, flags=flags, groups=[dataclasses.replace(base.groups[0], rollup=list(zip(ORDER, bounds)))] + list(base.groups[1:]))
        res = dt.query_agg(plan)
        note(f"d {kind} {bounds} {gran}", flags, res)
        check_path(res, flags, True, not micro, 4, res.ngroups)
        got[flags] = groups_of(res)
        assert got[flags] == want, (kind, bounds, gran, flags, len(got[flags]), len(want))


# ---- e. ragged snapshots
@pytest.mark.parametrize("cut", [1, 1023, 1024, 1025])
@pytest.mark.parametrize("kind", ["time", "microtime"])
def test_ragged_snapshots(mirrors, kind, cut):
    tab, dt = edge(mirrors, kind)
    seg_rows = [cut, 0, te.SEG_ROWS[2], 0]
    st = None
    for flags in (JIT, PREBUILT):
        res, st = run(tab, dt, select("month"), flags=flags, st=st, seg_rows=seg_rows, label=f"e {kind} {cut}")
        check_path(res, flags, True, kind == "time", 12, st.ngroups)
        assert res.scanned_recs == cut + te.SEG_ROWS[2]
        assert {int(x) for x in res.keys[0]} == {te.truth_value(v, kind == "microtime", "month") for v in te.table_values(tab, seg_rows=seg_rows)}


# ---- f. packed forms
FEW = {"op": "lt", "column": "id", "value": "40"}      # ~4 % of the rows


def _add_row(tab, dt, segno, ts_value):
    """One more row at the end of a segment, on both sides."""
    sg = tab.segments[segno]
    n = sg["size"]
    extra_d = [ts_value, 3, 7]
    extra_m = [2, -5]
    for i, v in enumerate(extra_d):
        sg["d"][i] = np.concatenate([sg["d"][i][:n], np.array([v], dtype=sg["d"][i].dtype)])
    for j, v in enumerate(extra_m):
        sg["m"][j] = np.concatenate([sg["m"][j][:n], np.array([v], dtype=sg["m"][j].dtype)])
    sg["size"] = n + 1
    dt.sync_segment(segno, sg["d"] + sg["m"], n + 1)


@pytest.mark.parametrize("how", ["warm", "pack", "pack_jit"])
@pytest.mark.parametrize("kind", ["time", "microtime"])
def test_packed_forms_through_a_sync(kind, how):
    """Selective queries gather a survivor's time value from a record: a plain projection (pre-built kernels), or compressed / bit-field
    records (compiled kernels), whichever vh_table_prepare or VH_PLAN_FORCE_PACK builds. The narrow-span segment and the one-value segment
    give the oracle's keys; then a row far outside comes in by sync and the next answer is the oracle's again."""
    if how == "pack_jit" and JIT_OFF:
        pytest.skip("VH_JIT=off: compressed records are read by the per-query compiled kernels only")
    tab = te.edge_table(kind)
    dt = mirror_table(tab)
    flags = {"warm": 0, "pack": PACK | capi.PLAN_NO_JIT, "pack_jit": PACK | JIT}[how]
    # vh_table_prepare builds a projection unasked only where its records (a power of two of bytes) do not outgrow the table's own rows of 24 /
    # 28 bytes: ts, k and count make 16-byte records, long_sum with them 32. So the prepared query selects count alone; the forced ones both
    q = dict(select("month", metrics=("count",) if how == "warm" else ("count", "long_sum")), filter=FEW)
    late = te.U32_MAX if kind == "time" else te.LAST_SECOND * 1000000
    try:
        if how == "warm":
            aq = vo.parse_query(tab, dict({"type": "aggregate", "table": "t"}, **q))
            assert dt.warm(plan_from_query(tab, aq, now=NOW)) & capi.INFO_PACKED, "vh_table_prepare built no projection for a query that keeps 4 % of the rows"
        for step in ("built", "after the sync"):
            res, st = run(tab, dt, q, flags=flags, label=f"f {kind} {how} {step}")
            assert 0.02 < st.passed_recs / st.scanned_recs < 0.06
            assert res.packed and res.path == "hash", (how, step, res.pack_bits, res.pack_rec_bytes, res.flags)
            assert how != "pack" or not res.packed_compressed, (how, step, res.pack_bits, res.pack_rec_bytes)
            assert how != "pack_jit" or (res.packed_compressed and res.jit), (how, step, res.pack_bits, res.pack_rec_bytes)
            seg2 = {te.truth_value(int(v), kind == "microtime", "month") for v, i in zip(tab.segments[2]["d"][0], tab.segments[2]["d"][2]) if i < 40}
            assert seg2 <= {int(x) for x in res.keys[0]} and len(seg2) == (2 if step == "built" else 3), (how, step, res.pack_bits, res.pack_rec_bytes)
            if step == "built":
                _add_row(tab, dt, 2, late)
    finally:
        dt.close()


@pytest.mark.parametrize("kind", ["time", "microtime"])
def test_bit_field_time_outgrown_by_a_sync(kind):
    """Every time value of the table within two minutes of a month end: the bit-field record keeps the column at the bits of its largest
    value. One synced row holding the type's last second needs more (microtime: 52 -> 58 bits; time: both need all 32): the records are
    rebuilt, and the month of every row is still the oracle's."""
    if JIT_OFF:
        pytest.skip("VH_JIT=off: bit-field records are read by the per-query compiled kernels only")
    tab = te.narrow_table(kind)
    dt = mirror_table(tab)
    q = dict(select("month", metrics=("count",)), filter=FEW)
    try:
        dt.pack([0, 1, 3], compressed=True)
        res, st = run(tab, dt, q, flags=JIT, label=f"f narrow {kind} built")
        # (bit fields are taken where they make the record smaller: 57 bits against 7 + 1 + 1 bytes; 37 bits against 4 + 1 + 1 bytes are 8 bytes either way)
        assert res.packed and res.packed_compressed and res.pack_bits == (kind == "microtime") and res.pack_rec_bytes == 8, (res.pack_bits, res.pack_rec_bytes, res.flags)
        before = st.ngroups
        _add_row(tab, dt, 1, te.U32_MAX if kind == "time" else te.LAST_SECOND * 1000000)
        res, st = run(tab, dt, q, flags=JIT, label=f"f narrow {kind} after the sync")
        assert res.packed and res.packed_compressed and st.ngroups == before + 1, (res.pack_bits, res.pack_rec_bytes, res.flags)
    finally:
        dt.close()


# ---- g. an 8-byte non-micro time column (the C ABI allows it; the oracle's schema cannot say it)
@pytest.fixture(scope="module")
def wide_seconds():
    vals = np.array(te.EDGE_SECS + te.WIDE_SECS, dtype=np.uint64)
    dt = DeviceTable([(capi.DIM_TIME, capi.U64), (capi.DIM_NUMERIC, capi.U32), (capi.METRIC_COUNT, capi.U32), (capi.METRIC_SUM, capi.I64)], te.SEG_SIZE, 2)
    segs = []
    for s, (rows, stride) in enumerate(((5120, 1), (4453, 37))):
        i = np.arange(rows, dtype=np.int64)
        cols = [vals[(i * stride + 11 * s) % len(vals)], (i % 5).astype(np.uint32), (1 + i % 3).astype(np.uint32), ((i * 37) % 2001 - 1000).astype(np.int64)]
        dt.sync_segment(s, cols, rows)
        segs.append(cols)
    yield [np.concatenate([sg[c] for sg in segs]) for c in range(4)], dt
    dt.close()


@pytest.mark.parametrize("gran", te.UNITS)
def test_eight_byte_seconds_keep_all_64_bits(wide_seconds, gran):
    (ts, k, cnt, v), dt = wide_seconds
    assert len(te.EDGE_SECS) + len(te.WIDE_SECS) == 703 and 5120 % 703 and 4453 > 703
    want = numpy_groups([mapped(ts, lambda x: te.truth(x, gran)), k], [cnt, v])
    assert max(key[0] for key in want) > te.U32_MAX
    got = {}
    for flags in (INTERP, PREBUILT, JIT):
        res = dt.query_agg(AggPlan(groups=[GroupSpec(0, granularity=UNIT[gran]), GroupSpec(1)], metrics=[2, 3], flags=flags))
        note(f"g u64 seconds {gran}", flags, res)
        check_path(res, flags, True, False, 12, res.ngroups)
        assert res.keys[0].dtype == np.uint64
        got[flags] = groups_of(res)
        assert got[flags] == want, (gran, flags, len(got[flags]), len(want), sorted(set(got[flags]) ^ set(want))[:4])
    assert got[INTERP] == got[JIT] == got[PREBUILT]


# ---- h. through the host shim
def test_host_shim_formats_sorts_and_filters_edge_times():
    import time as _time
    from viyadb_amd import hostdb
    fmt = "%Y-%m-%d %H:%M:%S"
    tconf = {"name": "t", "segment_size": te.SEG_SIZE, "dimensions": [{"name": "ts", "type": "time", "format": fmt}, {"name": "k", "type": "uint"}, {"name": "id", "type": "uint"}],
             "metrics": [{"name": "count", "type": "count"}, {"name": "long_sum", "type": "long_sum"}]}
    tab = te.edge_table("time")
    text = {v: _time.strftime(fmt, _time.gmtime(v)) for v in te.table_values(tab)}
    rows = []
    for sg in tab.segments:
        n = sg["size"]
        for t, k, i, v in zip(sg["d"][0][:n].tolist(), sg["d"][1][:n].tolist(), sg["d"][2][:n].tolist(), sg["m"][1][:n].tolist()):
            rows.append([text[t], str(k), str(i), str(v)])
    gdb, odb = hostdb.Database({"tables": [tconf]}), vo.Database({"tables": [tconf]})
    try:
        gdb.load("t", rows, now=NOW)
        odb.table("t").load(rows, now=NOW)
        for q in ({"select": [{"column": "ts", "granularity": "month", "format": "%m/%Y"}, {"column": "k"}, {"column": "count"}, {"column": "long_sum"}]},
                  {"select": [{"column": "ts", "granularity": "year"}, {"column": "count"}, {"column": "long_sum"}], "sort": [{"column": "ts", "ascending": True}]},
                  {"select": [{"column": "ts", "granularity": "day"}, {"column": "k"}, {"column": "count"}], "filter": {"op": "ge", "column": "ts", "value": "2100-03-01 00:00:00"}}):
            q = dict({"type": "aggregate", "table": "t"}, **q)
            got, _ = gdb.query(q, now=NOW)
            want, _ = odb.query(q, now=NOW)
            assert sorted(map(tuple, got)) == sorted(map(tuple, want)) and len(got) > 10, (q, got[:3], want[:3])
    finally:
        gdb.close()
