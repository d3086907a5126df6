"""The result tail at its switches: which kernels end an aggregate, and that every one of them answers like the oracle.

Every aggregate ends in dense_merge_kernel, emit_groups_kernel<2> / <16>, small_tail_kernel and publish_header_kernel (vh_small_kernels.h), all
of which share the HAVING evaluator. result_finalize and query_scan_tail choose between them by four rules; the tables here sit on each:

  entries <= 8192 and entries x private copies x states <= 65536     one launch (the fused tail) or three
  G <= 16384 (or DENSE_PART's blocks per partition)                  private copies to add up, or a single table
  output region <= 8 MB and the mode is not HASH                     emission straight into pinned host memory, or scratch plus copies
  entries <= 4 Mi                                                    emit_groups_kernel<2> or <16>

Every case is compared with the oracle (tests.parity.compare), bit for bit with its twin under VH_TEST_NO_SMALL_TAIL=1 where it is eligible for
the fused tail, and its res.tail (vh_result_tail) with the rule worked out here from tail.entries, tail.copies, tail.states_per_entry and
tail.region_bytes. The pairs on a switch also assert the kind literally: the rule check alone would repeat the library's arithmetic.

Float metrics are multiples of 1/8 (as in the typed tables): sums are exact in any order, so twins compare bit for bit."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import extremes as X
from tests.conftest import JIT_OFF
from tests.having import apply_keep, having_nodes, keep_mask
from tests.parity import compare, sort_rows
from tests.planner import mirror_table, plan_from_query
from viyadb_amd import capi

pytestmark = pytest.mark.gpu

GLOBAL, HASH, PART, JIT, HPART = capi.PLAN_FORCE_GLOBAL, capi.PLAN_FORCE_HASH, capi.PLAN_FORCE_PART, capi.PLAN_FORCE_JIT, capi.PLAN_FORCE_HPART
NO_XCD, NO_CARRIER = capi.PLAN_NO_XCD_PRIVATE, capi.PLAN_NO_CARRIER
SMALL_TAIL_MAX, SMALL_TAIL_STATES, DIRECT_BYTES, EMIT2_MAX = 8192, 65536, 8 << 20, 4 << 20
FUSED, EMIT2, EMIT16, NONE = capi.TAIL_FUSED, capi.TAIL_EMIT2, capi.TAIL_EMIT16, capi.TAIL_NONE


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def F(op, col, val):
    return {"op": op, "column": col, "value": str(val)}


# ------------------------------------------------------------------------------------------------------------------------------------
# table A: 3 segments of 32 768 rows; a group column per extent, a pattern column that selects which entries exist
# ------------------------------------------------------------------------------------------------------------------------------------
NSEG, SEG = 3, 32768
EXTENTS = [2048, 2049, 2730, 2731, 4096, 4097, 8192, 8193, 8320, 8704, 16384, 16385]
EMAX = max(EXTENTS)
PAIR = (64, 128)                                             # two columns whose product is 8192
HOT = 100                                                    # per segment and pattern: rows of groups that hold rows in every segment
A_METRICS = [("count", "count"), ("usum", "uint_sum"), ("lsum", "long_sum"), ("imin", "int_min"), ("dmax", "double_max"), ("fsum", "float_sum"),
             ("iavg", "int_avg"), ("s1", "ulong_sum"), ("s2", "short_sum"), ("s3", "double_sum"), ("s4", "ushort_sum")]


def gcol(extent):
    return "e%d" % extent


def col_type(extent):
    return "ushort" if EXTENTS.index(extent) % 2 == 0 else "uint"


def col_lo(extent):
    return 1000 + EXTENTS.index(extent) if col_type(extent) == "ushort" else 3_000_000_000 + EXTENTS.index(extent)


def members(pattern, extent):
    """The table entries of a pattern, in member order: (0) every entry; (1) entries 0 and n - 1; (2) every second entry; (3) lane 63 of every
    64; (4) the 128-entry span [128, 256) empty between full ones."""
    a = np.arange(extent, dtype=np.int64)
    if pattern == 0:
        return a
    if pattern == 1:
        return np.array([0, extent - 1], dtype=np.int64)
    if pattern == 2:
        return a[::2]
    if pattern == 3:
        return a[63::64]
    assert pattern == 4
    return a[(a < 128) | (a >= 256)]


def table_a(with_count=True):
    """Row i carries a pattern `pat`, a member number and a filter column `q`. In the column of extent E it holds lo_E + members(pat, E)[member
    % len]: `pat == k and q < len(members(k, E))` then selects every entry of pattern k exactly once (q == member for those rows), so most
    groups hold one row and live in one private copy only — plus the HOT rows of every segment (q == 0: they always pass), the same groups
    in all three segments. pat takes 0..4 and 6: the literal 5 lies inside the recorded range and no row holds it. Both ends of every
    column's range occur among the rows of pattern 0. with_count=False: the same table without its COUNT metric, which gives it the hidden
    count an AVG then needs (the reference's rule: a table has one or the other)."""
    rng = np.random.default_rng(23)
    n = NSEG * SEG
    pat = np.full(n, 6, dtype=np.int64)
    member = rng.integers(0, EMAX, n)
    q = np.full(n, 1 << 30, dtype=np.int64)
    slots = np.ones(n, dtype=bool)
    for s in range(NSEG):                                    # the hot rows first in every segment: the same (pattern, member) in each
        for j, k in enumerate((0, 2, 4)):
            at = s * SEG + j * HOT + np.arange(HOT)
            pat[at], member[at], q[at] = k, (np.arange(HOT) * 37 + 5) * 41, 0
            slots[at] = False
    free = rng.permutation(np.nonzero(slots)[0])
    used = 0
    for k in range(5):
        cnt = len(members(k, EMAX))
        at = free[used:used + cnt]
        used += cnt
        pat[at], member[at], q[at] = k, np.arange(cnt), np.arange(cnt)
    assert used < len(free)                                  # (the rest keeps pat == 6)

    def column(extent, lo, dtype, sub=None):
        out = np.zeros(n, dtype=np.int64)
        for k in range(5):
            sel = pat == k
            m = members(k, extent)
            out[sel] = m[member[sel] % len(m)]
        sel = pat == 6
        out[sel] = member[sel] % extent
        if sub is not None:
            out = sub(out)
        return (out + lo).astype(dtype)

    dims = [{"name": gcol(e), "type": col_type(e)} for e in EXTENTS]
    dims += [{"name": "ga", "type": "ushort"}, {"name": "gb", "type": "uint"}, {"name": "pat", "type": "ubyte"}, {"name": "q", "type": "uint"},
             {"name": "patw", "type": "uint"}]      # (pat once more, four bytes wide: the pre-built register-resident scan reads no narrower predicate)
    mets = [{"name": nm, "type": ty} for nm, ty in A_METRICS if with_count or ty != "count"]
    tab = vo.Table({"name": "a", "segment_size": SEG, "dimensions": dims, "metrics": mets})
    dcols = [column(e, col_lo(e), vo.NUMERIC_TYPES[col_type(e)][0]) for e in EXTENTS]
    dcols.append(column(PAIR[0] * PAIR[1], 7, np.uint16, lambda v: v // PAIR[1]))
    dcols.append(column(PAIR[0] * PAIR[1], 100_000, np.uint32, lambda v: v % PAIR[1]))
    dcols += [pat.astype(np.uint8), q.astype(np.uint32), pat.astype(np.uint32)]
    mcols = {"count": rng.integers(1, 4, n).astype(np.uint32), "usum": rng.integers(0, 3, n).astype(np.uint32),      # (sums of 0: the group still exists)
             "lsum": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), "imin": rng.integers(-(1 << 30), 1 << 30, n).astype(np.int32),
             "dmax": (rng.integers(-4000, 4000, n) / 8.0).astype(np.float64), "fsum": (rng.integers(-2000, 2000, n) / 8.0).astype(np.float32),
             "iavg": rng.integers(-1000, 1000, n).astype(np.int32), "s1": rng.integers(0, 1 << 50, n).astype(np.uint64),
             "s2": rng.integers(-60, 60, n).astype(np.int16), "s3": (rng.integers(-2000, 2000, n) / 8.0).astype(np.float64),
             "s4": rng.integers(0, 60, n).astype(np.uint16)}
    for s in range(NSEG):
        sl = slice(s * SEG, (s + 1) * SEG)
        tab.add_segment_arrays([c[sl] for c in dcols], [mcols[m["name"]][sl] for m in mets],
                               None if with_count else np.ones(SEG, dtype=np.uint64), SEG)
    return tab


class Bench:
    """An oracle table, its device mirror, and the oracle's answers (asked once per query, shared by the cases that repeat it)."""

    def __init__(self, tab):
        self.tab, self.dt, self.cache = tab, mirror_table(tab), {}

    def oracle(self, q, seg_rows=None):
        key = json.dumps({k: v for k, v in q.items() if k != "having"}, sort_keys=True) + repr(seg_rows)
        aq = vo.parse_query(self.tab, q)
        if key not in self.cache:
            self.cache[key] = vo.scan_aggregate(aq, now=0, seg_rows=seg_rows)
        st = self.cache[key]
        return aq, dataclasses.replace(st, keys=list(st.keys), states=list(st.states))

    def close(self):
        self.dt.close()


@pytest.fixture(scope="module")
def A():
    b = Bench(table_a())
    yield b
    b.close()


@pytest.fixture(scope="module")
def A_hidden():
    b = Bench(table_a(with_count=False))
    yield b
    b.close()


def a_query(dims, metrics, pattern, extent, pat="pat"):
    n = len(members(pattern, extent)) if pattern < 5 else EMAX
    return {"type": "aggregate", "table": "a", "dimensions": list(dims), "metrics": list(metrics),
            "filter": {"op": "and", "filters": [F("eq", pat, pattern), F("lt", "q", n)]}}


# ------------------------------------------------------------------------------------------------------------------------------------
# the rule, the twins, the comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def kind_by_rule(res, no_small_tail=False, having=False):
    """What result_finalize must have launched, from the sizes the result reports (and nothing else of the library's)."""
    t = res.tail
    dense = res.path != "hash"
    one_shot = t.region_bytes <= DIRECT_BYTES
    if res.hpart and not having:
        return NONE, False
    fused = (dense and one_shot and t.entries <= SMALL_TAIL_MAX and t.entries * max(1, t.copies) * max(1, t.states_per_entry) <= SMALL_TAIL_STATES
             and not no_small_tail)
    return (FUSED if fused else EMIT2 if t.entries <= EMIT2_MAX else EMIT16), dense and one_shot


def check_tail(res, label, no_small_tail=False, having=False):
    t = res.tail
    kind, direct = kind_by_rule(res, no_small_tail, having)
    what = (label, capi.TAIL_KIND_NAMES[t.kind], t.direct, t.merged, t.copies, t.entries, t.states_per_entry, t.region_bytes)
    print("tail:", *what)      # (shown with -s, or when the case fails)
    assert t.kind == kind and bool(t.direct) == direct, what
    if res.path == "hash" or t.copies == 1:
        assert t.merged == capi.MERGE_NONE and t.copies == 1, what
    else:
        assert t.merged == (capi.MERGE_FUSED if kind == FUSED else capi.MERGE_KERNEL), what
    return t


def same_bits(a, b, label):
    """tests/test_gpu_gplanes.py's same_bits, float columns included (compared as their bits)."""
    pa, pb = sort_rows(a.keys, a.states), sort_rows(b.keys, b.states)
    assert a.passed_recs == b.passed_recs and a.ngroups == b.ngroups and a.returned == b.returned, label
    cols_a = a.keys + a.states + ([a.hidden_count] if a.hidden_count is not None else [])
    cols_b = b.keys + b.states + ([b.hidden_count] if b.hidden_count is not None else [])
    assert len(cols_a) == len(cols_b), label
    for x, y in zip(cols_a, cols_b):
        assert x.dtype == y.dtype and x[pa].tobytes() == y[pb].tobytes(), label


class no_small_tail:
    def __enter__(self):
        os.environ["VH_TEST_NO_SMALL_TAIL"] = "1"

    def __exit__(self, *exc):
        del os.environ["VH_TEST_NO_SMALL_TAIL"]


def ask(b, q, flags=0, groups_hint=0, seg_rows=None, label="", twin=True):
    """One case, three ways: the oracle, the twin without the fused tail (where the fused tail was taken), res.tail against the rule."""
    aq, st = b.oracle(q, seg_rows)
    plan = plan_from_query(b.tab, aq, now=0, flags=flags, groups_hint=groups_hint, seg_rows=seg_rows)
    res = b.dt.query_agg(plan)
    label = f"{label} flags={flags:#x} {json.dumps(q.get('dimensions'))} {q.get('metrics')}"
    compare(res, st, label)
    t = check_tail(res, label)
    if twin and t.kind == FUSED:
        with no_small_tail():
            other = b.dt.query_agg(plan)
        compare(other, st, label + " (three launches)")
        ot = check_tail(other, label + " (three launches)", no_small_tail=True)
        assert ot.kind == EMIT2 and ot.direct == 1 and (ot.entries, ot.copies, ot.states_per_entry) == (t.entries, t.copies, t.states_per_entry), label
        same_bits(res, other, label + ": fused tail against three launches")
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused switch
# ------------------------------------------------------------------------------------------------------------------------------------
STATES = ["count", "usum", "lsum", "imin", "dmax", "fsum", "iavg", "s1", "s2"]
SWITCH_8 = [((gcol(8192),), 8192, 1, FUSED), ((gcol(8193),), 8193, 1, EMIT2), ((gcol(4096),), 4096, 2, FUSED), ((gcol(4097),), 4097, 2, EMIT2),
            ((gcol(2730),), 2730, 3, FUSED), ((gcol(2731),), 2731, 3, EMIT2), ((gcol(2048),), 2048, 4, FUSED), ((gcol(2049),), 2049, 4, EMIT2),
            (("ga", "gb"), 8192, 1, FUSED)]


@pytest.mark.parametrize("dims,extent,nstates,kind", SWITCH_8, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_dense_fused_switch_with_private_copies(A, dims, extent, nstates, kind):
    """Eight private copies: 8192 x 8 x 1, 4096 x 8 x 2, 2730 x 8 x 3 and 2048 x 8 x 4 states are the last the one block reads; one entry more and the three
    launches answer. Under the planner's own choice, DENSE_GLOBAL with the carrier and with presence bytes; every entry, the two ends, every
    second entry, and none at all."""
    for flags in (0, GLOBAL, GLOBAL | NO_CARRIER):
        for pattern in (0, 1, 2, 5):
            res = ask(A, a_query(dims, STATES[:nstates], pattern, extent), flags, label=f"pattern {pattern}")
            t = res.tail
            assert t.states_per_entry == nstates, (flags, pattern, t.states_per_entry)
            if flags & GLOBAL:
                assert res.path == "dense_global" and (t.entries, t.copies) == (extent, 8), (flags, res.path, t.entries, t.copies)      # (MI355X: one copy per XCD)
            if (t.entries, t.copies) == (extent, 8):
                assert t.kind == kind and t.direct == 1 and t.merged == (capi.MERGE_FUSED if kind == FUSED else capi.MERGE_KERNEL), (flags, pattern, t.kind)
            assert res.ngroups == (len(members(pattern, extent)) if pattern < 5 else 0)


@pytest.mark.parametrize("hidden,extent,nsel,nstates,kind", [(True, 8192, 7, 8, FUSED), (True, 8192, 8, 9, EMIT2), (False, 8192, 8, 8, FUSED),
                                                            (False, 8192, 9, 9, EMIT2), (False, 8193, 1, 1, EMIT2)])
def test_dense_fused_switch_with_one_copy(A, A_hidden, hidden, extent, nsel, nstates, kind):
    """PLAN_NO_XCD_PRIVATE: one table. 8192 entries x 8 states are 65536 and fused, 8192 x 9 and 8193 x 1 are not. The hidden cases select an
    AVG on the table without COUNT: the hidden count is a state like the others (8 = 7 selected + 1, 9 = 8 + 1)."""
    b = A_hidden if hidden else A
    metrics = [m for m in STATES if not (hidden and m == "count")][:nsel]
    for pattern in (0, 1, 2, 5):
        res = ask(b, a_query((gcol(extent),), metrics, pattern, extent), GLOBAL | NO_XCD, label=f"one copy, pattern {pattern}")
        t = res.tail
        assert (t.entries, t.copies, t.states_per_entry) == (extent, 1, nstates) and (res.hidden_count is not None) == hidden
        assert t.kind == kind and t.direct == 1 and t.merged == capi.MERGE_NONE, (pattern, t.kind, t.merged)


PART_CASES = [(4096, ["lsum", "s1"], 8, FUSED), (4096, ["lsum", "s1", "s3"], 8, EMIT2), (8192, ["lsum", "s1"], 4, FUSED), (8193, ["lsum", "s1"], None, EMIT2),
              (8192, ["lsum", "count"], None, EMIT2)]      # (two-word tuples: the compiled scan's ring writer counts them per partition)


@pytest.mark.parametrize("jit", [0, JIT], ids=["prebuilt", "compiled"])
def test_dense_part_on_the_fused_switch(A, jit):
    """DENSE_PART: a private copy of a partition's range per phase-2 block, as many blocks per partition as the CUs allow. The planner takes it
    only for a table that does not fit the 40 KB LDS budget (PLAN_FORCE_PART forces it no further), so these cases carry 8-byte states, and
    VH_PART_TABLE_KB=4 makes the ranges 128 entries: on 256 CUs 4096 entries then have 8 copies and 8192 have 4 — with two states both are
    exactly 65536 states and fused; a third state, or one entry more, is not. The last case (a 64-bit sum and COUNT: tuples of two words, 8192
    x 8 x 2 states) is where the compiled leg shares phase 2's blocks out by the partitions' tuple counts — more copies than blocks per
    partition then exist — and dense_merge_kernel reads only the copies a partition's blocks wrote (its part_count branch). `copies` is read
    from res.tail and asserted; the kinds are asserted literally."""
    os.environ["VH_PART_TABLE_KB"] = "4"
    try:
        kinds = set()
        for extent, metrics, copies, kind in PART_CASES:
            for pattern in (0, 1, 2, 5):
                res = ask(A, a_query((gcol(extent),), metrics, pattern, extent, pat="patw"), PART | jit, label=f"DENSE_PART {extent}, pattern {pattern}")
                t = res.tail
                assert res.path == "dense_part" and t.entries == extent and t.copies > 1, (res.path, t.entries, t.copies, res.kernel)
                assert t.merged == (capi.MERGE_FUSED if t.kind == FUSED else capi.MERGE_KERNEL), (t.kind, t.merged)
                assert copies is None or t.copies == copies, (extent, metrics, t.copies)      # (MI355X: 256 CUs over the partitions)
                assert t.kind == kind, (extent, metrics, t.copies, capi.TAIL_KIND_NAMES[t.kind])
                kinds.add(t.kind)
                if jit and not JIT_OFF:
                    assert res.jit, res.kernel
                    if metrics == ["lsum", "count"]:
                        assert t.copies > 8, t.copies      # (shared out by tuple counts: up to 128 copies, of which a partition's blocks wrote some)
        assert kinds == {FUSED, EMIT2}, kinds
    finally:
        del os.environ["VH_PART_TABLE_KB"]


@pytest.mark.parametrize("extent", [8193, 8320, 8704, 16384, 16385])
def test_dense_emit2_span_and_block_edges(A, extent):
    """emit_groups_kernel<2>: a wave covers 128 entries, a block 512. 8193 = one entry into a new span; 8320 = 65 spans, 8704 = 17 blocks, full to
    the last lane; 16385 is the first table without private copies. All six patterns: every entry, the two ends, every second entry, lane 63
    alone, a whole span empty between full ones (its wave returns early), nothing."""
    for flags in (GLOBAL, GLOBAL | NO_CARRIER):
        for pattern in range(6):
            res = ask(A, a_query((gcol(extent),), ["count", "lsum", "fsum"], pattern, extent), flags, label=f"emit<2> pattern {pattern}")
            t = res.tail
            assert t.kind == EMIT2 and t.direct == 1 and t.entries == extent, (pattern, t.kind, t.direct, t.entries)
            if extent == 16385:
                assert t.copies == 1 and t.merged == capi.MERGE_NONE, (t.copies, t.merged)
            else:
                assert t.copies == 8 and t.merged == capi.MERGE_KERNEL, (t.copies, t.merged)
            assert res.ngroups == (len(members(pattern, extent)) if pattern < 5 else 0)


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "three_launches"])
def test_dense_empty_snapshot_after_a_full_query(A, unfused):
    """A snapshot that shows none of the table's rows, asked directly after a full query on the same context: no group, no count, nothing
    left over from the query before — through the fused tail and through the three launches."""
    q = a_query((gcol(4096),), ["count", "usum", "iavg"], 0, 4096)
    for flags in (GLOBAL, GLOBAL | NO_CARRIER, 0):
        if unfused:
            os.environ["VH_TEST_NO_SMALL_TAIL"] = "1"
        try:
            aq, st = A.oracle(q)
            full = A.dt.query_agg(plan_from_query(A.tab, aq, now=0, flags=flags))
            compare(full, st, "full query")
            assert full.ngroups == 4096
            aq, st0 = A.oracle(q, seg_rows=[0] * NSEG)
            res = A.dt.query_agg(plan_from_query(A.tab, aq, now=0, flags=flags, seg_rows=[0] * NSEG))
            compare(res, st0, "empty snapshot")
            check_tail(res, "empty snapshot", no_small_tail=unfused)
            assert res.tail.kind == (EMIT2 if unfused else FUSED)
            assert res.ngroups == 0 and res.returned == 0 and res.scanned_recs == 0 and res.passed_recs == 0 and all(len(k) == 0 for k in res.keys + res.states)
        finally:
            os.environ.pop("VH_TEST_NO_SMALL_TAIL", None)


# ------------------------------------------------------------------------------------------------------------------------------------
# table B: 2 segments of 600 000 rows (dense_limit is four times the rows scanned: 4 Mi + 1 dense entries need more than 1 048 576 rows)
# ------------------------------------------------------------------------------------------------------------------------------------
B_SEG = 600_000
B_COLS = {"c1": 4_194_304, "c2": 4_194_305, "m1": 1_040_000, "m2": 1_056_000}


def table_b():
    rng = np.random.default_rng(31)
    tab = vo.Table({"name": "b", "segment_size": B_SEG, "dimensions": [{"name": c, "type": "uint"} for c in B_COLS],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "lsum", "type": "long_sum"}]})
    for s in range(2):
        dims = []
        for k, (c, extent) in enumerate(B_COLS.items()):
            v = rng.integers(0, extent, B_SEG)
            v[0], v[1] = (0, extent - 1) if s == 0 else (extent - 1, 0)      # both ends of the range, in either segment
            dims.append((v + 10 * (k + 1)).astype(np.uint32))
        tab.add_segment_arrays(dims, [rng.integers(1, 3, B_SEG).astype(np.uint32), rng.integers(-(1 << 40), 1 << 40, B_SEG).astype(np.int64)], None, B_SEG)
    return tab


@pytest.fixture(scope="module")
def B():
    b = Bench(table_b())
    yield b
    b.close()


def b_query(dims, metrics=("count", "lsum")):
    return {"type": "aggregate", "table": "b", "dimensions": list(dims), "metrics": list(metrics)}


@pytest.mark.parametrize("col,kind", [("c1", EMIT2), ("c2", EMIT16)])
def test_big_dense_emit2_against_emit16(B, col, kind):
    """A dense table of 4 Mi entries is the last emit_groups_kernel<2> walks; 4 Mi + 1 take <16>. Either region is far beyond 8 MB: emitted
    into scratch, packed on its way out."""
    res = ask(B, b_query([col]), GLOBAL, label="big dense")
    t = res.tail
    assert res.path == "dense_global" and t.entries == B_COLS[col] and t.kind == kind and t.direct == 0 and t.region_bytes > DIRECT_BYTES, (t.kind, t.entries, t.region_bytes)
    assert t.copies == 1 and t.merged == capi.MERGE_NONE


def test_big_hash_emit2_against_emit16(B):
    """A hash table's entries are its capacity + 1 (the reserved slot): groups_hint 2^20 and 2^21 give 2 Mi + 1 and 4 Mi + 1. (PLAN_NO_HPART:
    the hashed partitioning writes its rows itself, kind `none`, and would leave neither kernel to see.)"""
    kinds = {}
    for hint in (1 << 20, 1 << 21):      # (the capacity is the power of two at or above twice the hint)
        res = ask(B, b_query(["c1"]), HASH | capi.PLAN_NO_HPART, groups_hint=hint, label=f"big hash, hint {hint}")
        t = res.tail
        assert res.path == "hash" and t.direct == 0 and t.copies == 1, (res.path, t.direct)
        assert t.entries == 2 * hint + 1 or res.retries, (t.entries, hint, res.retries)
        kinds[t.kind] = t.entries
    assert set(kinds) == {EMIT2, EMIT16}, kinds
    assert kinds[EMIT2] == (2 << 20) + 1 and kinds[EMIT16] == (4 << 20) + 1, kinds


def test_big_region_on_either_side_of_8_mb(B):
    """The output region (header + columns laid out for every entry): up to 8 MB the kernels write rows and header into pinned host memory,
    beyond it into scratch. From a probe's bytes per entry: m1's table lies below 8 MB, m2's above."""
    probe = ask(B, b_query(["m1"], ["count"]), GLOBAL, label="region probe").tail
    per_entry = (probe.region_bytes - 512) / probe.entries
    at = DIRECT_BYTES / per_entry
    assert B_COLS["m1"] < at < B_COLS["m2"], (per_entry, at)
    small = ask(B, b_query(["m1"], ["count"]), GLOBAL, label="region below 8 MB")
    big = ask(B, b_query(["m2"], ["count"]), GLOBAL, label="region above 8 MB")
    assert small.tail.region_bytes <= DIRECT_BYTES < big.tail.region_bytes, (small.tail.region_bytes, big.tail.region_bytes)
    assert small.tail.direct == 1 and big.tail.direct == 0 and small.tail.kind == EMIT2 and big.tail.kind == EMIT2
    assert DIRECT_BYTES - small.tail.region_bytes < DIRECT_BYTES // 50 and big.tail.region_bytes - DIRECT_BYTES < DIRECT_BYTES // 50      # (within 2 % of the switch)


# ------------------------------------------------------------------------------------------------------------------------------------
# HAVING on every tail
# ------------------------------------------------------------------------------------------------------------------------------------
def ask_having(b, q, hv, flags=0, groups_hint=0, label="", edges=False, expect=None):
    """The query with `hv` pushed down, against the oracle's groups filtered by tests/having.py. res.ngroups must be the number of groups
    before HAVING, res.returned the number kept. edges: float SUM / AVG states against the exact sums (tests/extremes.py)."""
    q = dict(q, having=hv)
    aq, st = b.oracle(q)
    total = st.ngroups
    keep = keep_mask(b.tab, aq, st)
    apply_keep(st, keep)
    plan = plan_from_query(b.tab, aq, now=0, flags=flags, groups_hint=groups_hint)
    plan.having = having_nodes(b.tab, aq)
    res = b.dt.query_agg(plan)
    label = f"{label} flags={flags:#x} {q['dimensions']} having {json.dumps(hv)}"
    assert res.ngroups == total and res.returned == int(keep.sum()), (label, res.ngroups, total, res.returned, int(keep.sum()))
    if expect is not None:
        assert res.returned == expect, (label, res.returned, expect)
    t = check_tail(res, label, having=True)
    res.ngroups = res.returned
    if edges:
        addends = b.addends(q)
        kept = {tuple(k[row].item() for k in st.keys) for row in range(st.ngroups)}
        pos = X.float_sum_positions(aq)
        compare(X._without(res, pos), X._without(st, pos), label)
        X.check_float_sums(res.keys, res.states, aq, {k: v for k, v in addends.items() if k in kept}, label, pos)
    else:
        compare(res, st, label)
    if t.kind == FUSED:
        with no_small_tail():
            other = b.dt.query_agg(plan)
        assert other.tail.kind == EMIT2 and other.ngroups == total, label
        other.ngroups = other.returned
        if edges:      # (the edge table's float sums depend on the order two runs of one scan add in: everything else bit for bit, those against the exact sums)
            same_bits(X._without(res, pos), X._without(other, pos), label + ": fused tail against three launches")
            X.check_float_sums(other.keys, other.states, aq, {k: v for k, v in addends.items() if k in kept}, label + " (three launches)", pos)
        else:
            same_bits(res, other, label + ": fused tail against three launches")
    return res


def all_none_first_last(b, q, key, lo, hi, flags, kind, groups_hint=0, label=""):
    """A program that keeps every group, one that keeps none (no rows, ngroups still the total), one that keeps exactly the group of the
    lowest key and one that keeps exactly the highest — in a dense table the first and the last entry."""
    for hv, expect in ((F("ge", "count", 0), None), (F("lt", "count", 0), 0), (F("eq", key, lo), 1), (F("eq", key, hi), 1),
                       ({"op": "or", "filters": [F("le", key, lo), F("ge", key, hi)]}, 2)):
        res = ask_having(b, q, hv, flags, groups_hint, label, expect=expect)
        assert res.tail.kind == kind, (label, hv, capi.TAIL_KIND_NAMES[res.tail.kind])
        if expect == 0:
            assert all(len(c) == 0 for c in res.keys + res.states)
    return res


def test_having_on_the_fused_tail(A):
    e = 2048
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "usum", "lsum"]}
    for flags in (GLOBAL, GLOBAL | NO_CARRIER):
        res = all_none_first_last(A, q, gcol(e), col_lo(e), col_lo(e) + e - 1, flags, FUSED, label="fused")
        assert res.tail.copies == 8 and res.tail.merged == capi.MERGE_FUSED


def test_having_on_emit2_direct(A):
    e = 16385
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "usum", "lsum"]}
    res = all_none_first_last(A, q, gcol(e), col_lo(e), col_lo(e) + e - 1, GLOBAL, EMIT2, label="emit<2> direct")
    assert res.tail.direct == 1 and res.path == "dense_global"
    e = 8704                                                 # ... and behind dense_merge_kernel
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "usum", "lsum"]}
    res = all_none_first_last(A, q, gcol(e), col_lo(e), col_lo(e) + e - 1, GLOBAL, EMIT2, label="emit<2> direct, merged")
    assert res.tail.direct == 1 and res.tail.merged == capi.MERGE_KERNEL


def test_having_on_emit2_from_a_hash_table(A):
    """(Which group lies in a hash table's first slot cannot be seen from outside: the lowest and the highest key stand in. The last slot is
    the reserved one: test_having_keeps_the_group_in_the_reserved_slot.)"""
    e = 16385
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "usum", "lsum"]}
    res = all_none_first_last(A, q, gcol(e), col_lo(e), col_lo(e) + e - 1, HASH | capi.PLAN_NO_HPART, EMIT2, groups_hint=1 << 15, label="emit<2> hash")
    assert res.path == "hash" and res.tail.direct == 0 and not res.hpart


def test_having_on_the_compact_list_of_hashed_partitioning(A):
    e = 16385
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "usum"]}      # (its tuples carry 64 bits of states at most)
    plain = ask(A, q, HASH | JIT | HPART, label="hpart, no HAVING")      # (without HAVING its aggregation kernel writes the rows itself: kind `none`)
    assert JIT_OFF or (plain.hpart and plain.tail.kind == NONE and plain.tail.direct == 0), (plain.hpart, capi.TAIL_KIND_NAMES[plain.tail.kind])
    res = all_none_first_last(A, q, gcol(e), col_lo(e), col_lo(e) + e - 1, HASH | JIT | HPART, EMIT2, label="hpart list")
    assert res.path == "hash" and (JIT_OFF or res.hpart), (res.path, res.hpart, res.kernel)


def test_big_having_on_emit16(B):
    q = b_query(["c2"])
    lo = 20
    res = all_none_first_last(B, q, "c2", lo, lo + B_COLS["c2"] - 1, GLOBAL, EMIT16, label="emit<16>")
    assert res.tail.direct == 0


@pytest.fixture(scope="module")
def E():
    b = Bench(X.edge_table())
    cache = {}

    def addends(q):
        key = json.dumps({k: v for k, v in q.items() if k != "having"}, sort_keys=True)
        if key not in cache:
            cache[key] = X.group_addends(b.tab, vo.parse_query(b.tab, {k: v for k, v in q.items() if k != "having"}), 0, None)
        return cache[key]
    b.addends = addends
    yield b
    b.close()


def test_having_keeps_the_group_in_the_reserved_slot(E):
    """A one-word key that IS the empty marker (a long of -1, a ulong at its maximum) lives in the table's last, reserved entry. A two-word key
    has no such entry; there the leaf reads a column of the key's second word."""
    imax = (1 << 64) - 1
    for dims, hv in ((["d_long"], F("eq", "d_long", -1)), (["d_ulong"], F("eq", "d_ulong", imax)), (["d_ulong"], F("ne", "d_ulong", imax)),
                     (["d_ulong", "d_byte"], F("eq", "d_byte", -128)), (["d_long", "d_int", "d_ubyte"], F("ge", "d_ubyte", 255))):
        for flags in (HASH, HASH | capi.PLAN_FORCE_HASH_RECORDS):
            res = ask_having(E, X.key_query(dims, ("count", "long_sum", "int_min")), hv, flags, label="reserved slot")
            assert res.path == "hash" and res.tail.kind == EMIT2 and res.returned >= 1
            if hv["op"] == "eq" and len(dims) == 1:
                assert res.returned == 1 and int(res.keys[0][0]) == int(hv["value"]), (dims, res.keys[0])


def test_having_counts_the_groups_once_when_the_hash_table_regrows(A):
    e = 16385
    q = {"type": "aggregate", "table": "a", "dimensions": [gcol(e)], "metrics": ["count", "lsum"]}
    res = ask_having(A, q, F("ge", "count", 3), HASH | capi.PLAN_NO_HPART, groups_hint=1, label="regrow")
    assert res.retries >= 1 and res.path == "hash", res.retries
    assert 0 < res.returned < e


def leaves(n):
    pool = [F("ge", "count", 2), F("lt", "usum", 2), F("gt", "lsum", 0), F("ne", "count", 3), F("le", "usum", 0), F("lt", "lsum", -(1 << 39)),
            F("eq", "count", 1), F("gt", "usum", 1), F("ge", "lsum", 1 << 39)]
    return [pool[k % len(pool)] for k in range(n)]


def test_having_program_limits(A):
    """16 nodes are accepted and 17 are not; 24 literals and 25; stack depth 8 and 9; a program that leaves two values is invalid."""
    e = 2048
    q = a_query((gcol(e),), ["count", "usum", "lsum"], 0, e)      # (most groups hold one row: the leaves split them)
    L = leaves(10)
    inner = {"op": "or", "filters": [{"op": "and", "filters": L[5:8]}, {"op": "and", "filters": L[8:10]}]}
    tail = {"op": "and", "filters": [L[3], {"op": "and", "filters": [L[4], inner]}]}
    p16 = {"op": "or", "filters": [L[0], L[1], L[2], tail]}                       # 10 leaves + 6 operators, eight values on the stack at its deepest
    p17 = {"op": "or", "filters": [L[0], {"op": "or", "filters": [L[1], L[2], tail]}]}
    aq = vo.parse_query(A.tab, dict(q, having=p16))
    assert len(having_nodes(A.tab, aq)) == 16
    res = ask_having(A, q, p16, GLOBAL, label="16 nodes, depth 8")
    assert 0 < res.returned < e
    in24 = {"op": "in", "column": gcol(e), "values": [str(col_lo(e) + 3 * k) for k in range(24)]}
    assert ask_having(A, q, in24, GLOBAL, label="24 literals").returned == 24
    assert ask_having(A, q, {"op": "not", "filter": in24}, GLOBAL, label="24 literals, not in").returned == e - 24

    def refused(hv=None, nodes=None):
        aq = vo.parse_query(A.tab, dict(q, having=hv) if hv else q)
        plan = plan_from_query(A.tab, aq, now=0, flags=GLOBAL)
        plan.having = nodes if nodes is not None else having_nodes(A.tab, aq)
        with pytest.raises(capi.VhError) as err:
            A.dt.query_agg(plan)
        return err.value.code, len(plan.having)
    assert refused(p17) == (-4, 17)                                              # VH_E_UNSUPPORTED
    in25 = dict(in24, values=in24["values"] + [str(col_lo(e) + 100)])
    assert refused(in25) == (-1, 1)                                              # VH_E_INVALID
    assert refused({"op": "and", "filters": leaves(9)}) == (-4, 10)              # nine values on the stack
    assert ask_having(A, q, {"op": "and", "filters": leaves(8)}, GLOBAL, label="and of 8").tail.kind == FUSED
    two = having_nodes(A.tab, vo.parse_query(A.tab, dict(q, having={"op": "and", "filters": leaves(2)})))[:2]
    assert refused(nodes=two) == (-1, 2)                                         # two values left


FAR = {"float": "1e30", "double": "1e200"}      # float SUM / AVG leaves: see test_having_at_type_extremes


def wrapped_rows(E, t, aq, st, q):
    """Rows of the oracle's state whose integer SUM left the type's range (the state holds the wrapped value)."""
    info = np.iinfo(X.np_type(t))
    wide = E.addends(q)
    rows = [row for row in range(st.ngroups)
            if not info.min <= sum(int(x) for x in wide[tuple(k[row].item() for k in st.keys)][1]) <= info.max]
    return rows


def extreme_programs(E, t, aq, st, q):
    """[(program, splits)]: splits = the program must keep some of the oracle's groups and drop others (its literal is one group's own
    value); the others may keep all or none on one of the groupings."""
    info = None if t in X.FLOAT_TYPES else np.iinfo(X.np_type(t))
    lo = X.lit_str(t, -np.finfo(X.np_type(t)).max) if info is None else str(info.min)
    hi = X.lit_str(t, np.finfo(X.np_type(t)).max) if info is None else str(info.max)
    out = [(F("le", f"{t}_min", lo), False), (F("ge", f"{t}_max", hi), False)]
    if info is None:
        out += [(F(op, f"{t}_sum", FAR[t]), False) for op in ("ne", "eq", "lt", "ge")]      # (the NaN sums: ne keeps them; eq, lt and ge drop them)
        out += [(F("gt", f"{t}_avg", FAR[t]), False), (F("le", f"{t}_avg", "-" + FAR[t]), False)]
    else:
        rows = wrapped_rows(E, t, aq, st, q)
        assert rows, "no integer sum wraps"
        row = rows[len(rows) // 2]
        w, v = int(st.states[1][row]), int(st.states[4][row])      # one wrapped group's SUM and the raw sum of its AVG, as the type holds them
        mid = str((info.min + info.max) // 2)
        out += [(F("eq", f"{t}_sum", w), True), (F("ne", f"{t}_sum", w), True), (F("lt", f"{t}_sum", mid), False),
                (F("eq", f"{t}_avg", v), True), (F("gt", f"{t}_avg", mid), False)]
    if t == "ubyte":                                                                    # wraps to 0, as the reference's stoul + cast
        zero = int((st.states[2] == 0).sum())
        out += [(F("eq", "ubyte_min", "256"), 0 < zero < st.ngroups), (F("ne", "ubyte_min", "256"), 0 < zero < st.ngroups), (F("gt", "ubyte_max", "256"), False)]
    if t == "uint":                                                                     # wraps to 4294967295
        top = int((st.states[3] == 0xFFFFFFFF).sum())
        out += [(F("eq", "uint_max", "-1"), 0 < top < st.ngroups), (F("lt", "uint_min", "-1"), False)]
    return out


@pytest.mark.parametrize("dims,flags", [(["g"], 0), (["d_ulong", "d_byte"], HASH)], ids=["fused", "hash"])
@pytest.mark.parametrize("t", X.TYPES)
def test_having_at_type_extremes(E, t, dims, flags):
    """tests/extremes.edge_table grouped by g (16 groups: the fused tail) and by a two-word key (hash): per type, MIN against the type's minimum
    and MAX against its maximum, SUM and AVG leaves whose literal is the wrapped value of a group whose integer sum left the type's range
    (the comparison happens in the column's type; such a group exists on either grouping: asserted), and the float sums that are NaN
    (opposite infinities): `ne` keeps them, `eq`, `lt` and `ge` drop them. A float MIN of zero has a table of its own:
    test_having_float_min_of_zero.

    A leaf on a float SUM of finite values: the device adds in another order than the oracle, so a literal on top of a value would leave the
    oracle alone unable to decide the case. FAR (1e30 / 1e200) differs from every group's finite sum by orders of magnitude — asserted
    below: no finite oracle sum lies within a factor of 1000 of it, where parity's tolerance is 4e-6 relative."""
    q = X.metric_query(t, dims)
    aq, st = E.oracle(q)
    if t in X.FLOAT_TYPES:
        far = float(FAR[t])
        nan_groups = 0
        for j in X.float_sum_positions(aq):
            v = st.states[j].astype(np.float64)
            fin = v[np.isfinite(v)]
            assert not np.any((np.abs(fin) > far / 1000) & (np.abs(fin) < far * 1000)), (t, fin)
            nan_groups += int(np.isnan(v).sum())
        assert nan_groups > 0
    decided = 0
    for hv, splits in extreme_programs(E, t, aq, st, q):
        res = ask_having(E, q, hv, flags, label=f"extremes {t}", edges=t in X.FLOAT_TYPES)
        assert res.tail.kind == (FUSED if dims == ["g"] else EMIT2), capi.TAIL_KIND_NAMES[res.tail.kind]
        assert not splits or 0 < res.returned < st.ngroups, (hv, res.returned, st.ngroups)
        decided += 0 < res.returned < st.ngroups
        if t in X.FLOAT_TYPES and hv["column"] == f"{t}_sum":
            nan = int(np.isnan(res.states[1]).sum())
            assert (nan > 0) == (hv["op"] == "ne"), (hv, nan)
    assert decided >= 1, decided


ZKINDS = 8


def zero_table():
    """Float MINs around zero: 16 groups g, their kind g % 8. Kinds 0, 1, 3: +0.0 beside positive values, or alone — the minimum is +0.0;
    2: -0.0 beside positive values; 4: a negative subnormal; 5: a positive subnormal; 6: -1.5; 7: 3.0 beside +inf. (No group mixes the two
    zeros: the sign of such a minimum depends on the order the rows arrive in.)"""
    n = 4096
    g = (np.arange(n) % 16).astype(np.uint16)
    i = np.arange(n) // 16
    tab = vo.Table({"name": "z", "segment_size": n, "dimensions": [{"name": "g", "type": "ushort"}, {"name": "k", "type": "ulong"}, {"name": "b", "type": "byte"}],
                    "metrics": [{"name": "count", "type": "count"}, {"name": "float_min", "type": "float_min"}, {"name": "double_min", "type": "double_min"}]})
    cols = []
    for dt in (np.float32, np.float64):
        sub = dt(np.finfo(dt).smallest_subnormal)
        v = np.zeros(n, dtype=dt)
        kind = g % ZKINDS
        v[(kind == 0) & (i % 3 == 1)] = dt(1.5)
        v[(kind == 0) & (i % 3 == 2)] = dt(np.finfo(dt).tiny)
        v[kind == 2] = np.where(i[kind == 2] % 2 == 0, dt(-0.0), dt(2.0))
        v[(kind == 3) & (i % 5 == 0)] = dt(5.0)
        v[kind == 4] = np.where(i[kind == 4] % 4 == 0, -sub, dt(0.0))
        v[kind == 5] = np.where(i[kind == 5] % 4 == 0, sub, dt(1.0))
        v[kind == 6] = np.where(i[kind == 6] % 7 == 0, dt(-1.5), dt(0.0))
        v[kind == 7] = np.where(i[kind == 7] % 2 == 0, dt(np.inf), dt(3.0))
        cols.append(v)
    tab.add_segment_arrays([g, (g.astype(np.uint64) << np.uint64(40)) + np.uint64(7), (g.astype(np.int64) - 8).astype(np.int8)],
                           [np.ones(n, dtype=np.uint32)] + cols, None, n)
    return tab


@pytest.fixture(scope="module")
def Z():
    b = Bench(zero_table())
    yield b
    b.close()


@pytest.mark.parametrize("dims,flags,kind", [(["g"], 0, FUSED), (["g"], HASH, EMIT2), (["k", "b"], HASH, EMIT2)], ids=["fused", "hash", "hash_two_words"])
@pytest.mark.parametrize("t", X.FLOAT_TYPES)
def test_having_float_min_of_zero(Z, t, dims, flags, kind):
    """`t_min eq -0.0` keeps the groups whose minimum is +0.0 (and the one whose minimum is -0.0) and drops subnormal, negative and positive
    minima: the comparison is IEEE's, not one of bit patterns. On the fused tail and from a hash table, one-word and two-word keys."""
    q = {"type": "aggregate", "table": "z", "dimensions": list(dims), "metrics": ["count", f"{t}_min"]}
    aq, st = Z.oracle(q)
    mins = st.states[1]
    plus = int(((mins == 0) & ~np.signbit(mins)).sum())
    minus = int(((mins == 0) & np.signbit(mins)).sum())
    assert st.ngroups == 16 and plus == 6 and minus == 2, (st.ngroups, plus, minus)      # (the oracle holds +0.0 minima, and -0.0 ones)
    for hv, expect in ((F("eq", f"{t}_min", "-0.0"), 8), (F("eq", f"{t}_min", "0.0"), 8), (F("ne", f"{t}_min", "-0.0"), 8), (F("lt", f"{t}_min", "-0.0"), 4),
                       (F("ge", f"{t}_min", "-0.0"), 12), (F("gt", f"{t}_min", "0.0"), 4), (F("le", f"{t}_min", "0.0"), 12),
                       ({"op": "in", "column": f"{t}_min", "values": ["-0.0", "3.0"]}, 10)):
        res = ask_having(Z, q, hv, flags, label=f"zero {t}", expect=expect)
        assert res.tail.kind == kind and (res.path == "hash") == bool(flags & HASH), (capi.TAIL_KIND_NAMES[res.tail.kind], res.path)
        if hv.get("op") == "eq":
            kept = res.states[1]
            assert np.all(kept == 0) and int((~np.signbit(kept)).sum()) == 6 and int(np.signbit(kept).sum()) == 2, kept


@pytest.mark.parametrize("flags", [0, HASH], ids=["dense", "hash"])
def test_having_on_a_count_distinct(flags):
    """The table of test_gpu_typed.py::test_count_distinct: a bitset compares as its cardinality."""
    rng = np.random.default_rng(9)
    n = 8000
    tab = vo.Table({"name": "t", "segment_size": n, "dimensions": [{"name": "c", "type": "ushort"}, {"name": "x", "type": "uint"}],
                    "metrics": [{"name": "users", "type": "bitset", "max": 2 ** 31}, {"name": "count", "type": "count"}]})
    for _ in range(3):
        sets = [set(int(v) for v in rng.integers(0, 500, rng.integers(0, 4))) for _ in range(n)]
        tab.add_segment_arrays([rng.integers(0, 40, n).astype(np.uint16), rng.integers(0, 100, n).astype(np.uint32)],
                               [sets, np.ones(n, dtype=np.uint32)], None, n)
    b = Bench(tab)
    try:
        q = {"type": "aggregate", "table": "t", "dimensions": ["c", "x"], "metrics": ["users", "count"]}
        _, st = b.oracle(q)
        cut = int(np.median(st.states[0]))
        res = ask_having(b, q, F("ge", "users", cut), flags, label="count distinct")
        assert 0 < res.returned < res.ngroups + res.returned
        ask_having(b, q, {"op": "and", "filters": [F("ge", "users", cut), F("lt", "count", 8)]}, flags, label="count distinct and count")
    finally:
        b.close()


def test_nothing_depends_on_what_scratch_held():
    """The dense cases of this module (tables A and B, scratch emission and emit<16> included, and HAVING on the dense tails) again in a fresh process whose device scratch is filled with 0xA5 at allocation (VH_POISON): a tail that
    reads a word nobody wrote (a private copy no block of this query touched, a header word) shows as a wrong result instead of passing by
    luck."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VH_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_result_tail.py"), "-q", "-x", "-k",
                        "test_dense or test_big_dense or test_big_region or test_big_having or having_on_the_fused or having_on_emit2_direct"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
