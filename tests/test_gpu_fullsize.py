"""BASELINE.json's full sizes (C3: 1 B rows / 12 columns / 60 GB in HBM; C2: 100 M rows): the oracle cannot
follow there in seconds, so parity is carried by size-independent properties — totals that must agree across
independent kernel paths, linearity over segment ranges, idempotence — plus an exact oracle comparison on a
contiguous sample of the same generated rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
from tests.conftest import JIT_OFF  # noqa: E402
needs_jit = pytest.mark.skipif(JIT_OFF, reason="VH_JIT=off: this layout / form is read by the per-query compiled kernels only")


@pytest.fixture(scope="module")
def c3_full():
    from viyadb_amd import executor, synth
    executor.init(0)
    w = synth.c3()
    t = synth.create_device_table(w, 1000)
    yield w, t
    t.close()


def _plan(w, **kw):
    from viyadb_amd.executor import AggPlan
    d = dict(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, groups_hint=w.plan.groups_hint)
    d.update(kw)
    return AggPlan(**d)


def _canon(res):
    order = np.lexsort([k for k in reversed(res.keys)]) if res.keys else np.arange(res.ngroups)
    return [k[order] for k in res.keys], [s[order] for s in res.states]


def test_c3_full_size_properties(c3_full):
    w, t = c3_full
    full = t.query_agg(_plan(w))
    assert full.scanned_recs == 1_000_000_000 and full.scanned_segments == 1000
    assert full.ngroups == 100_000          # d0 x d1 = 1000 x 100, every cell is hit at 50 M survivors
    # (1) totals through an independent path: no GROUP BY -> LDS scalar table, different kernel instantiation
    tot = t.query_agg(_plan(w, groups=[]))
    assert tot.ngroups == 1 and tot.passed_recs == full.passed_recs
    assert int(full.states[0].sum(dtype=np.int64)) == int(tot.states[0][0])
    assert int(full.states[1].sum(dtype=np.uint64) & 0xFFFFFFFF) == int(tot.states[1][0])   # uint32 COUNT wraps mod 2^32
    # (2) every table organisation gives the same groups and states bit for bit
    kf, sf = _canon(full)
    for flags in (1, 1 | 2048, 8, 16 | 32, 64):   # hash table (arrays / records); generic kernel; no presence carrier; radix-partitioned
        other = t.query_agg(_plan(w, flags=flags))
        ko, so = _canon(other)
        assert other.ngroups == full.ngroups, flags
        for a, b in zip(kf + sf, ko + so):
            assert np.array_equal(a, b), flags
    # (3) linearity over segment ranges (size() snapshots of 0 hide a segment)
    lo = t.query_agg(_plan(w, seg_rows=[1_000_000] * 400 + [0] * 600))
    hi = t.query_agg(_plan(w, seg_rows=[0] * 400 + [1_000_000] * 600))
    assert lo.scanned_recs + hi.scanned_recs == full.scanned_recs and lo.passed_recs + hi.passed_recs == full.passed_recs
    acc = {}
    for part in (lo, hi):
        g = part.keys[0].astype(np.int64) * 100 + part.keys[1]
        for j in (0, 1):
            a = acc.setdefault(j, np.zeros(100_000, dtype=np.int64))
            np.add.at(a, g, part.states[j].astype(np.int64))
    g = kf[0].astype(np.int64) * 100 + kf[1]
    assert np.array_equal(acc[0][g], sf[0]) and np.array_equal((acc[1][g] & 0xFFFFFFFF).astype(np.uint32), sf[1])
    # (4) idempotence
    again = t.query_agg(_plan(w))
    for a, b in zip(kf + sf, sum(map(list, _canon(again)), [])):
        assert np.array_equal(a, b)


def test_c3_full_size_sample_against_oracle(c3_full):
    """Segments 497..499 of the 1 B-row table vs the oracle on the same generated rows."""
    from oracle import viya_oracle as vo
    from tests.parity import build_oracle_table, compare
    w, t = c3_full
    snap = [0] * 1000
    for s in (497, 498, 499):
        snap[s] = 1_000_000
    res = t.query_agg(_plan(w, seg_rows=snap))
    ot = build_oracle_table(w, 3, 1_000_000, row_base=497 * 1_000_000)
    st = vo.scan_aggregate(vo.parse_query(ot, w.query))
    st.scanned_recs, st.scanned_segments = res.scanned_recs, res.scanned_segments   # 997 hidden segments are still "scanned"
    compare(res, st, "C3 full table, 3-segment window")


@needs_jit
def test_c3_headline_configuration_is_what_bench_times(c3_full):
    """The configuration the bench line is quoted on — a caller that prepared its query shape (vh_table_prepare): compiled scan kernel,
    predicate columns out of the bit-packed predicate projection, payload out of 4-byte bit-field records, one-word tuples — checked
    in the GPU suite itself: the result flags say that IS what ran, the answer equals the hash organisation's bit for bit over the 10^9
    rows, and a 3-segment window equals the oracle on THAT plan. (Runs after the unprepared cases above: preparing changes the table's
    derived layouts for whatever follows.)"""
    from oracle import viya_oracle as vo
    from tests.parity import build_oracle_table, compare
    from viyadb_amd import capi
    w, t = c3_full
    plan = _plan(w)
    flags = t.warm(plan)
    res = t.query_agg(plan)
    assert res.flags == flags or (res.flags ^ flags) & ~512 == 0        # (bit 9, the placed pool, belongs to the context that ran)
    assert res.path == "dense_part" and res.jit and res.packed and res.packed_compressed and res.predpack and res.sliced and res.narrow, (res.flags, res.kernel)
    assert res.flags & capi.INFO_TUPLE1, "one-word tuples"
    assert res.scanned_recs == 1_000_000_000 and res.ngroups == 100_000
    other = t.query_agg(_plan(w, flags=1))
    kf, sf = _canon(res)
    ko, so = _canon(other)
    for a, b in zip(kf + sf, ko + so):
        assert np.array_equal(a, b)
    snap = [0] * 1000
    for s in (495, 496, 497, 498, 499):           # (5 M rows: a scan of fewer than VH_JIT_MIN_ROWS takes the pre-built kernels)
        snap[s] = 1_000_000
    win = t.query_agg(_plan(w, seg_rows=snap))
    assert win.jit and win.predpack and win.packed
    ot = build_oracle_table(w, 5, 1_000_000, row_base=495 * 1_000_000)
    st = vo.scan_aggregate(vo.parse_query(ot, w.query))
    st.scanned_recs, st.scanned_segments = win.scanned_recs, win.scanned_segments
    compare(win, st, "C3 prepared, 5-segment window")


@needs_jit
def test_one_word_tuples_replan_when_an_upsert_outgrows_their_bits():
    """One-word tuples (gid + every metric value in 63 bits, sized from the columns' recorded min / max) and bit-field records: between two
    queries an in-place upsert (vh_table_sync_batch, metrics only) makes m0 need more bits than were recorded. The stats widen with the
    batch, the next query plans wider tuples / records (or falls back) — and its answer is the oracle's."""
    from oracle import viya_oracle as vo
    from tests.parity import build_oracle_table, compare
    from viyadb_amd import capi, executor, synth
    from viyadb_amd.executor import AggPlan
    executor.init(0)
    w = synth.c3(segment_rows=500_000)
    nseg, rows = 10, 500_000                  # (5 M rows: enough for the library to compress projections and compile kernels unasked)
    t = synth.create_device_table(w, nseg, rows)
    try:
        ot = build_oracle_table(w, nseg, rows)
        plan = lambda: AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, groups_hint=w.plan.groups_hint,
                               flags=capi.PLAN_FORCE_JIT | capi.PLAN_FORCE_PART | capi.PLAN_FORCE_PACK)
        res = t.query_agg(plan())
        compare(res, vo.scan_aggregate(vo.parse_query(ot, w.query)), "before")
        assert res.jit and res.path == "dense_part" and res.flags & capi.INFO_TUPLE1 and res.packed_compressed
        # m0 (long_sum, values < 1001: 10 bits) of a few rows that PASS the filter in three segments becomes 2^40 + x; count of one row 77
        items = []
        for s in (1, 4, 6):
            seg = ot.segments[s]
            hit = np.nonzero((seg["d"][2] == 1) & (seg["d"][3] < 447) & (seg["d"][4] >= 553))[0][:5]
            assert len(hit) == 5
            lo, hi = int(hit.min()), int(hit.max()) + 1
            seg["m"][0][hit] = (1 << 40) + np.arange(5)
            if s == 4:
                seg["m"][2][hit[0]] = 77
            items.append((s, lo, hi - lo, rows, list(seg["d"]) + list(seg["m"]), capi.SYNC_METRICS_ONLY))
        t.sync_batch(items)
        res = t.query_agg(plan())
        compare(res, vo.scan_aggregate(vo.parse_query(ot, w.query)), "after the upsert")
        assert res.jit and res.path == "dense_part"
        res = t.query_agg(plan())                                   # steady again, same answer
        compare(res, vo.scan_aggregate(vo.parse_query(ot, w.query)), "steady")
    finally:
        t.close()


def test_c2_full_size_against_twin():
    """C2 at its full 100 M rows: the CPU twin finishes this one in seconds, so compare exactly."""
    from oracle import cpu_twin
    from tests.parity import build_oracle_table, compare
    from viyadb_amd import synth
    w = synth.c2()
    t = synth.create_device_table(w, 100)
    try:
        res = t.query_agg(_plan(w))
        ot = build_oracle_table(w, 100, 1_000_000)
        st = cpu_twin.Twin(ot, w.query).run()
        st.passed_recs = res.passed_recs
        compare(res, st, "C2 100M")
    finally:
        t.close()


def test_c5_per_gpu_share_properties():
    """BASELINE config 5 (time rollup + COUNT DISTINCT, millions of sparse groups) at one GPU's share of the 8-GPU run:
    125 M rows. Size-independent properties: COUNT is linear over segment ranges group by group, a distinct count is
    bounded by max / sum of the halves' distinct counts and by the ids stored, nothing depends on the run, and a
    two-segment window equals the oracle exactly."""
    from oracle import viya_oracle as vo
    from tests.parity import build_oracle_table, compare
    from viyadb_amd import executor, synth
    executor.init(0)
    w = synth.c5()
    nseg, rows = 125, 1_000_000
    t = synth.create_device_table(w, nseg)
    try:
        def run(snap=None):
            r = t.query_agg(_plan(w, seg_rows=snap))
            key = (r.keys[0].astype(np.uint64) << np.uint64(32)) | r.keys[1].astype(np.uint64)
            o = np.argsort(key, kind="stable")
            return r, key[o], r.states[0][o].astype(np.int64), r.states[1][o].astype(np.int64)

        full, kf, df, cf = run()
        assert full.path == "hash" and full.scanned_recs == nseg * rows
        assert full.ngroups == len(kf) == len(np.unique(kf)) > 20_000_000
        assert int(cf.sum()) >= full.passed_recs            # every stored row counts 1..3 (the generator's count column)
        assert (df >= 1).all() and (df <= 2 * cf).all()      # a stored row holds 2 ids; a group cannot see more than 2 per counted row
        lo, kl, dl, cl = run([rows] * 60 + [0] * 65)
        hi, kh, dh, ch = run([0] * 60 + [rows] * 65)
        assert lo.passed_recs + hi.passed_recs == full.passed_recs
        il, ih = np.searchsorted(kf, kl), np.searchsorted(kf, kh)
        assert (kf[il] == kl).all() and (kf[ih] == kh).all()
        c2, dsum, dmax = np.zeros_like(cf), np.zeros_like(df), np.zeros_like(df)
        c2[il] += cl; c2[ih] += ch
        dsum[il] += dl; dsum[ih] += dh
        dmax[il] = dl; dmax[ih] = np.maximum(dmax[ih], dh)
        assert np.array_equal(c2, cf)                        # COUNT: linear
        assert (df <= dsum).all() and (df >= dmax).all()     # COUNT DISTINCT: sub-additive, monotone
        again, ka, da, ca = run()
        assert np.array_equal(ka, kf) and np.array_equal(da, df) and np.array_equal(ca, cf)
        snap = [0] * nseg
        snap[61] = snap[62] = rows
        res = t.query_agg(_plan(w, seg_rows=snap))
        ot = build_oracle_table(w, 2, rows, row_base=61 * rows)
        st = vo.scan_aggregate(vo.parse_query(ot, w.query), now=w.now)
        st.scanned_recs, st.scanned_segments = res.scanned_recs, res.scanned_segments
        compare(res, st, "C5 125-segment table, 2-segment window")
    finally:
        t.close()
