"""Derived layouts through their whole life: payload projections (vh_table_pack), predicate planes (vh_table_predpack) and narrow copies
(vh_table_narrow) kept coherent with the arenas by the table's journal while syncs land, vh_table_prepare moves them to other allocations
(place_layouts: derived_move / derived_settle), readers and other prepares run beside it, values outgrow their stored widths, the table
grows and the journal drops its older half. Placement is made deterministic by the VH_TEST_PLACE_* hooks (tests/conftest.py opens the
gate): a fixed number of candidates, a fixed verdict, and — VH_TEST_PLACE_WAIT_SYNC — a sync of another thread inside every window between
a move and its settle. Every answer is checked against the oracle over the host's CURRENT arrays, and every check asserts which layout the
query read, so that none passes on the arenas alone."""
import threading
import time

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import build_oracle_table, compare
from tests.test_gpu_sync_batch import restat, seg_columns
from viyadb_amd import capi, synth
from viyadb_amd.executor import AggPlan, DeviceTable

pytestmark = pytest.mark.gpu
PACK, JIT = capi.PLAN_FORCE_PACK, capi.PLAN_FORCE_JIT
D2, D3, D4 = 2, 3, 4          # C3's filter columns (synth.c3): d2 = 1, d3 < 447, d4 >= 553; SUM m0 + COUNT by (d0, d1)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture
def place(monkeypatch):
    """Forced placement: n candidates, a verdict, optionally a sync in every window (the hooks are read per call)."""
    def set_(n, verdict, wait_sync=False):
        monkeypatch.setenv("VH_TEST_PLACE_CANDIDATES", str(n))
        monkeypatch.setenv("VH_TEST_PLACE_VERDICT", verdict)
        if wait_sync:
            monkeypatch.setenv("VH_TEST_PLACE_WAIT_SYNC", "1")
        else:
            monkeypatch.delenv("VH_TEST_PLACE_WAIT_SYNC", raising=False)
    return set_


class C3Host:
    """A C3-shaped table whose rows live in host arrays (the oracle's segments) and reach the mirror by vh_table_sync_batch only. Segments
    are generated with `cap` rows and hold `rows` of them, so that rows can be appended inside a segment."""

    def __init__(self, nseg, rows, cap, reserve=None, seed=42):
        self.w = synth.c3(segment_rows=cap)
        self.query, self.base = self.w.query, self.w.plan          # (what tests/cluster_shapes.py's comparisons take from a host)
        self.cap, self.seed = cap, seed
        self.tab = build_oracle_table(self.w, nseg, cap, seed=seed)
        for seg in self.tab.segments:
            seg["size"] = rows
            restat(self.tab, seg)
        self.dt = DeviceTable([(c.kind, c.elem) for c in self.w.columns], cap, reserve_segments=reserve or nseg)
        self.dt.sync_batch([(s, 0, rows, rows, seg_columns(self.tab, seg), 0) for s, seg in enumerate(self.tab.segments)])

    def plan(self, flags):
        p = self.w.plan
        return AggPlan(filter=p.filter, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint)

    def columns(self, s):
        return seg_columns(self.tab, self.tab.segments[s])

    def sync(self, s, first, n, ship_dims=True):
        """Send rows [first, first + n) of segment s as they stand in the host arrays."""
        seg = self.tab.segments[s]
        restat(self.tab, seg)
        self.dt.sync_batch([(s, first, n, seg["size"], self.columns(s), 0 if ship_dims else capi.SYNC_METRICS_ONLY)])

    def change(self, s, first, n, flip=True):
        """Metrics changed in place; with flip, the filter columns' values moved across the query's literals (d2 = 1 <-> 0,
        d3 < 447 <-> d3 > 552, d4 >= 553 <-> d4 < 447): a projection AND the planes go stale if they miss it."""
        seg = self.tab.segments[s]
        sl = slice(first, first + n)
        m0 = seg["m"][0]
        m0[sl] = (m0[sl] * 3 + 1) % 1001
        cnt = seg["m"][2]
        cnt[sl] = cnt[sl] % 3 + 1
        if flip:
            d2 = seg["d"][D2]
            d2[sl] = np.where(d2[sl] < 2, 1 - d2[sl], d2[sl])
            for c in (D3, D4):
                seg["d"][c][sl] = 999 - seg["d"][c][sl]

    def append(self, s, n):
        seg = self.tab.segments[s]
        first = seg["size"]
        seg["size"] = first + n
        self.sync(s, first, n)

    def add_segment(self, rows):
        """A new segment from a generator stream of its own (beyond reserve_segments: every arena and layout moves)."""
        s = len(self.tab.segments)
        src = build_oracle_table(self.w, 1, self.cap, row_base=s * self.cap, seed=self.seed + 1000 + s).segments[0]
        seg = self.tab.add_segment_arrays(src["d"], src["m"], None, rows)
        restat(self.tab, seg)
        self.dt.sync_batch([(s, 0, rows, rows, self.columns(s), 0)])

    def want(self):
        return vo.scan_aggregate(vo.parse_query(self.tab, self.w.query))

    def check(self, flags, label):
        res = self.dt.query_agg(self.plan(flags))
        compare(res, self.want(), label)
        return res

    def close(self):
        self.dt.close()


def _layouts(h, compressed=None):
    """A projection over the plan's payload columns and predicate planes over its filter columns (the compiled scan reads both)."""
    p = h.plan(0)
    h.dt.pack(h.dt.gather_columns(p), compressed=(not JIT_OFF) if compressed is None else compressed)
    h.dt.predpack(h.dt.filter_columns(p))


def _assert_layouts(res, label):
    assert res.packed, (label, res.flags)
    if not JIT_OFF:
        assert res.jit and res.predpack, (label, res.flags, res.kernel)


HOT = 64 | JIT | PACK                        # the flagship's organisation: compiled scan, predicate planes, projection records


def _race(h, plan, outgrow_at=None, gap_s=0.02):
    """Thread A prepares `plan` (forced placement, a sync in every window); thread B sends single-range batches on row ranges no other
    batch touches until A returns. outgrow_at: the batch with that index also pushes m0 past its stored bits (the projection is dropped
    and rebuilt wider by the next query, which runs inside a window). Returns how many batches B sent."""
    done, errors, sent = threading.Event(), [], [0]
    chunk = 512
    ranges = [(s, f) for f in range(0, h.tab.segments[0]["size"] - chunk, chunk) for s in range(len(h.tab.segments))]

    def writer():
        try:
            for i, (s, f) in enumerate(ranges):
                if done.is_set():
                    return
                h.change(s, f, chunk)
                if i == outgrow_at:
                    h.tab.segments[s]["m"][0][f:f + 8] = 5000 + i      # 13 bits instead of 10: C3's bit-field record still fits 4 bytes
                h.sync(s, f, chunk)
                sent[0] += 1
                time.sleep(gap_s)
        except Exception as e:      # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    def preparer():
        try:
            h.dt.warm(plan)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    tb, ta = threading.Thread(target=writer), threading.Thread(target=preparer)
    tb.start(); ta.start()
    ta.join(); tb.join()
    assert not errors, errors
    return sent[0]


@pytest.mark.parametrize("verdict", ["reject", "keep", "alternate"])
def test_sync_racing_placement(place, verdict):
    """a sync that lands between derived_move and derived_settle is refreshed into the NEW buffers by the measuring
    queries; a rejected candidate must not point the layout back at the old buffer under an applied_epoch that says it is current."""
    h = C3Host(nseg=3, rows=249_000, cap=250_000)
    try:
        _layouts(h)
        plan = h.plan(HOT)
        _assert_layouts(h.check(HOT, "before"), "before")       # (compiles the plan's kernel: the prepare's own rounds are quick)
        place(4, verdict, wait_sync=True)
        sent = _race(h, plan)
        assert sent >= 4
        _assert_layouts(h.check(HOT, f"after a placement ({verdict}) raced by {sent} syncs"), verdict)
        h.dt.relocate(0)
        _assert_layouts(h.check(HOT, "relocated after the race"), "relocate")
        h.dt.narrow(h.dt.filter_columns(plan))
        res = h.check(capi.PLAN_NO_JIT, "narrow copies after the race")
        assert res.narrow and not res.predpack, res.flags
        res = h.check(PACK | capi.PLAN_NO_JIT, "plain projection after the race")      # (the pre-built kernels read plain records only)
        assert res.packed and not res.packed_compressed, res.flags
    finally:
        h.close()


def test_outgrow_inside_a_placement_window(place):
    """A synced m0 outgrows the bit-field projection while a candidate place is being measured: the projection is dropped and rebuilt at
    the same record size — its buffer and its host object may come back at the addresses of the ones just freed. A rejected candidate
    must not install the old narrow-width buffer under the rebuilt layout."""
    h = C3Host(nseg=3, rows=249_000, cap=250_000)
    try:
        _layouts(h)
        plan = h.plan(HOT)
        res = h.check(HOT, "before")
        _assert_layouts(res, "before")
        bits_before = res.pack_bits
        place(4, "reject", wait_sync=True)
        _race(h, plan, outgrow_at=2, gap_s=0.05)
        res = h.check(HOT, "after the outgrowing sync")
        _assert_layouts(res, "after")
        if not JIT_OFF:
            assert bits_before and res.pack_bits and res.pack_rec_bytes == 4, (res.flags, res.pack_rec_bytes)
        h.dt.relocate(1)
        h.change(0, 200_000, 300)
        h.sync(0, 200_000, 300)
        _assert_layouts(h.check(HOT, "sync after relocating the rebuilt projection"), "rebuilt + relocate + sync")
    finally:
        h.close()


@pytest.mark.parametrize("verdict", ["keep", "reject"])
def test_readers_during_placement(place, verdict):
    """No writer: three threads query the plan throughout a forced placement. Every answer equals the oracle's exactly."""
    h = C3Host(nseg=3, rows=249_000, cap=250_000)
    try:
        _layouts(h)
        plan = h.plan(HOT)
        want = h.want()
        _assert_layouts(h.check(HOT, "before"), "before")
        place(6, verdict)
        done, errors, seen = threading.Event(), [], []

        def reader(i):
            try:
                while not done.is_set():
                    res = h.dt.query_agg(plan)
                    compare(res, want, f"reader {i}")
                    _assert_layouts(res, f"reader {i}")
                    seen.append(i)
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        rs = [threading.Thread(target=reader, args=(i,)) for i in range(3)]
        for t in rs:
            t.start()
        try:
            h.dt.warm(plan)
        finally:
            done.set()
            for t in rs:
                t.join()
        assert not errors, errors
        assert len(seen) >= 3
        _assert_layouts(h.check(HOT, "after"), "after")
    finally:
        h.close()


def test_two_prepares_and_a_writer(place):
    """Two prepares of one table at once (each moves what the other may have moved) while a writer syncs: no error, no double free, and
    the answer afterwards is the oracle's."""
    h = C3Host(nseg=3, rows=249_000, cap=250_000)
    try:
        _layouts(h)
        plan = h.plan(HOT)
        _assert_layouts(h.check(HOT, "before"), "before")
        place(4, "alternate")
        done, errors = threading.Event(), []

        def writer():
            try:
                for f in range(0, 240_000, 512):
                    if done.is_set():
                        return
                    s = (f // 512) % 3
                    h.change(s, f, 512)
                    h.sync(s, f, 512)
                    time.sleep(0.005)
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        def preparer():
            try:
                h.dt.warm(plan)
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        tw = threading.Thread(target=writer)
        ps = [threading.Thread(target=preparer) for _ in range(2)]
        tw.start()
        for t in ps:
            t.start()
        for t in ps:
            t.join()
        done.set()
        tw.join()
        assert not errors, errors
        _assert_layouts(h.check(HOT, "after two prepares"), "after")
        h.dt.relocate(0)
        _assert_layouts(h.check(HOT, "after two prepares + relocate"), "relocate")
    finally:
        h.close()


def test_journal_trim(monkeypatch):
    """VH_TEST_JOURNAL_CAP=64: the journal drops its older half when it holds 64 entries. One entry and one epoch per synced item, so with
    the initial load at epochs 1..4 the floor moves to 32 at the 65th entry, to 64 at the 97th. After 100 single-range syncs: the narrow
    copies (refreshed at epoch 4) are behind the floor — whole segments, except segment 3, which no sync touched (whole() skips it); the
    predicate planes were refreshed at epoch 64, exactly the floor (the journal still reaches back to them); the projection was kept current
    by a query every 10 syncs."""
    monkeypatch.setenv("VH_TEST_JOURNAL_CAP", "64")
    h = C3Host(nseg=4, rows=60_000, cap=65_536)
    try:
        assert h.dt.info()[0] == 4
        plan = h.plan(0)
        h.dt.narrow(h.dt.filter_columns(plan))
        _layouts(h)
        r = h.check(HOT, "after the load")
        _assert_layouts(r, "after the load")
        assert h.check(capi.PLAN_NO_JIT, "narrow after the load").narrow
        rng = np.random.default_rng(3)
        epoch = 4
        for i in range(100):
            s, n = int(rng.integers(0, 3)), int(rng.integers(1, 700))
            f = int(rng.integers(0, 60_000 - n))
            h.change(s, f, n)
            h.sync(s, f, n)
            epoch += 1
            if epoch == 64:
                h.dt.predpack(h.dt.filter_columns(plan))                                 # the planes are refreshed exactly at the epoch that becomes the floor
            if i % 10 == 9:
                res = h.dt.query_agg(h.plan(JIT | PACK | capi.PLAN_NO_NARROW))         # keeps the projection current (reads neither planes nor narrow copies)
                compare(res, h.want(), f"projection kept current, sync {i}")
                assert res.packed and not res.predpack and not res.narrow
        assert epoch == 104
        res = h.check(capi.PLAN_NO_JIT, "narrow copies behind the floor")
        assert res.narrow and not res.predpack
        _assert_layouts(h.check(HOT, "planes at the floor, projection current"), "after the trim")
        res = h.check(capi.PLAN_NO_JIT | capi.PLAN_NO_NARROW, "the arenas")
        assert not res.narrow
    finally:
        h.close()


# ----------------------------------------------------------------------------------------------------------------- lifecycle state machine
FLAG_SETS = [JIT | PACK, 64, 0]


def _lifecycle(seed, steps, place):
    rng = np.random.default_rng(seed)
    h = C3Host(nseg=2, rows=24_000, cap=32_768, reserve=2, seed=100 + seed)
    cov = dict(projection=0, planes=0, narrow=0, relocate_sync=0, rebuild=0, grow=0)
    relocated = False          # a relocate since the last sync
    outgrown = set()           # layouts whose stored widths a sync overran since they were last read
    bits = {"m0": 10, "d2": 2}
    try:
        for step in range(steps):
            op = rng.choice(["metrics", "flip", "append", "segment", "outgrow", "pack", "predpack", "narrow", "relocate", "unpack", "warm",
                             "query", "query"], p=[.1, .1, .07, .04, .08, .08, .08, .07, .1, .03, .05, .1, .1])
            nseg = len(h.tab.segments)
            s = int(rng.integers(0, nseg))
            size = h.tab.segments[s]["size"]
            if op in ("metrics", "flip", "outgrow"):
                f = int(rng.integers(0, size - 1))
                n = int(rng.integers(1, min(3000, size - f) + 1))
                h.change(s, f, n, flip=op != "metrics")
                if op == "outgrow":
                    which = rng.choice(["m0", "d2"])
                    bits[which] += 1
                    col = h.tab.segments[s]["m"][0] if which == "m0" else h.tab.segments[s]["d"][D2]
                    col[f] = (1 << (bits[which] - 1)) | 1
                    outgrown.add("projection" if which == "m0" else "planes")
                h.sync(s, f, n, ship_dims=op != "metrics")
                cov["relocate_sync"] += relocated
                relocated = False
            elif op == "append":
                room = h.cap - size
                if room > 0:
                    h.append(s, int(rng.integers(1, min(room, 4000) + 1)))
                    cov["relocate_sync"] += relocated
                    relocated = False
            elif op == "segment":
                if nseg < 6:
                    h.add_segment(int(rng.integers(1000, h.cap + 1)))
                    cov["grow"] += nseg in (2, 4)             # (capacity 2, then 4, then 8 segments)
                    cov["relocate_sync"] += relocated
                    relocated = False
            elif op == "pack":
                form = rng.choice([None, False, True])
                h.dt.pack(h.dt.gather_columns(h.plan(0)), compressed=None if form is None else bool(form))
            elif op == "predpack":
                h.dt.predpack(h.dt.filter_columns(h.plan(0)), sliced=bool(rng.integers(0, 2)))
            elif op == "narrow":
                h.dt.narrow(h.dt.filter_columns(h.plan(0)))
            elif op == "relocate":
                h.dt.relocate(int(rng.integers(0, 3)))
                relocated = True
            elif op == "unpack":
                h.dt.unpack()
            elif op == "warm":
                place(int(rng.integers(1, 4)), str(rng.choice(["keep", "reject", "alternate"])))
                h.dt.warm(h.plan(FLAG_SETS[int(rng.integers(0, len(FLAG_SETS)))]))
            flags = FLAG_SETS[int(rng.integers(0, len(FLAG_SETS)))]
            if op.startswith("query") or op in ("warm", "relocate", "outgrow") or rng.random() < 0.3:
                res = h.check(flags, f"seed {seed} step {step} ({op}) flags {flags}")
                cov["projection"] += res.packed
                cov["planes"] += res.predpack
                cov["narrow"] += res.narrow and not res.predpack
                if "projection" in outgrown and res.packed and res.packed_compressed:
                    cov["rebuild"] += 1
                    outgrown.discard("projection")
                if "planes" in outgrown and res.predpack:
                    cov["rebuild"] += 1
                    outgrown.discard("planes")
        return cov
    finally:
        h.close()


def test_lifecycle_state_machine(place):
    """Seeded random sequences of syncs (in-place metrics, filter values across the literals, appends inside a segment, new segments beyond
    the reserve: table_grow moves every layout), values that outgrow a narrow copy / a compressed or bit-field projection / a predicate
    projection's bits, pack (plain, compressed, bits) / predpack (sliced, byte planes) / narrow / relocate / unpack / a prepare with forced
    placement, and queries under three flag sets — every answer against the oracle. The coverage counts at the end keep it from passing
    vacuously."""
    total = {}
    for seed in range(6):
        for k, v in _lifecycle(seed, 40, place).items():
            total[k] = total.get(k, 0) + v
    need = dict(projection=10, narrow=3, relocate_sync=3, grow=3)
    if not JIT_OFF:                    # (compressed projections and predicate planes are read by the compiled kernels alone)
        need.update(planes=5, rebuild=3)
    assert all(total[k] >= v for k, v in need.items()), total


def test_device_bytes_ledger():
    """vh_table_info's device_bytes is a ledger every derived layout pays into and out of. A table that builds every kind of layout — narrow
    copies, a projection, predicate planes in both forms, the grouped records and clustered planes — relocates them, grows past its reserve
    (every arena moves, the grouped form starts over) and loses its predicate projections to a value that outgrew their bits reports, after
    vh_table_unpack, exactly the bytes of an identical table that took the same syncs and never built a layout. Two segments of 5 000 rows
    with room for 8 192: two full tiles and one of 904 rows. No byte count is written here: the second table is the yardstick throughout."""
    h = C3Host(nseg=2, rows=5000, cap=8192, reserve=2)
    y = C3Host(nseg=2, rows=5000, cap=8192, reserve=2)
    try:
        assert h.dt.info()[2] == y.dt.info()[2]
        cols = h.dt.filter_columns(h.plan(0))
        h.dt.narrow(cols)
        _layouts(h)
        h.dt.predpack(cols, sliced=False)
        h.dt.predpack(cols, sliced=True)
        flags = h.dt.warm(h.plan(HOT))
        if not JIT_OFF:
            assert flags & capi.INFO_GROUPED_PAYLOAD and flags & capi.INFO_GROUPED_PLANES, hex(flags)
        built = h.dt.info()[2]
        assert built > y.dt.info()[2]
        res = h.check(HOT, "every layout built")
        _assert_layouts(res, "every layout built")
        assert JIT_OFF or (res.grouped_payload and res.grouped_planes), hex(res.flags)
        assert h.check(capi.PLAN_NO_JIT, "narrow copies").narrow
        h.dt.relocate(0)
        assert h.dt.info()[2] == built
        _assert_layouts(h.check(HOT, "relocated"), "relocated")
        for t in (h, y):
            t.add_segment(5000)                      # a third segment with room for two: every arena and every layout moves or starts over
        assert h.dt.info()[0] == 3 and h.dt.info()[2] > y.dt.info()[2] > 0
        res = h.check(HOT, "grown")
        _assert_layouts(res, "grown")
        assert JIT_OFF or (res.grouped_payload and res.grouped_planes), hex(res.flags)
        assert h.check(capi.PLAN_NO_JIT, "narrow copies, grown").narrow
        d = h.tab.segments[0]["d"]
        row = int(np.flatnonzero((d[D2][:5000] == 1) & (d[D3][:5000] < 447) & (d[D4][:5000] >= 553))[0])
        for t in (h, y):
            t.tab.segments[0]["d"][D2][row] = 4      # d2 held 0..3 in 2 bits: both predicate projections and the clustered planes are void
            t.sync(0, row, 1)
        res = h.check(HOT, "d2 outgrew the planes")
        assert res.packed and not res.predpack and not res.grouped_planes, hex(res.flags)
        assert h.dt.info()[2] > y.dt.info()[2]
        h.dt.unpack()
        assert h.dt.info()[2] == y.dt.info()[2]
        res = h.check(HOT & ~PACK, "no layout left")
        assert not res.packed and not res.predpack and not res.narrow, hex(res.flags)
    finally:
        h.close()
        y.close()
