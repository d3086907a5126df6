"""The derived layouts' byte budget (vh_table_set_layout_budget): LRU eviction, pins, the listing (vh_table_layouts), drop by serial.

Tables are C3-shaped: 2 segments of 5 000 rows with room for 8 192 each — two full 2 048-row tiles and one of 904 rows. The query shapes
share C3's filter and differ in their payload columns, none a subset of another, so every shape wants a projection of its own; the library
builds them unasked on the third sighting (VH_AUTO_PACK's default). No byte count is written here: a second, identical table with no
budget (the module's yardstick) builds every shape once, its listing gives every projection's size, and budgets are sums of those.
Every answer is compared with the oracle over the host's current arrays."""
import ctypes as C
import threading

import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4, HOT as HOT_FLAGS
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

pytestmark = pytest.mark.gpu
ROWS, CAP = 5000, 8192
NN = capi.PLAN_NO_NARROW          # the cycles are about projections: no narrow copy joins the budget unasked
DIM = {"d0": (0, 1000), "d1": (1, 100)}
MET = {"m0": 7, "m1": 8, "count": 9, "m4": 11}
PROJ, PBYTES, PSLICED, NARROW = capi.LAYOUT_PROJECTION, capi.LAYOUT_PRED_BYTES, capi.LAYOUT_PRED_SLICED, capi.LAYOUT_NARROW


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


class Shape:
    """C3's filter over other payload columns: GROUP BY `dims`, the metrics `mets`."""

    def __init__(self, dims, mets, filter=None, where=None):
        self.dims, self.mets = tuple(dims), tuple(mets)
        self.filter, self.where = filter, where            # another filter: the plan's nodes and the query's tree
        self.name = "+".join(self.dims + self.mets) + ("" if filter is None else "|" + repr(filter))
        self.cols = tuple(sorted([DIM[d][0] for d in dims] + [MET[m] for m in mets]))

    def plan(self, h, flags=NN):
        hint = 1
        for d in self.dims:
            hint *= DIM[d][1]
        return AggPlan(filter=self.filter or h.w.plan.filter, groups=[GroupSpec(DIM[d][0]) for d in self.dims], metrics=[MET[m] for m in self.mets],
                       flags=flags, groups_hint=hint)

    def query(self, h):
        q = dict(h.w.query)
        q["dimensions"], q["metrics"] = list(self.dims), list(self.mets)
        if self.where is not None:
            q["filter"] = self.where
        return q


HOT = Shape(("d0", "d1"), ("m0", "count"))          # C3 itself
# eight more; with HOT an antichain under inclusion (a projection that covers a plan's columns would be taken for it)
OTHERS = [Shape(("d0", "d1"), ("m0", "m1")), Shape(("d0", "d1"), ("m1", "count")), Shape(("d0", "d1"), ("count", "m4")), Shape(("d0", "d1"), ("m0", "m4")),
          Shape(("d0",), ("m0", "m1", "count")), Shape(("d1",), ("m0", "m1", "m4")), Shape(("d0",), ("m1", "count", "m4")), Shape(("d1",), ("m0", "count", "m4"))]
_WANT = {}


def host(**kw):
    return C3Host(nseg=2, rows=ROWS, cap=CAP, reserve=kw.pop("reserve", 2), **kw)


def want(h, shape, fresh=False):
    """The oracle's answer (every table of this module holds the same rows until a test changes them: fresh=True then)."""
    if fresh:
        return vo.scan_aggregate(vo.parse_query(h.tab, shape.query(h)))
    if shape.name not in _WANT:
        _WANT[shape.name] = vo.scan_aggregate(vo.parse_query(h.tab, shape.query(h)))
    return _WANT[shape.name]


def ask(h, shape, flags=NN, fresh=False, label="", st=None):
    res = h.dt.query_agg(shape.plan(h, flags))
    compare(res, st if st is not None else want(h, shape, fresh), f"{shape.name} {label}")
    return res


def listing(h):
    lay, summ = h.dt.layouts()
    assert [x.serial for x in lay] == sorted(x.serial for x in lay)
    assert sum(x.bytes for x in lay) == summ.bytes
    assert sum(x.bytes for x in lay if x.flags & capi.LAYOUT_PINNED) == summ.pinned_bytes
    return lay, summ


def cols_of(x):
    return tuple(sorted(x.cols[:x.ncols]))


def find(lay, shape, kind=PROJ):
    hit = [x for x in lay if x.kind == kind and cols_of(x) == shape.cols]
    assert len(hit) <= 1, shape.name
    return hit[0] if hit else None


def raw(lay):
    return [C.string_at(C.addressof(x), C.sizeof(x)) for x in lay]


@pytest.fixture(scope="module")
def yard():
    """The yardstick: an identical table with no budget on which every shape was queried to its build. sizes: shape name -> bytes of its
    projection; base: device_bytes of the table before any layout."""
    y = host()
    base = y.dt.info()[2]
    for s in [HOT] + OTHERS:
        seen = [ask(y, s, label="yardstick").packed for _ in range(3)]
        assert seen == [False, False, True], (s.name, seen)
    lay, summ = listing(y)
    assert summ.budget == 0 and summ.evictions == 0 and summ.declined == 0 and len(lay) == 9
    sizes = {s.name: find(lay, s).bytes for s in [HOT] + OTHERS}
    assert summ.bytes == y.dt.info()[2] - base
    y.dt.unpack()
    assert y.dt.info()[2] == base
    yield {"sizes": sizes, "base": base}
    y.close()


class Model:
    """What the budget should do to a table on which only projections are built unasked, kept beside the library: sightings per shape, the
    layouts with their last use, the victims of every build."""

    def __init__(self, sizes, budget):
        self.sizes, self.budget = sizes, budget
        self.tick, self.seen, self.lay = 0, {}, {}          # lay: shape name -> [serial, last_use, pinned]
        self.evictions = self.declined = 0
        self.pending = None                                  # background: the shape whose job is queued

    def bytes(self):
        return sum(self.sizes[n] for n in self.lay)

    def query(self, name, background=False):
        """-> (packed, evicted names) of a query of the shape. background: the third sighting queues a job (worker() runs it)."""
        self.tick += 1
        if name in self.lay:
            self.lay[name][1] = self.tick
            return True, []
        self.seen[name] = self.seen.get(name, 0) + 1
        if self.seen[name] < 3:
            return False, []
        if background:
            self.pending = name
            return False, []
        return self.build(name, self.tick)

    def worker(self):
        """The queued job: the budget is asked at its step (a), the layout is published unread, the asking plan runs once more (a tick, no stamp)."""
        name, self.pending = self.pending, None
        built, victims = self.build(name, 0)
        self.tick += 1
        return built, victims

    def build(self, name, last_use):
        victims = []
        if self.budget:
            deficit = self.bytes() + self.sizes[name] - self.budget
            order = sorted((n for n in self.lay if not self.lay[n][2]), key=lambda n: (self.lay[n][1], self.lay[n][0]))
            if deficit > sum(self.sizes[n] for n in order):
                self.declined += 1
                self.seen[name] = 0
                return False, []
            while deficit > 0:
                v = order.pop(0)
                deficit -= self.sizes[v]
                victims.append(v)
        for v in victims:
            del self.lay[v]
            self.seen.pop(v, None)
            self.evictions += 1
        self.lay[name] = [None, last_use, False]             # (the serial is learnt from the listing)
        return True, victims


def step(h, m, shape, label="", background=False):
    """One query of `shape` on the table and on the model; the listing must be the model's afterwards. background: a job the query queued
    is waited for (vh_table_build_wait) before the listing is read: the worker's choice of victims is the model's too."""
    packed, victims = m.query(shape.name, background)
    res = ask(h, shape, label=label)
    assert res.packed == packed, (shape.name, label, res.packed, packed, hex(res.flags))
    assert bool(res.flags & capi.INFO_EVICTED) == bool(victims), (shape.name, label, hex(res.flags), victims)
    if background and m.pending:
        assert res.flags & capi.INFO_BUILD_PENDING, hex(res.flags)
        lay, summ = listing(h)
        assert summ.bytes + summ.reserved_bytes <= summ.budget
        h.dt.build_wait()
        m.worker()
    lay, summ = listing(h)
    assert summ.bytes + summ.reserved_bytes <= summ.budget or not summ.budget, (summ.bytes, summ.reserved_bytes, summ.budget)
    known = {v[0] for v in m.lay.values() if v[0] is not None}
    new = [x for x in lay if x.serial not in known]
    if m.lay.get(shape.name, [0])[0] is None:
        assert len(new) == 1 and new[0].kind == PROJ and cols_of(new[0]) == shape.cols, (shape.name, [(x.serial, cols_of(x)) for x in new])
        assert new[0].serial > max(known, default=0) and new[0].bytes == m.sizes[shape.name]
        m.lay[shape.name][0] = new[0].serial
    assert {x.serial for x in lay} == {v[0] for v in m.lay.values()}, (label, [(x.serial, cols_of(x)) for x in lay], m.lay)
    for x in lay:
        name = [n for n, v in m.lay.items() if v[0] == x.serial][0]
        assert x.last_use == m.lay[name][1] and bool(x.flags & capi.LAYOUT_PINNED) == m.lay[name][2], (name, x.last_use, m.lay[name])
    assert (summ.evictions, summ.declined, summ.tick) == (m.evictions, m.declined, m.tick), (summ.evictions, summ.declined, summ.tick, m.evictions, m.declined, m.tick)
    return res


# ------------------------------------------------------------------------------------------------------------------------------------ 1
def test_listing(yard):
    """No budget. Three sightings of C3 build narrow copies of its filter columns and a plain projection unasked; under the compiled scan
    the same sightings build a compressed projection and the bit-sliced predicate planes, and a plan that streams its payload the byte
    planes. The listing names each with kind, columns, `automatic` and no pin, their bytes add up to what the ledger gained over the
    yardstick, uses / last_use advance by exactly the queries that read them, and cap = 0 / cap < n behave as the header says."""
    h = host()
    try:
        assert h.dt.info()[2] == yard["base"]
        lay, summ = listing(h)
        assert lay == [] and (summ.budget, summ.bytes, summ.tick) == (0, 0, 0)
        seen = [ask(h, HOT, flags=0, label="listing") for _ in range(3)]
        assert [r.packed for r in seen] == [False, False, True] and seen[2].narrow
        lay, summ = listing(h)
        assert summ.tick == 3 and summ.evictions == 0 and summ.declined == 0 and summ.reserved_bytes == 0 and summ.pinned_bytes == 0
        nar = sorted(x.cols[0] for x in lay if x.kind == NARROW)
        assert nar == [D2, D3, D4] and all(x.ncols == 1 for x in lay if x.kind == NARROW), [(x.kind, cols_of(x)) for x in lay]
        pk = find(lay, HOT)
        assert pk is not None and len(lay) == 4 and pk.ncols == 4 and pk.bytes == yard["sizes"][HOT.name] and pk.grouped_bytes == 0
        for x in lay:
            assert x.flags & capi.LAYOUT_AUTOMATIC and not x.flags & capi.LAYOUT_PINNED and x.flags & capi.LAYOUT_CURRENT, (x.kind, x.flags)
            assert x.uses == 1 and x.last_use == 3, (x.kind, x.uses, x.last_use)      # the query that built them read them
        assert not pk.flags & (capi.LAYOUT_COMPRESSED | capi.LAYOUT_BITS | capi.LAYOUT_GROUPED)
        assert sum(x.bytes for x in lay) == h.dt.info()[2] - yard["base"]
        for _ in range(4):
            ask(h, HOT, flags=0, label="further")
        ask(h, HOT, flags=capi.PLAN_NO_PACK, label="the arenas' payload")           # reads the narrow copies alone
        lay2, summ2 = listing(h)
        assert summ2.tick == 8 and [x.serial for x in lay2] == [x.serial for x in lay]
        for x in lay2:
            assert (x.uses, x.last_use) == ((5, 7) if x.kind == PROJ else (6, 8)), (x.kind, x.uses, x.last_use)
        # cap = 0 with n only; cap < n fills cap entries and leaves the rest alone
        n = C.c_uint32()
        capi.check(h.dt.lib.vh_table_layouts(h.dt.handle, None, 0, C.byref(n), None))
        assert n.value == 4
        arr = (capi.LayoutInfo * 4)()
        capi.check(h.dt.lib.vh_table_layouts(h.dt.handle, arr, 2, C.byref(n), None))
        assert n.value == 4 and [a.serial for a in arr] == [lay2[0].serial, lay2[1].serial, 0, 0]
        if not JIT_OFF:
            J = capi.PLAN_FORCE_JIT
            h.dt.drop_layout(pk.serial)           # (the plain records would serve the compiled scan as well: nothing compressed would be built)
            for _ in range(4):          # (the third builds projection and planes; the planes are read from the fourth on)
                res = ask(h, HOT, flags=J, label="compiled")
            assert res.jit and res.packed and res.packed_compressed and res.predpack and res.sliced, hex(res.flags)
            for _ in range(3):
                res = ask(h, HOT, flags=J | capi.PLAN_FORCE_QPAY, label="streamed payload")
            lay3, _ = listing(h)
            kinds = sorted(x.kind for x in lay3)
            assert kinds == [PROJ, PBYTES, PSLICED, NARROW, NARROW, NARROW], kinds
            for x in lay3:
                if x.kind in (PBYTES, PSLICED):
                    assert cols_of(x) == (D2, D3, D4) and x.flags & capi.LAYOUT_AUTOMATIC and not x.flags & capi.LAYOUT_PINNED, (x.kind, x.flags)
            comp = [x for x in lay3 if x.kind == PROJ and x.flags & capi.LAYOUT_COMPRESSED]
            assert len(comp) == 1 and cols_of(comp[0]) == HOT.cols and comp[0].flags & capi.LAYOUT_BITS and comp[0].bytes >= comp[0].grouped_bytes
            assert sum(x.bytes for x in lay3) == h.dt.info()[2] - yard["base"]
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"] and listing(h)[0] == []
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 2
def _cycle(h, m, label):
    for s in OTHERS:
        for k in range(3):
            step(h, m, s, f"{label}: sighting {k + 1}")
            res = step(h, m, HOT, f"{label}: hot between")
            assert res.packed


def test_cycle(yard):
    """A budget of the two largest projections, eight shapes queried to their build with the hot shape between every two queries: the
    listing follows the LRU model query by query, the hot shape keeps its serial and its projection, INFO_EVICTED is set on exactly the
    queries whose build evicted, and an evicted shape comes back on its third NEW sighting only, under a new serial."""
    big = sorted(yard["sizes"].values())[-2:]
    h = host()
    try:
        h.dt.set_layout_budget(sum(big))
        m = Model(yard["sizes"], sum(big))
        for _ in range(3):
            step(h, m, HOT, "hot to its build")
        hot_serial = m.lay[HOT.name][0]
        _cycle(h, m, "cycle")
        assert m.lay[HOT.name][0] == hot_serial and m.evictions > 0 and m.declined == 0
        lay, summ = listing(h)
        assert summ.evictions == m.evictions and summ.evicted_bytes > 0
        gone = OTHERS[0]
        assert gone.name not in m.lay and m.seen.get(gone.name, 0) == 0
        before = {x.serial for x in lay}
        seen = [step(h, m, gone, f"evicted shape, new sighting {k + 1}").packed for k in range(3)]
        assert seen == [False, False, True]
        assert m.lay[gone.name][0] not in before and m.lay[gone.name][0] > max(before)
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 3
def test_pins(yard):
    """An explicit projection and one that vh_table_prepare built, under a budget smaller than their sum: both stay through the cycle,
    every automatic build is declined and evicts nothing; unpinned, the prepared one is the next victim."""
    a, b = OTHERS[0], HOT
    h = host()
    try:
        h.dt.pack(list(a.cols), compressed=False)
        h.dt.warm(b.plan(h))
        lay, summ = listing(h)
        la, lb = find(lay, a), find(lay, b)
        assert len(lay) == 2 and la.flags & capi.LAYOUT_PINNED and not la.flags & capi.LAYOUT_AUTOMATIC
        assert lb.flags & capi.LAYOUT_PINNED and lb.flags & capi.LAYOUT_AUTOMATIC
        assert (la.bytes, lb.bytes) == (yard["sizes"][a.name], yard["sizes"][b.name]) and summ.pinned_bytes == la.bytes + lb.bytes
        h.dt.set_layout_budget(la.bytes + lb.bytes - 1)
        assert raw(listing(h)[0]) == raw(lay)                      # pinned layouts stay, over the budget as they are
        declined = 0
        for s in OTHERS[1:]:
            for k in range(3):
                res = ask(h, s, label="declined")
                assert not res.packed and not res.flags & capi.INFO_EVICTED
                assert ask(h, a, label="pinned, explicit").packed and ask(h, b, label="pinned by prepare").packed
            declined += 1
            now, summ = listing(h)
            assert (summ.declined, summ.evictions) == (declined, 0)
            assert [(x.serial, x.bytes, x.flags) for x in now] == [(x.serial, x.bytes, x.flags) for x in lay]
        h.dt.pin_layout(lb.serial, False)
        small = [s for s in OTHERS[1:] if yard["sizes"][s.name] < lb.bytes]
        res = ask(h, small[0], label="after the unpin")             # the table is over its budget and something may leave now
        assert res.flags & capi.INFO_EVICTED and not res.packed
        now, summ = listing(h)
        assert [x.serial for x in now] == [la.serial] and summ.evictions == 1 and summ.evicted_bytes == lb.bytes
        seen = [ask(h, small[0], label="room now").packed for _ in range(3)]
        assert seen[-1] and len(listing(h)[0]) == 2
        with pytest.raises(capi.VhError):
            h.dt.pin_layout(lb.serial, True)                        # it is gone
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 4
def test_infeasible(yard):
    """A shape whose projection is larger than everything evictable together: declined, and the listing is byte for byte what it was."""
    sizes = yard["sizes"]
    small = [s for s in OTHERS if sizes[s.name] < sizes[HOT.name]]
    large = [s for s in OTHERS if sizes[s.name] == sizes[HOT.name]]
    assert small and large
    h = host()
    try:
        h.dt.pack(list(HOT.cols), compressed=False)                 # pinned
        h.dt.set_layout_budget(sizes[HOT.name] + sizes[small[0].name] + 1)
        assert [ask(h, small[0], label="fits").packed for _ in range(3)] == [False, False, True]
        lay, summ = listing(h)
        assert len(lay) == 2 and (summ.declined, summ.evictions) == (0, 0)
        for k in range(3):
            res = ask(h, large[0], label="infeasible")
            assert not res.packed and not res.flags & capi.INFO_EVICTED
        now, summ = listing(h)
        assert raw(now) == raw(lay) and (summ.declined, summ.evictions, summ.evicted_bytes) == (1, 0, 0)
        assert ask(h, small[0], label="still there").packed
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 5
def test_lowering(yard):
    """vh_table_set_layout_budget evicts inside the call, least recently used first; down to 1 byte exactly the pinned layouts are left;
    back to 0 everything is built again without limit."""
    h = host()
    try:
        h.dt.pack(list(HOT.cols), compressed=False)
        three = OTHERS[:3]
        for s in three:
            assert [ask(h, s, label="unlimited").packed for _ in range(3)] == [False, False, True]
        ask(h, three[0], label="the first is the most recent now")
        lay, _ = listing(h)
        hot, l0, l1, l2 = find(lay, HOT), find(lay, three[0]), find(lay, three[1]), find(lay, three[2])
        assert l1.last_use < l2.last_use < l0.last_use
        h.dt.set_layout_budget(hot.bytes + l0.bytes + l2.bytes)
        now, summ = listing(h)
        assert [x.serial for x in now] == sorted([hot.serial, l0.serial, l2.serial]) and (summ.evictions, summ.evicted_bytes) == (1, l1.bytes)
        h.dt.set_layout_budget(hot.bytes + l0.bytes)
        now, summ = listing(h)
        assert [x.serial for x in now] == sorted([hot.serial, l0.serial]) and summ.evictions == 2
        h.dt.set_layout_budget(1)
        now, summ = listing(h)
        assert [x.serial for x in now] == [hot.serial] and summ.evictions == 3 and summ.bytes == summ.pinned_bytes == hot.bytes > summ.budget
        assert not ask(h, three[0], label="no room").packed and ask(h, HOT, label="pinned").packed
        h.dt.set_layout_budget(0)
        for s in OTHERS:
            assert [ask(h, s, label="unlimited again").packed for _ in range(3)][-1]
        now, summ = listing(h)
        assert len(now) == 9 and summ.budget == 0 and summ.evictions == 3
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 6
def test_drop_by_serial(yard):
    """vh_table_layout_drop: an unknown serial is VH_E_INVALID; a pinned layout goes all the same, the next queries answer from the arenas
    and three sightings build it again."""
    h = host()
    try:
        with pytest.raises(capi.VhError) as e:
            h.dt.drop_layout(1)
        assert e.value.code == -1
        h.dt.pack(list(HOT.cols), compressed=False)
        lay, _ = listing(h)
        assert len(lay) == 1 and lay[0].flags & capi.LAYOUT_PINNED and ask(h, HOT, label="explicit").packed
        with pytest.raises(capi.VhError):
            h.dt.drop_layout(lay[0].serial + 1)
        h.dt.drop_layout(lay[0].serial)
        now, summ = listing(h)
        assert now == [] and summ.evictions == 0 and h.dt.info()[2] == yard["base"]
        assert [ask(h, HOT, label="dropped").packed for _ in range(3)] == [False, False, True]
        now, _ = listing(h)
        assert len(now) == 1 and now[0].serial > lay[0].serial and now[0].flags & capi.LAYOUT_AUTOMATIC and not now[0].flags & capi.LAYOUT_PINNED
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 7
def test_readers_during_eviction(yard):
    """A budget that fits one of two shapes; four threads alternate between them, so every build of one evicts the other while other
    threads' queries may still be reading it. Every answer is the oracle's; after vh_table_unpack the ledger is the yardstick's."""
    a, b = HOT, OTHERS[0]
    assert yard["sizes"][a.name] == yard["sizes"][b.name]
    wants = {s.name: want(None, s) for s in (a, b)}
    h = host()
    try:
        h.dt.set_layout_budget(yard["sizes"][a.name])
        plans = {s.name: s.plan(h) for s in (a, b)}
        errors, packed = [], [0]

        def reader(i):
            try:
                for k in range(30):
                    s = (a, b)[(i + k) % 2]
                    res = h.dt.query_agg(plans[s.name])
                    compare(res, wants[s.name], f"thread {i} query {k} {s.name}")
                    packed[0] += res.packed
            except Exception as e:      # noqa: BLE001 (reported by the main thread)
                errors.append(e)

        ts = [threading.Thread(target=reader, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        lay, summ = listing(h)
        assert summ.evictions > 0 and packed[0] > 0 and summ.bytes <= summ.budget and len(lay) <= 1, (summ.evictions, packed[0], len(lay))
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 8
def test_background_mode(yard, monkeypatch):
    """The cycle of test_cycle on a VH_BUILD_BACKGROUND table, vh_table_build_wait after each third sighting: the worker asks the budget
    at its step (a) and its victims are the LRU model's, serial by serial; no query reports an eviction of its own. Then a job is held
    between build and publish: the listing shows the coming layout's bytes as reserved, within the budget; released, the layout is listed."""
    big = sorted(yard["sizes"].values())[-2:]
    h = host()
    try:
        h.dt.set_build_mode(True)
        h.dt.set_layout_budget(sum(big))
        m = Model(yard["sizes"], sum(big))
        for _ in range(3):
            step(h, m, HOT, "hot to its build", background=True)
        hot_serial = m.lay[HOT.name][0]
        for s in OTHERS:
            for k in range(3):
                step(h, m, s, f"background sighting {k + 1}", background=True)
                assert step(h, m, HOT, "hot between", background=True).packed
            assert s.name in m.lay and step(h, m, s, "built by the worker", background=True).packed
        assert m.lay[HOT.name][0] == hot_serial and m.evictions > 0
        lay, summ = listing(h)
        held = OTHERS[0]
        assert held.name not in m.lay and find(lay, held) is None
        monkeypatch.setenv("VH_TEST_BUILD_HOLD", "publish")
        for k in range(3):
            assert ask(h, HOT, label="hot before the held job").packed
            ask(h, held, label=f"held sighting {k + 1}")
        for _ in range(20000):                                      # (the job reaches its hold within milliseconds of its third sighting)
            lay, summ = listing(h)
            if summ.reserved_bytes:
                break
        assert summ.reserved_bytes == yard["sizes"][held.name] and find(lay, held) is None
        assert summ.bytes + summ.reserved_bytes <= summ.budget
        assert not ask(h, held, label="held: the arenas answer").packed and ask(h, HOT, label="hot beside the held job").packed
        monkeypatch.delenv("VH_TEST_BUILD_HOLD")
        h.dt.build_wait()
        lay, summ = listing(h)
        assert summ.bytes + summ.reserved_bytes <= summ.budget
        assert summ.reserved_bytes == 0 and find(lay, held).bytes == yard["sizes"][held.name] and find(lay, HOT).serial == hot_serial
        assert ask(h, held, label="released").packed
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        monkeypatch.delenv("VH_TEST_BUILD_HOLD", raising=False)
        h.dt.build_info()
        h.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 9
def test_growth_and_staleness(yard):
    """After evictions the table grows past its reserve — every layout a query reads moves to arenas twice the size — and the budget, taken
    from a yardstick that grew the same way, still holds after every query. Under the compiled scan a synced value then outgrows the
    field of a pinned compressed projection: its rebuild is pinned again. After vh_table_unpack the ledger is the grown yardstick's."""
    y = host()
    try:
        y.add_segment(ROWS)                                         # a third segment with room for two: the arenas double
        grown, wants = {}, {}
        for s in [HOT] + OTHERS[:3]:
            wants[s.name] = want(y, s, fresh=True)
            assert [ask(y, s, st=wants[s.name], label="grown yardstick").packed for _ in range(3)][-1]
            grown[s.name] = find(listing(y)[0], s).bytes
        y.dt.unpack()
        base = y.dt.info()[2]
    finally:
        y.close()
    h = host()
    try:
        budget = sum(sorted(grown.values())[-2:])
        h.dt.set_layout_budget(budget)
        for s in [HOT] + OTHERS[:3]:
            assert [ask(h, s, label="before the growth").packed for _ in range(3)][-1]
        lay, summ = listing(h)
        assert summ.bytes <= budget
        ev = summ.evictions
        h.add_segment(ROWS)
        for s in [HOT] + OTHERS[:3] + [HOT]:
            for k in range(3):
                ask(h, s, st=wants[s.name], label=f"grown {k}")
                lay, summ = listing(h)
                assert summ.bytes + summ.reserved_bytes <= budget, (s.name, k, summ.bytes, budget)
        assert summ.evictions > ev and find(lay, HOT) is not None and find(lay, HOT).bytes == grown[HOT.name]
        if not JIT_OFF:
            h.dt.set_layout_budget(0)
            h.dt.unpack()
            h.dt.pack(list(HOT.cols), compressed=True)
            h.dt.predpack([D2, D3, D4])
            res = ask(h, HOT, flags=HOT_FLAGS, fresh=True, label="compressed, pinned")
            assert res.packed and res.packed_compressed and res.pack_bits
            lay, _ = listing(h)
            pk = find(lay, HOT)
            assert pk.flags & capi.LAYOUT_PINNED and pk.flags & capi.LAYOUT_COMPRESSED
            h.dt.set_layout_budget(sum(x.bytes for x in lay))
            h.tab.segments[0]["m"][0][10:18] = 5000                  # 13 bits instead of 10: the record still fits 4 bytes
            h.sync(0, 10, 8)
            res = ask(h, HOT, flags=HOT_FLAGS, fresh=True, label="m0 outgrew its field")
            assert res.packed and res.packed_compressed
            lay, summ = listing(h)
            pk2 = find(lay, HOT)
            assert pk2.serial > pk.serial and pk2.flags & capi.LAYOUT_PINNED and pk2.flags & capi.LAYOUT_CURRENT
            assert summ.bytes + summ.reserved_bytes <= summ.budget
        h.dt.unpack()
        assert h.dt.info()[2] == base
    finally:
        h.close()


# ----------------------------------------------------------------------------------------------------------------------------------- 10
J = capi.PLAN_FORCE_JIT | capi.PLAN_FORCE_PART
# three shapes over three predicate column sets, one payload: C3 itself (d2, d3, d4: bit-sliced planes, the grouped form and its clustered
# planes), a plan that streams its payload and so reads rows (d3, d4: byte planes), and a third (d1, d3: bit-sliced planes of its own)
BYTES = Shape(HOT.dims, HOT.mets, filter=[("rel", D3, capi.OP_LT, 447), ("rel", D4, capi.OP_GE, 553), ("and", 2)],
              where={"op": "and", "filters": [{"op": "lt", "column": "d3", "value": "447"}, {"op": "ge", "column": "d4", "value": "553"}]})
THIRD = Shape(HOT.dims, HOT.mets, filter=[("rel", 1, capi.OP_LT, 20), ("rel", D3, capi.OP_LT, 447), ("and", 2)],
              where={"op": "and", "filters": [{"op": "lt", "column": "d1", "value": "20"}, {"op": "lt", "column": "d3", "value": "447"}]})
JQ = J | capi.PLAN_FORCE_QPAY


def _compiled(h, yard):
    """Every compiled layout built unasked, no budget: -> (the oracle's answers, the listing)."""
    st = {s.name: want(h, s, fresh=True) for s in (BYTES, THIRD)}
    st[HOT.name] = want(h, HOT)
    flags = [ask(h, HOT, flags=J, label=f"compiled sighting {k + 1}").flags for k in range(6)]
    assert flags[-1] & capi.INFO_GROUPED_PAYLOAD and flags[-1] & capi.INFO_GROUPED_PLANES, [hex(f) for f in flags]
    for k in range(4):
        res = ask(h, BYTES, flags=JQ, st=st[BYTES.name], label=f"streamed payload {k + 1}")
    assert res.predpack and not res.sliced, hex(res.flags)
    for k in range(4):
        res = ask(h, THIRD, flags=J, st=st[THIRD.name], label=f"third predicate set {k + 1}")
    assert res.predpack and res.sliced, hex(res.flags)
    lay, summ = listing(h)
    pk = find(lay, HOT)
    assert pk is not None and pk.flags & capi.LAYOUT_GROUPED and pk.flags & capi.LAYOUT_GPLANES and 0 < pk.grouped_bytes < pk.bytes
    assert sorted(cols_of(x) for x in lay if x.kind == PSLICED) == [(1, D3), (D2, D3, D4)] and [cols_of(x) for x in lay if x.kind == PBYTES] == [(D3, D4)]
    assert {D2, D3, D4} <= {x.cols[0] for x in lay if x.kind == NARROW}
    assert all(x.flags & capi.LAYOUT_AUTOMATIC and not x.flags & capi.LAYOUT_PINNED for x in lay)
    assert summ.bytes == h.dt.info()[2] - yard["base"]
    return st, lay


def _evict_only(h, yard, victim):
    """Everything but `victim` pinned, the budget one byte short of what exists: exactly `victim` leaves, inside the call; the budget is then
    what it was (room for a rebuild of the same size) and every other layout is unpinned again. -> the listing afterwards."""
    lay, summ = listing(h)
    for x in lay:
        h.dt.pin_layout(x.serial, x.serial != victim.serial)
    h.dt.set_layout_budget(summ.bytes - 1)
    now, after = listing(h)
    assert [x.serial for x in now] == [x.serial for x in lay if x.serial != victim.serial]
    assert (after.evictions, after.evicted_bytes) == (summ.evictions + 1, summ.evicted_bytes + victim.bytes)
    assert after.bytes <= summ.bytes - victim.bytes and after.bytes == h.dt.info()[2] - yard["base"]      # (less: what belonged to it elsewhere went too)
    h.dt.set_layout_budget(summ.bytes)
    for x in now:
        h.dt.pin_layout(x.serial, False)
    return listing(h)[0]


@pytest.mark.skipif(JIT_OFF, reason="VH_JIT=off: predicate projections and grouped forms are read by the per-query compiled kernels only")
def test_compiled_planes_evicted(yard):
    """Byte planes and bit-sliced planes built unasked for three predicate column sets, then evicted by the budget one at a time. The byte
    planes come back on the third new sighting only, under a new serial. With the bit-sliced projection of C3's columns go the clustered
    planes paired with it by serial: the next plans read neither, report no INFO_GROUPED_PLANES and answer as the oracle does; three
    sightings rebuild the projection, three more the clustered planes beside the grouped records it had kept (the budget credits the
    form that is replaced)."""
    h = host()
    try:
        st, lay = _compiled(h, yard)
        total = listing(h)[1].bytes
        pb = [x for x in lay if x.kind == PBYTES][0]
        now = _evict_only(h, yard, pb)
        assert not [x for x in now if x.kind == PBYTES]
        seen = []
        for k in range(4):
            res = ask(h, BYTES, flags=JQ, st=st[BYTES.name], label=f"byte planes evicted, sighting {k + 1}")
            seen.append([x.serial for x in listing(h)[0] if x.kind == PBYTES])
        assert seen[0] == seen[1] == [] and len(seen[2]) == 1 and seen[2][0] > max(x.serial for x in lay) and seen[3] == seen[2], seen
        assert res.predpack and not res.sliced and listing(h)[1].bytes == total
        lay, _ = listing(h)
        ps = [x for x in lay if x.kind == PSLICED and cols_of(x) == (D2, D3, D4)][0]
        grouped = find(lay, HOT).grouped_bytes
        now = _evict_only(h, yard, ps)
        pk = find(now, HOT)
        assert pk.flags & capi.LAYOUT_GROUPED and not pk.flags & capi.LAYOUT_GPLANES and 0 < pk.grouped_bytes < grouped
        flags = [ask(h, HOT, flags=J, label=f"planes evicted, sighting {k + 1}") for k in range(6)]
        assert not flags[0].sliced and not flags[1].sliced and not (flags[0].flags | flags[1].flags | flags[2].flags) & capi.INFO_GROUPED_PLANES
        assert flags[3].sliced and flags[5].flags & capi.INFO_GROUPED_PLANES, [hex(f.flags) for f in flags]
        lay, summ = listing(h)
        pk = find(lay, HOT)
        assert pk.flags & capi.LAYOUT_GPLANES and pk.grouped_bytes == grouped and summ.bytes == total <= summ.budget
        assert [x for x in lay if x.kind == PSLICED and cols_of(x) == (D2, D3, D4)][0].serial > ps.serial
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        h.close()


@pytest.mark.skipif(JIT_OFF, reason="VH_JIT=off: predicate projections and grouped forms are read by the per-query compiled kernels only")
def test_compiled_projection_and_narrow_copy_evicted(yard):
    """The budget evicts a projection that carries a grouped form with clustered planes — counted, listed and gone as one — and a narrow
    copy. The projection comes back on the third new sighting, its grouped form and planes on the third sighting of the new pair; the narrow copy on the third
    sighting of a plan that reads it. Every answer is the oracle's, the ledger is exact throughout."""
    h = host()
    try:
        st, lay = _compiled(h, yard)
        total = listing(h)[1].bytes
        pk = find(lay, HOT)
        now = _evict_only(h, yard, pk)
        assert not [x for x in now if x.kind == PROJ]
        res = [ask(h, HOT, flags=J, label=f"projection evicted, sighting {k + 1}") for k in range(6)]
        assert [r.packed for r in res] == [False, False, True, True, True, True]
        # (the new projection meets the bit-sliced planes from its first query on: the pair's third sighting is the fifth query)
        assert not res[3].flags & capi.INFO_GROUPED_PAYLOAD and res[4].flags & capi.INFO_GROUPED_PAYLOAD and res[4].flags & capi.INFO_GROUPED_PLANES
        lay, summ = listing(h)
        pk2 = find(lay, HOT)
        assert pk2.serial > pk.serial and (pk2.bytes, pk2.grouped_bytes) == (pk.bytes, pk.grouped_bytes) and summ.bytes == total <= summ.budget
        nw = [x for x in lay if x.kind == NARROW and x.cols[0] == D2][0]
        now = _evict_only(h, yard, nw)
        assert D2 not in [x.cols[0] for x in now if x.kind == NARROW]
        assert ask(h, HOT, flags=J, label="narrow copy evicted").flags & capi.INFO_GROUPED_PLANES      # (the compiled scan reads the planes)
        seen = []
        for k in range(3):
            ask(h, HOT, flags=capi.PLAN_NO_JIT | capi.PLAN_NO_PACK, label=f"narrow copy evicted, sighting {k + 1}")
            seen.append([x.serial for x in listing(h)[0] if x.kind == NARROW and x.cols[0] == D2])
        assert seen[0] == seen[1] == [] and len(seen[2]) == 1 and seen[2][0] > nw.serial, seen
        assert listing(h)[1].bytes == total
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        h.close()


# ----------------------------------------------------------------------------------------------------------------------------------- 11
def test_placement_beside_evictions(yard, monkeypatch):
    """vh_table_prepare tries two other places for its layouts (forced, alternating verdicts) while a second thread cycles two shapes
    under a budget that fits one: whatever the prepare's layouts meet, it succeeds or fails cleanly, every answer is the oracle's and
    the ledger is exact after vh_table_unpack."""
    monkeypatch.setenv("VH_TEST_PLACE_CANDIDATES", "2")
    monkeypatch.setenv("VH_TEST_PLACE_VERDICT", "alternate")
    a, b = OTHERS[0], OTHERS[1]
    wants = {s.name: want(None, s) for s in (a, b, HOT)}
    h = host()
    try:
        h.dt.set_layout_budget(yard["sizes"][a.name])
        errors, done = [], threading.Event()

        def cycler():
            try:
                k = 0
                while not done.is_set() or k < 12:
                    s = (a, b)[(k // 3) % 2]
                    compare(h.dt.query_agg(s.plan(h)), wants[s.name], f"cycler {k}")
                    k += 1
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        t = threading.Thread(target=cycler)
        t.start()
        try:
            prepared = None
            try:
                prepared = h.dt.warm(HOT.plan(h))
            except capi.VhError as e:
                assert e.code != 0 and str(e)
        finally:
            done.set()
            t.join()
        assert not errors, errors
        compare(h.dt.query_agg(HOT.plan(h)), wants[HOT.name], "after the prepare")
        lay, summ = listing(h)
        if prepared is not None:       # (the prepare pins as its queries stamp: nothing the cycler does evicts what it read last)
            assert find(lay, HOT) is not None and find(lay, HOT).flags & capi.LAYOUT_PINNED
        h.dt.unpack()
        assert h.dt.info()[2] == yard["base"]
    finally:
        h.close()
