"""The clustered scan at geometries other than C3's (tests/cluster_shapes.py lists them and what each reaches): grouping fields below,
between and above the other fields, at bit 28 of a 32-plane word, of 1 and of 4 bits (a 32-byte tile header); word groups of 4, 20, 28 and
32 dwords with and without padding; sub fields of 1, 7, 10, 11, 15 and 16 bits at offsets 0, 7 and 15; source columns of 1, 2, 4 and 8
bytes, signed ones among them; and the two widths at which the planner's rule stops (a 5-bit equality field, a 17-bit range field).

Every answer is compared with the oracle over the host's current arrays (tests/parity.compare) and the forms — clustered planes, row-order
planes over grouped records, row-order records, the arenas; the sub-sorted form trimmed, untrimmed and against its row-order twin; tile
groups that span segments and those that do not — with each other bit for bit; all states are integers. What ran (grouped_payload,
grouped_planes, sub_trimmed, gp_spanned) must be what the planner's rule says for the shape. A literal the segments' recorded ranges rule
out reaches no scan (scanned_segments is 0, as the oracle's): its forms are compared all the same, and none of those bits may be set.

From 15 % of the rows passing (VH_QPAY_MIN_SEL, by a probe of the data) the planner streams the payload records beside the planes and
reads no grouped form at all; the literals here go up to every row of a run passing, and `one` cannot pass fewer than a quarter, so every
plan of this module carries VH_PLAN_NO_QPAY and stays the gathering scan whose geometry is under test. Below 15 % the flag changes nothing."""
import numpy as np
import pytest

from tests import cluster_shapes
from tests.cluster_shapes import CAP, JIT, PART, ROWS, SHAPES, TILE, ShapeHost, ask, four_forms, same_bits, twins
from tests.conftest import JIT_OFF
from viyadb_amd import capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="clustered planes are read by the compiled scan only")]
KEEP = capi.PLAN_NO_QPAY
HOT = cluster_shapes.HOT | KEEP
PATHS = capi.INFO_GROUPED_PAYLOAD | capi.INFO_GROUPED_PLANES
RELATIONS = ("lt", "le", "gt", "ge", "eq")
# (shape, the column the relations are put on): every sub column of every shape, and seventeen's 17-bit field, which is none
SUB_CASES = [(n, s) for n, sh in SHAPES.items() for s in sh.subs] + [("seventeen", "w")]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture
def make(monkeypatch):
    """ShapeHost(name) with VH_TEST_SUBSORT as asked (None: unset — a table this small is not sub-sorted by itself)."""
    made = []

    def get(name, subsort=None):
        monkeypatch.delenv("VH_TEST_SUBSORT", raising=False)
        monkeypatch.delenv("VH_TEST_NO_SUBTRIM", raising=False)
        monkeypatch.delenv("VH_TEST_NO_GPSPAN", raising=False)
        if subsort is not None:
            monkeypatch.setenv("VH_TEST_SUBSORT", subsort)
        made.append(ShapeHost(name))
        return made[-1]
    yield get
    for h in made:
        h.close()


def warm(h, sub=None, trim=False):
    flags = h.dt.warm(h.plan(HOT, sub))
    want = (PATHS if h.shape.grouped else 0) | (capi.INFO_SUBTRIM if trim else 0)
    assert flags & (PATHS | capi.INFO_SUBTRIM) == want, (h.name, hex(flags))
    return flags


def unscanned(h, c, leaves, label):
    """The recorded ranges ruled the literal out: no scan, compiled or other, read a row — under any of the four forms' flags."""
    assert c.passed_recs == 0 and c.ngroups == 0 and not c.grouped_payload and not c.grouped_planes and not c.sub_trimmed and not c.gp_spanned, (label, hex(c.flags))
    for flags in (HOT | capi.PLAN_NO_GPLANES, HOT | capi.PLAN_NO_GROUPED, PART | JIT | KEEP | capi.PLAN_NO_PACK):
        o = ask(h, leaves, flags, label=label)
        assert o.scanned_segments == 0, (label, hex(flags))
        same_bits(c, o, label)
    return c


def forms(h, leaves, label):
    c = ask(h, leaves, HOT, label=label)
    return four_forms(h, leaves, label=label, grouped=h.shape.grouped, extra=KEEP) if c.scanned_segments else unscanned(h, c, leaves, label)


@pytest.mark.parametrize("name", list(SHAPES))
def test_four_forms(make, name):
    h = make(name)
    warm(h)
    c = forms(h, h.main(), f"{name}: the main filter")
    assert c.scanned_segments == 3 and 0.01 * c.scanned_recs <= c.passed_recs, (c.scanned_segments, c.passed_recs)
    forms(h, h.main()[::-1], f"{name}: the == leaf last")


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_grouping_literal(make, name):
    """Every value of g's field, the first beyond it and — on the signed column — a negative literal and a 64-bit one whose low 32 bits are
    a value of the field. The values the data holds pass rows; the planted absent one is scanned and passes none; the others reach no scan."""
    h = make(name)
    sh = h.shape
    warm(h)
    top = dict((n, t) for n, _, t in sh.cols)["g"]
    field = 1 << sh.bits["g"]
    for v in list(range(field + 1)) + ([-1, (1 << 32) + 1] if name == "signed" else []):
        c = forms(h, h.main(v=v), f"{name}: g == {v}")
        held = 0 <= v <= top and not (sh.absent and v == sh.absent[0])
        assert (c.passed_recs > 0) == held and (c.scanned_segments > 0) == (0 <= v <= top), (v, c.passed_recs, c.scanned_segments)


@pytest.mark.parametrize("rel", RELATIONS)
@pytest.mark.parametrize("name, sub", SUB_CASES)
def test_sub_sorted_and_trimmed(make, monkeypatch, name, sub, rel):
    """Under VH_TEST_SUBSORT=1 a prepare for the plan whose first range leaf is on `sub` builds the form sub-sorted by it (again, where the
    form was another sub column's). The leaf's literals: 0, 1, a value the data holds, one it does not (moved to its neighbour first), the
    field's last value and the first beyond it — trimmed exactly when the literal is a value of the field; seventeen's 17-bit field is no sub
    column, so nothing is ever trimmed there."""
    h = make(name, subsort="1")
    sh = h.shape
    bits, trims = sh.bits[sub], sub in sh.subs
    if len(sh.subs) > 1:          # the form exists for the shape's other sub column first: this prepare builds it again
        warm(h, next(s for s in sh.subs if s != sub), trim=True)
    lits = [0, 1]
    if bits > 1:
        gone = next(l[2] for l in sh.leaves if l[0] == sub) - 1
        for s in range(len(h.tab.segments)):
            col = h.named(s)[sub]
            col[col == gone] = gone - 1
            h.sync(s, 0, ROWS)
        lits += [int(h.named(0)[sub][17]), gone]
    lits += [(1 << bits) - 1, 1 << bits]
    warm(h, sub, trim=trims)
    cases = [(lit, KEEP) for lit in dict.fromkeys(lits)]
    if name == "signed" and rel in ("lt", "gt"):          # a negative literal is no value of the field: `a < -1` passes no row, `a > -1` every one
        cases.append((-1, KEEP | capi.PLAN_NO_LANES))
    passed = {}
    for lit, extra in cases:
        leaves = h.main(sub=sub, leaf=(rel, lit))
        label = f"{name}: {sub} {rel} {lit}"
        c = ask(h, leaves, HOT | extra, label=label)
        if not c.scanned_segments:
            unscanned(h, c, leaves, label)
        else:
            c = twins(h, leaves, label=label, trim=trims and 0 <= lit < 1 << bits, extra=extra)
            monkeypatch.setenv("VH_TEST_NO_SUBTRIM", "1")
            u = twins(h, leaves, label=label + ", VH_TEST_NO_SUBTRIM=1", trim=False, extra=extra)
            monkeypatch.delenv("VH_TEST_NO_SUBTRIM")
            assert u.kernel != c.kernel or not c.sub_trimmed, (label, c.kernel)
            same_bits(c, u, label + ": trimmed against untrimmed")
        passed[lit] = c.passed_recs
    others = h.want([h.main()[0]] + [l for l in h.main(sub=sub)[1:] if l[1]["column"] != sub]).passed_recs      # (rows that pass every other leaf)
    last = (1 << bits) - 1
    if rel == "lt":
        assert passed[0] == 0 and (passed[1] >= 9 or not trims) and passed[1 << bits] == others, passed      # (nine planted rows hold the sub field's 0)
    if rel == "eq":
        assert passed[1 << bits] == 0 and (passed[last] >= 12 if trims else True) and (bits == 1 or passed[gone] == 0), passed
    if rel == "ge":
        assert passed[0] == others and passed[1 << bits] == 0, passed
    if rel == "gt" and -1 in passed:
        assert passed[-1] == others, passed
    if rel == "lt" and -1 in passed:
        assert passed[-1] == 0, passed


@pytest.mark.parametrize("name", list(SHAPES))
def test_spanning_groups(make, monkeypatch, name):
    """The main filter with tile groups that span segments and, under VH_TEST_NO_GPSPAN=1, with groups that end with their segment: the same
    bits from two code objects wherever the clustered planes are read, and one code object where they are not."""
    h = make(name)
    warm(h)
    spans = h.shape.grouped
    c = ask(h, h.main(), HOT, label=f"{name}: spanning")
    print(f"{name}: {c.kernel} flags {c.flags:#x} passed {c.passed_recs}")
    assert c.jit and c.grouped_planes == spans and c.gp_spanned == spans and bool(c.flags & capi.INFO_GPSPAN) == spans, (hex(c.flags), c.kernel)
    monkeypatch.setenv("VH_TEST_NO_GPSPAN", "1")
    u = ask(h, h.main(), HOT, label=f"{name}: VH_TEST_NO_GPSPAN=1")
    monkeypatch.delenv("VH_TEST_NO_GPSPAN")
    assert u.jit and u.grouped_planes == spans and not u.gp_spanned, (hex(u.flags), u.kernel)
    assert (c.kernel != u.kernel) == c.gp_spanned, (c.kernel, u.kernel)
    same_bits(c, u, name)
    assert c.ngroups == u.ngroups and c.passed_recs == u.passed_recs > 0


@pytest.mark.parametrize("name", ["middle", "top"])
def test_after_a_sync(make, name):
    h = make(name)
    warm(h)
    before = forms(h, h.main(), f"{name}: before").passed_recs
    h.regenerate(1, TILE + 52, 300, np.random.default_rng(11))          # segment 1 held g == v alone: most of these rows leave the run
    h.sync(1, TILE + 52, 300)
    after = forms(h, h.main(), f"{name}: after 300 rows of one tile were drawn again").passed_recs
    assert after != before
    h.append(0, 1500)                          # fills the tile of 904 rows and runs 356 rows into the next
    assert h.tab.segments[0]["size"] == ROWS + 1500 <= CAP
    grown = forms(h, h.main(), f"{name}: after an append across a tile's end").passed_recs
    assert grown > after
    forms(h, h.main(v=h.shape.absent[1]), f"{name}: ... the value that took the absent one's rows")
