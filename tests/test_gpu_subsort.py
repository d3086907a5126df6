"""The sub-sorted grouped form (viyadb_amd/csrc/vh_grouped.h): every 2048-row tile ordered by (d2, the d3 field, row), 64 boundary keys per
tile, and the compiled scan trimming every run of `d2 == literal` to the words that can pass the one range leaf on d3. Tables as in
tests/test_gpu_gplanes.py — 3 segments of 5 000 mirrored rows with room for 8 192 — far below the size at which the form is sub-sorted by
itself, so VH_TEST_SUBSORT=1 forces it. Every answer is compared with the oracle over the host's current arrays, bit for bit with its
VH_PLAN_NO_GROUPED twin (row-order planes, ungrouped records), and `sub_trimmed` (vh_result_info.reserved bit 28) must be set exactly where
the planner's rule says."""
import numpy as np
import pytest

from tests.conftest import JIT_OFF
from tests.cluster_shapes import ask, twins
from tests.test_gpu_gplanes import C3, D3_LT, D4_GE, EQ, HOT, REL, ROWS, CAP, TILE, same_bits
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3
from viyadb_amd import capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="a sub-sorted form is read by the compiled scan only")]
FIELD_MAX = 1023          # d3 holds 0 .. 999: a field of 10 bits
OPS = {"lt": capi.OP_LT, "le": capi.OP_LE, "gt": capi.OP_GT, "ge": capi.OP_GE, "eq": capi.OP_EQ}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("VH_TEST_SUBSORT", "1")
    h = C3Host(3, ROWS, CAP)
    yield h
    h.close()


def warm(h, trim=True):
    flags = h.dt.warm(h.plan(HOT))
    assert flags & capi.INFO_GROUPED_PAYLOAD and flags & capi.INFO_GROUPED_PLANES and bool(flags & capi.INFO_SUBTRIM) == trim, hex(flags)
    return flags


def test_c3(host):
    flags = warm(host)
    c = twins(host, C3, label="C3")
    paths = capi.INFO_GROUPED_PAYLOAD | capi.INFO_GROUPED_PLANES | capi.INFO_SUBTRIM
    assert c.passed_recs > 0 and c.flags & paths == flags & paths, (hex(c.flags), hex(flags))       # (warm reports what the next query runs on)
    twins(host, [EQ(D2, 1), D4_GE, D3_LT], label="the d3 leaf last")
    twins(host, [D3_LT, D4_GE, EQ(D2, 1)], label="the d3 leaf first")


@pytest.mark.parametrize("name", sorted(OPS))
def test_every_relation(host, name):
    """Literals 0, 1, the field maximum, a value the data holds and one it does not (446 is moved to 445 first). Every segment gets a few
    rows with d3 = 0 and d3 = 1023, so that both ends of the 10-bit field are keys of the data and no literal is ruled out by the columns'
    recorded ranges before a scan."""
    for s, seg in enumerate(host.tab.segments):
        col = seg["d"][D3]
        col[col == 446] = 445
        ones = np.flatnonzero((seg["d"][D2][:ROWS] == 1) & (seg["d"][4][:ROWS] >= 553))
        col[ones[:6:2]] = 0
        col[ones[1:6:2]] = FIELD_MAX
        col[ones[-1]] = FIELD_MAX       # (in the segment's last tile of 904 rows)
        host.sync(s, 0, ROWS)
    present = int(host.tab.segments[0]["d"][D3][17])
    warm(host)
    passed = {}
    for lit in (0, 1, FIELD_MAX, present, 446):
        passed[lit] = twins(host, [EQ(D2, 1), REL(D3, OPS[name], name, lit), D4_GE], label=f"d3 {name} {lit}").passed_recs
    if name == "eq":
        assert passed[446] == 0 and passed[FIELD_MAX] == 12 and passed[0] >= 9, passed
    if name == "lt":
        assert passed[0] == 0 and passed[1] >= 9, passed
    if name in ("le", "ge"):
        assert passed[present] > 0, passed


def test_planner_rule(host):
    warm(host)
    twins(host, [EQ(D2, 1), D4_GE], label="no d3 leaf", trim=False)
    twins(host, [EQ(D2, 1), D3_LT, REL(D3, capi.OP_GE, "ge", 100), D4_GE], label="two leaves on d3", trim=False)
    twins(host, [EQ(D2, 1), REL(D3, capi.OP_NE, "ne", 447), D4_GE], label="the d3 leaf as NE", trim=False)
    twins(host, [EQ(D2, 1), REL(D3, capi.OP_LT, "lt", 5000), D4_GE], label="a literal beyond the field", trim=False)
    o = ask(host, [EQ(D2, 1), D3_LT, D4_GE], HOT, label="a top-level OR", node="or")
    assert not o.grouped_payload and not o.grouped_planes and not o.sub_trimmed, hex(o.flags)


def test_every_d2_literal(host):
    for s, seg in enumerate(host.tab.segments):
        col = seg["d"][D2]
        col[col == 2] = 3        # the segments' min / max stay 0 and 3: `d2 == 2` is scanned, and every tile's run of 2 is empty
        host.sync(s, 0, ROWS)
    warm(host)
    for v in (0, 1, 3):
        assert twins(host, [EQ(D2, v), D3_LT, D4_GE], label=f"d2 == {v}").passed_recs > 0
    assert twins(host, [EQ(D2, 2), D3_LT, D4_GE], label="a value no row has").passed_recs == 0


def test_a_segment_of_one_value(host):
    host.tab.segments[1]["d"][D2][:] = 1
    host.sync(1, 0, ROWS)
    warm(host)
    twins(host, C3, label="segment 1 holds d2 = 1 alone: runs of 64 words")
    twins(host, [EQ(D2, 0), D3_LT, D4_GE], label="... and no 0")
    twins(host, [EQ(D2, 3), REL(D3, capi.OP_GE, "ge", 447), D4_GE], label="... and no 3, trimmed from the front")


def test_runs_of_31_32_33_places(host):
    """One value's count in a tile set to 31, 32 and 33 through the host arrays and a sync, as tests/test_gpu_gplanes.py does; the runs' d3
    keys are 430, 431, ... — distinct and ascending along the run — so that with literals 429 .. 464 the cut falls on every place of the
    run in turn, the word boundaries the run crosses among them. Every row of the runs passes d4."""
    warm(host)
    rng = np.random.default_rng(7)
    for (s, tile), n in zip(((0, 0), (1, 0), (2, 1)), (31, 32, 33)):
        seg = host.tab.segments[s]
        sl = slice(tile * TILE, (tile + 1) * TILE)
        d2 = seg["d"][D2][sl]
        d2[d2 == 1] = 0
        at = rng.choice(TILE, size=n, replace=False)
        d2[at] = 1
        seg["d"][3][sl][at] = 430 + rng.permutation(n)
        seg["d"][4][sl][at] = 900
        host.sync(s, tile * TILE, TILE)
    snap = [TILE, TILE, 2 * TILE]      # those tiles alone (and segment 2's first)
    first = host.tab.segments[2]["d"]
    for lit in range(429, 465):
        c = twins(host, [EQ(D2, 1), REL(D3, capi.OP_LT, "lt", lit), D4_GE], seg_rows=snap, label=f"runs of 31, 32, 33: d3 < {lit}")
        in_first = int(np.count_nonzero((first[D2][:TILE] == 1) & (first[3][:TILE] < lit) & (first[4][:TILE] >= 553)))
        assert c.passed_recs == sum(min(max(lit - 430, 0), n) for n in (31, 32, 33)) + in_first, (lit, c.passed_recs)
    for name in ("ge", "eq"):
        for lit in (430, 447, 461, 462):
            twins(host, [EQ(D2, 1), REL(D3, OPS[name], name, lit), D4_GE], label=f"runs of 31, 32, 33: d3 {name} {lit}")
    twins(host, [EQ(D2, 0), D3_LT, D4_GE], label="the value that took the rows")


def test_a_sync_moves_keys_across_the_literal(host):
    warm(host)
    before = twins(host, C3, label="before").passed_recs
    host.change(1, 2100, 300)                  # d3 -> 999 - d3 (and d2, d4, the metrics) for 300 rows of segment 1's second tile
    host.sync(1, 2100, 300)
    after = twins(host, C3, label="after rows' d3 crossed the literal in one tile").passed_recs
    assert after != before
    host.append(0, 1500)                       # fills the tile of 904 rows and runs 356 rows into the next
    twins(host, C3, label="after an append across a tile's end")


def test_snapshots_and_the_readers_given_up(host, monkeypatch):
    warm(host)
    twins(host, C3, seg_rows=[2048, 4096, ROWS], label="a snapshot of whole tiles")
    twins(host, C3, seg_rows=[0, ROWS, 0], label="a snapshot of whole segments")
    twins(host, C3, seg_rows=[0, 2048 + 37, ROWS], label="a snapshot that cuts a tile: the ungrouped records", grouped=False)
    g = ask(host, C3, HOT | capi.PLAN_NO_GPLANES, label="VH_PLAN_NO_GPLANES: the ungrouped records")
    assert g.packed and g.sliced and not g.grouped_payload and not g.grouped_planes and not g.sub_trimmed, hex(g.flags)
    c = twins(host, C3, label="trimmed")
    same_bits(c, g, "VH_PLAN_NO_GPLANES against the trimmed scan")
    monkeypatch.setenv("VH_TEST_NO_SUBTRIM", "1")
    u = twins(host, C3, label="VH_TEST_NO_SUBTRIM=1", trim=False)
    same_bits(c, u, "the untrimmed scan of the sub-sorted form against the trimmed one")


def test_the_gate_keeps_small_tables_as_they_were(host, monkeypatch):
    """Without the hook a table of 15 000 rows gets the form it always got: nothing is trimmed, and the records-only reader still has it."""
    monkeypatch.delenv("VH_TEST_SUBSORT")
    warm(host, trim=False)
    twins(host, C3, label="below VH_SUBSORT_MIN_ROWS", trim=False)
    g = ask(host, C3, HOT | capi.PLAN_NO_GPLANES, label="VH_PLAN_NO_GPLANES below the gate")
    assert g.grouped_payload and not g.grouped_planes and not g.sub_trimmed, hex(g.flags)
    monkeypatch.setenv("VH_TEST_SUBSORT", "1")
    warm(host, trim=True)                      # (a prepared plan has the form built again for its sub column)
    twins(host, C3, label="after a prepare under the hook")
    monkeypatch.setenv("VH_TEST_SUBSORT", "0")
    warm(host, trim=False)
    twins(host, C3, label="after a prepare with the sub-sort forced off", trim=False)
