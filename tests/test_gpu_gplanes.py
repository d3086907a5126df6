"""Clustered predicate planes (viyadb_amd/csrc/vh_grouped.h): beside the grouped payload records, the other predicate columns' bits of every
2048-row tile kept in the tile's grouped order, word-major, so that the compiled scan for `d2 == literal` reads only the words of the
literal's run of every tile — and no plane of d2. Tables: 3 segments of 5 000 mirrored rows (two full tiles and one of 904) with room for
8 192. Every answer is compared with the oracle over the host's current arrays (tests/parity.compare); the four forms — clustered planes,
row-order planes over grouped records (VH_PLAN_NO_GPLANES), row-order records (VH_PLAN_NO_GROUPED), the arenas (VH_PLAN_NO_PACK) — must
agree bit for bit; and `grouped_planes` (vh_result_info.reserved bit 21) must be set exactly where the planner's rule says."""
import numpy as np
import pytest

from tests.conftest import JIT_OFF
from tests.cluster_shapes import ask, four_forms, same_bits          # noqa: F401 (other modules take them from here)
from tests.test_gpu_layout_lifecycle import C3Host, D2
from viyadb_amd import capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="clustered planes are read by the compiled scan only")]
PART, JIT, PACK = 64, capi.PLAN_FORCE_JIT, capi.PLAN_FORCE_PACK
HOT = PART | JIT | PACK
ROWS, CAP, TILE = 5000, 8192, 2048


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def EQ(col, v):
    return ("rel", col, capi.OP_EQ, v), {"op": "eq", "column": f"d{col}", "value": str(v)}


def REL(col, op, name, v):
    return ("rel", col, op, v), {"op": name, "column": f"d{col}", "value": str(v)}


D3_LT, D4_GE = REL(3, capi.OP_LT, "lt", 447), REL(4, capi.OP_GE, "ge", 553)
C3 = [EQ(D2, 1), D3_LT, D4_GE]


@pytest.fixture
def host():
    h = C3Host(3, ROWS, CAP)
    yield h
    h.close()


def warm(h):
    """vh_table_prepare of the C3 plan: projection, bit-sliced planes, grouped records and — in the same launch — the clustered planes."""
    flags = h.dt.warm(h.plan(HOT))
    assert flags & capi.INFO_GROUPED_PAYLOAD and flags & capi.INFO_GROUPED_PLANES, hex(flags)


def test_every_literal(host):
    warm(host)
    assert four_forms(host, C3, label="C3").passed_recs > 0
    for v in (0, 2, 3):          # (3 is the field's last value: its run ends with the tile's valid rows — 904 of them in every segment's last tile)
        assert four_forms(host, [EQ(D2, v), D3_LT, D4_GE], label=f"d2 == {v}").passed_recs > 0
    four_forms(host, [D4_GE, EQ(D2, 1)], label="the == leaf last; the filter reads d4 alone beside d2")


def test_a_value_no_row_has(host):
    for s, seg in enumerate(host.tab.segments):
        col = seg["d"][D2]
        col[col == 2] = 3        # the segments' min / max stay 0 and 3: `d2 == 2` is scanned, and every tile's run of 2 is empty
        host.sync(s, 0, ROWS)
    warm(host)
    assert four_forms(host, [EQ(D2, 2), D3_LT, D4_GE], label="a value no row has").passed_recs == 0
    assert four_forms(host, [EQ(D2, 3), D3_LT, D4_GE], label="the value that took the rows").passed_recs > 0
    assert four_forms(host, C3, label="the value before the empty run").passed_recs > 0


def test_a_segment_of_one_value(host):
    host.tab.segments[1]["d"][D2][:] = 1
    host.sync(1, 0, ROWS)
    warm(host)
    four_forms(host, C3, label="segment 1 holds d2 = 1 alone: runs of 64 words")
    four_forms(host, [EQ(D2, 0), D3_LT, D4_GE], label="... and no 0")
    four_forms(host, [EQ(D2, 3), D3_LT, D4_GE], label="... and no 3 (an empty run at the tile's end)")


def test_runs_of_31_32_33_places(host):
    """One value's count in a tile set to 31, 32 and 33 through the host arrays and a sync: runs that end inside a word, at its last bit and
    one bit into the next. Every row of those runs passes d3 and d4, so a place lost at a run's edge changes the answer."""
    warm(host)
    rng = np.random.default_rng(7)
    for (s, tile), n in zip(((0, 0), (1, 0), (2, 1)), (31, 32, 33)):
        seg = host.tab.segments[s]
        sl = slice(tile * TILE, (tile + 1) * TILE)
        d2 = seg["d"][D2][sl]
        d2[d2 == 1] = 0
        at = rng.choice(TILE, size=n, replace=False)
        d2[at] = 1
        seg["d"][3][sl][at] = 5
        seg["d"][4][sl][at] = 900
        host.sync(s, tile * TILE, TILE)
    for v in (1, 0, 2):
        four_forms(host, [EQ(D2, v), D3_LT, D4_GE], label=f"counts of 31, 32 and 33 in three tiles, d2 == {v}")
    snap = [TILE, TILE, 2 * TILE]      # those tiles alone (and segment 2's first)
    c = four_forms(host, C3, seg_rows=snap, label="the edited tiles alone")
    first = host.tab.segments[2]["d"]
    in_first = int(np.count_nonzero((first[D2][:TILE] == 1) & (first[3][:TILE] < 447) & (first[4][:TILE] >= 553)))
    assert c.passed_recs == 31 + 32 + 33 + in_first, c.passed_recs


@pytest.mark.parametrize("snap, planes", [([ROWS, ROWS, ROWS], True), ([0, ROWS, 0], True), ([2048, 4096, ROWS], True), ([0, 2048 + 37, ROWS], False)])
def test_snapshots(host, snap, planes):
    """A snapshot per segment that is the mirrored rows or whole tiles (0 included) is honoured by the clustered planes; one that cuts into a
    built tile keeps the row-order planes (places have lost their row numbers) — over the grouped records, as before."""
    warm(host)
    four_forms(host, C3, seg_rows=snap, label="snapshot", planes=planes)
    four_forms(host, [EQ(D2, 0), D3_LT, D4_GE], seg_rows=snap, label="snapshot, literal 0", planes=planes)
    four_forms(host, [EQ(D2, 3), D3_LT, D4_GE], seg_rows=snap, label="snapshot, the last value", planes=planes)


def test_syncs_rebuild_whole_tiles(host):
    warm(host)
    host.append(0, 1500)                       # fills the tile of 904 rows and runs 356 rows into the next
    four_forms(host, C3, label="after an append across a tile's end")
    four_forms(host, [EQ(D2, 3), D3_LT, D4_GE], label="... the last value")
    host.change(1, 2040, 16)                   # 16 rows astride the first tile's end change their d2, d3, d4 and metrics
    host.sync(1, 2040, 16)
    four_forms(host, C3, label="after rows changed astride a tile's end")
    host.add_segment(ROWS)                     # beyond the reserved segments: arenas and layouts move, the form starts over in new buffers
    four_forms(host, C3, label="after the table grew")
    four_forms(host, [EQ(D2, 3), D3_LT, D4_GE], label="after the table grew, the last value")


def test_placement_moves_the_clustered_planes(host, monkeypatch):
    warm(host)
    monkeypatch.setenv("VH_TEST_PLACE_CANDIDATES", "4")
    for verdict in ("alternate", "reject", "keep"):
        monkeypatch.setenv("VH_TEST_PLACE_VERDICT", verdict)
        flags = host.dt.warm(host.plan(HOT))
        assert flags & capi.INFO_GROUPED_PLANES, hex(flags)
        four_forms(host, C3, label=f"after a prepare that moved the layouts ({verdict})")
    host.change(0, 100, 300)
    host.sync(0, 100, 300)
    four_forms(host, C3, label="a sync after the moves")


def test_planner_rule(host):
    warm(host)
    four_forms(host, [EQ(D2, 1), REL(D2, capi.OP_LT, "lt", 3), D3_LT], label="a second leaf on d2", planes=False)
    four_forms(host, [EQ(D2, 1), D3_LT], label="the filter reads d3 alone beside d2")
    four_forms(host, [EQ(D2, 1), EQ(D2, 1), D3_LT], label="two == leaves on d2", grouped=False)


def test_background_build_reaches_the_clustered_planes():
    """A background-build table: queries answer from what exists while the worker compiles and builds; once vh_table_build_wait finds the
    worker idle and nothing more is asked for, the steady state reads the clustered planes."""
    h = C3Host(3, ROWS, CAP)
    try:
        h.dt.set_build_mode(True)
        res = None
        for rnd in range(8):     # (projection and planes, the grouped form, then the kernel of each shape: a few rounds of sightings and jobs)
            for _ in range(3):
                res = ask(h, C3, HOT, label=f"background round {rnd}")
            bi = h.dt.build_wait(120_000)
            assert bi.jobs_queued == 0 and bi.jobs_running == 0
            res = ask(h, C3, HOT, label=f"background round {rnd}, after the wait")
            if res.grouped_planes and not res.flags & capi.INFO_BUILD_PENDING:
                break
        assert res.grouped_payload and res.grouped_planes and not res.flags & capi.INFO_BUILD_PENDING, hex(res.flags)
        assert res.passed_recs == ask(h, C3, PART | JIT | capi.PLAN_NO_PACK, label="background table, the arenas").passed_recs
    finally:
        h.close()
