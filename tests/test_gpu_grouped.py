"""Grouped payload records (viyadb_amd/csrc/vh_grouped.h): a second form of a 4-byte bit-record projection whose 2048-row tiles are sorted
by a narrow column the filter compares for equality, read by the compiled bit-sliced scan through places it computes from the planes.
Tables: 3 segments of 5 000 mirrored rows (two full tiles and one of 904) in segments with room for 8 192. Every answer is compared with
the oracle over the host's current arrays (tests/parity.compare), the three forms — grouped, row-order records (VH_PLAN_NO_GROUPED), the
arenas (VH_PLAN_NO_PACK) — must agree bit for bit, and `grouped_payload` must be set exactly where the planner's rule says."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare, sort_rows
from tests.test_gpu_layout_lifecycle import C3Host, D2
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="grouped records are read by the compiled scan only")]
PART, JIT, PACK = 64, capi.PLAN_FORCE_JIT, capi.PLAN_FORCE_PACK
HOT = PART | JIT | PACK                      # the flagship's organisation: compiled bit-sliced scan, 4-byte bit records, partitioned tuples
ROWS, CAP = 5000, 8192


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def EQ(col, v):
    return ("rel", col, capi.OP_EQ, v), {"op": "eq", "column": f"d{col}", "value": str(v)}


def REL(col, op, name, v):
    return ("rel", col, op, v), {"op": name, "column": f"d{col}", "value": str(v)}


D3_LT, D4_GE = REL(3, capi.OP_LT, "lt", 447), REL(4, capi.OP_GE, "ge", 553)


def ask(h, leaves, flags, seg_rows=None, label="", top="and"):
    """The C3 query with `leaves` under one top-level AND (or OR), on the device and in the oracle."""
    filt = [l[0] for l in leaves] + [(top, len(leaves))]
    q = dict(h.w.query, filter={"op": top, "filters": [l[1] for l in leaves]})
    p = h.w.plan
    res = h.dt.query_agg(AggPlan(filter=filt, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint, seg_rows=seg_rows))
    compare(res, vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows), f"{label} flags={flags:#x} snapshot={seg_rows}")
    return res


def same_bits(a, b, label):
    """Integer states (and keys) of two results, row for row in key order."""
    pa, pb = sort_rows(a.keys, a.states), sort_rows(b.keys, b.states)
    for x, y in zip(a.keys + a.states, b.keys + b.states):
        assert x.dtype == y.dtype and x.dtype.kind in "iu" and np.array_equal(x[pa], y[pb]), label


def three_forms(h, leaves, seg_rows=None, label="", grouped=True):
    g = ask(h, leaves, HOT, seg_rows, label + " grouped")
    assert g.jit and g.sliced and g.packed and g.pack_bits and g.pack_rec_bytes == 4, (label, hex(g.flags), g.kernel)
    assert g.grouped_payload == grouped, (label, hex(g.flags))
    r = ask(h, leaves, HOT | capi.PLAN_NO_GROUPED, seg_rows, label + " row order")
    assert r.packed and r.sliced and not r.grouped_payload, (label, hex(r.flags))
    a = ask(h, leaves, PART | JIT | capi.PLAN_NO_PACK, seg_rows, label + " arenas")
    assert not a.packed and not a.grouped_payload, (label, hex(a.flags))
    same_bits(g, r, label + ": grouped against row-order records")
    same_bits(g, a, label + ": grouped against the arenas")
    return g


def nothing_scanned(h, leaves, seg_rows=None, label=""):
    """A plan whose every segment is left out before the scan (an empty snapshot, a literal outside the segments' recorded min / max): it
    binds no projection, so the planner's rule gives it no grouped records either; the three forms still answer alike."""
    g = ask(h, leaves, HOT, seg_rows, label + " grouped")
    assert g.passed_recs == 0 and not g.packed and not g.grouped_payload, (label, hex(g.flags))
    r = ask(h, leaves, HOT | capi.PLAN_NO_GROUPED, seg_rows, label + " row order")
    a = ask(h, leaves, PART | JIT | capi.PLAN_NO_PACK, seg_rows, label + " arenas")
    assert not r.grouped_payload and not a.grouped_payload, (label, hex(r.flags), hex(a.flags))
    same_bits(g, r, label + ": grouped against row-order records")
    same_bits(g, a, label + ": grouped against the arenas")


@pytest.fixture
def host():
    h = C3Host(3, ROWS, CAP)
    yield h
    h.close()


def warm(h):
    """vh_table_prepare of the C3 plan: projection, bit-sliced planes and — the plan qualifies — the grouped records."""
    flags = h.dt.warm(h.plan(HOT))
    assert flags & capi.INFO_GROUPED_PAYLOAD, hex(flags)


C3 = [EQ(D2, 1), D3_LT, D4_GE]


def test_c3_plan_reads_grouped_records(host):
    warm(host)
    g = three_forms(host, C3, label="C3")
    assert g.passed_recs > 0     # (a table this small is planned onto the hash table; DENSE_PART reads the same queue: tests/test_gpu_fullsize.py)
    for v in (0, 2, 3):         # every value of the field: another run of the same tiles
        three_forms(host, [EQ(D2, v), D3_LT, D4_GE], label=f"d2 == {v}")
    three_forms(host, [D3_LT, EQ(D2, 1)], label="the == leaf last, two conjuncts")


def test_literals_without_rows(host):
    d2 = [seg["d"][D2] for seg in host.tab.segments]
    for s, col in enumerate(d2):
        col[col == 2] = 3        # no row holds 2; the segments' min / max stay 0 and 3, so none is left out for `d2 == 2` and the scan runs
        host.sync(s, 0, ROWS)
    warm(host)
    assert three_forms(host, [EQ(D2, 2), D3_LT, D4_GE], label="a value no row has").passed_recs == 0      # (an empty run in every tile)
    assert three_forms(host, [EQ(D2, 3), D3_LT, D4_GE], label="the value that took the rows").passed_recs > 0
    nothing_scanned(host, [EQ(D2, 7), D3_LT, D4_GE], label="a literal beyond the field")      # (beyond every segment's max too)


def test_a_segment_of_one_value(host):
    host.tab.segments[1]["d"][D2][:] = 1
    host.sync(1, 0, ROWS)
    warm(host)
    three_forms(host, C3, label="segment 1 holds d2 = 1 alone")
    three_forms(host, [EQ(D2, 0), D3_LT, D4_GE], label="... and no 0")


@pytest.mark.parametrize("snap", [[0, 0, 0], [0, 2048 + 37, ROWS], [2048 + 37, ROWS, 0], [ROWS, 2048, 4096 + 1], [ROWS, ROWS, ROWS]])
def test_snapshots(host, snap):
    warm(host)
    forms = three_forms if any(snap) else nothing_scanned
    forms(host, C3, seg_rows=snap, label="snapshot")
    forms(host, [EQ(D2, 0), D3_LT, D4_GE], seg_rows=snap, label="snapshot, literal 0 (what rows behind the mirrored ones read as)")


def test_syncs_rebuild_whole_tiles(host):
    warm(host)
    host.append(0, 1500)                       # fills the tile of 904 rows (4096 .. 6143) and runs 356 rows into the next
    three_forms(host, C3, label="after an append across a tile's end")
    host.change(1, 2040, 16)                   # 16 rows astride the first tile's end change their d2, d3, d4 and metrics
    host.sync(1, 2040, 16)
    three_forms(host, C3, label="after rows changed astride a tile's end")
    host.change(2, 4999, 1)
    host.sync(2, 4999, 1)
    host.append(2, 1)                          # the last mirrored row, then one more
    three_forms(host, C3, label="after the last row changed and one was appended")
    host.add_segment(ROWS)                     # beyond the reserved segments: arenas and layouts move, the grouped form starts over
    three_forms(host, C3, label="after the table grew")


def test_planner_rule(host):
    warm(host)
    no = dict(grouped=False)
    r = ask(host, [EQ(D2, 1), D3_LT], HOT, top="or", label="top-level OR")
    assert not r.grouped_payload, hex(r.flags)
    three_forms(host, [REL(D2, capi.OP_NE, "ne", 1), D3_LT, D4_GE], label="no == leaf", **no)
    three_forms(host, [EQ(D2, 1), EQ(D2, 1), D3_LT], label="two == leaves on the column", **no)
    three_forms(host, [EQ(3, 5), D4_GE], label="== on a 10-bit field only", **no)
    three_forms(host, [EQ(3, 5), EQ(D2, 1), D4_GE], label="== on a wide field, then on d2")
    r = ask(host, C3, HOT | capi.PLAN_NO_SLICED, label="byte planes")
    assert not r.grouped_payload and not r.sliced, hex(r.flags)
    r = ask(host, C3, HOT | capi.PLAN_FORCE_QPAY, label="streamed records")
    assert not r.grouped_payload, hex(r.flags)


def test_placement_moves_the_grouped_records(host, monkeypatch):
    warm(host)
    monkeypatch.setenv("VH_TEST_PLACE_CANDIDATES", "4")
    for verdict in ("alternate", "reject", "keep"):
        monkeypatch.setenv("VH_TEST_PLACE_VERDICT", verdict)
        assert host.dt.warm(host.plan(HOT)) & capi.INFO_GROUPED_PAYLOAD
        three_forms(host, C3, label=f"after a prepare that moved the layouts ({verdict})")
    host.change(0, 100, 300)
    host.sync(0, 100, 300)
    three_forms(host, C3, label="a sync after the moves")
