"""Set leaves (VH_F_INSET) evaluated as truth tables on the bit-sliced predicate planes (viyadb_amd/csrc/vh_inset.h: vh_inset_bits; the
planner's rule: every set leaf's field in the sliced projection has at most VH_INSET_TRUTH_BITS = 10 bits). Tables are C3Host(3, 5000,
8192): two full 2048-row tiles and one of 904 rows per segment. Every answer goes through compare() against the oracle over the host's
current arrays, and is held bit for bit against the same plan under VH_PLAN_NO_SLICED (the lookup per row on byte planes / arenas: the
path such a plan took before); short lists against the VH_F_IN plan too. `inset_sliced` (vh_result_info.reserved bit 25) must be set
exactly where the planner's rule says."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.test_gpu_gplanes import CAP, D4_GE, EQ, HOT, JIT, PART, REL, ROWS, ask, same_bits, warm
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from viyadb_amd import capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="bit-sliced planes are read by the compiled scan only")]
NO_SLICED = capi.PLAN_NO_SLICED


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture
def host():
    h = C3Host(3, ROWS, CAP)
    yield h
    h.close()


def SET(col, values, equal=True, kind="inset"):
    f = {"op": "in", "column": f"d{col}", "values": [str(v) for v in values]}
    return (kind, col, equal, [int(v) for v in values]), f if equal else {"op": "not", "filter": f}


def held(h, col):
    return np.unique(np.concatenate([seg["d"][col][:seg["size"]] for seg in h.tab.segments]))


def both(h, leaves, flags, seg_rows=None, label="", sliced=True):
    """The plan on the bit planes and its twin under VH_PLAN_NO_SLICED: each against the oracle (inside ask), then bit for bit."""
    a = ask(h, leaves, flags, seg_rows, label)
    assert a.jit and a.inset, (label, hex(a.flags), a.kernel)
    assert a.sliced == sliced and a.inset_sliced == sliced, (label, hex(a.flags), a.kernel)
    b = ask(h, leaves, flags | NO_SLICED, seg_rows, label + " NO_SLICED")
    assert b.inset and not b.sliced and not b.inset_sliced, (label, hex(b.flags))
    same_bits(a, b, label + ": bit planes against the lookup per row")
    return a


# ---- 1. forms of the d3 set (fails without the feature: `sliced` is false for a plan with a set leaf)
def test_forms_of_the_d3_set(host):
    warm(host)
    d3 = held(host, D3)
    top = int(d3.max())
    assert top < 1024 and top >= 512, top      # a 10-bit field
    rng = np.random.default_rng(11)
    sets = {"one held value": [int(d3[len(d3) // 3])], "zero": [0], "the column's maximum": [top], "word edges": [31, 32, 33, 63, 64],
            "500 members": sorted(int(v) for v in rng.choice(1000, size=500, replace=False)), "every value of the field": list(range(1024)),
            "in range and beyond": [5, 31, 32, 700, 1024, 5000, top], "beyond alone": [1024, 5000]}
    D2_EQ = EQ(D2, 1)
    base = ask(host, [D2_EQ, D4_GE], PART | JIT | capi.PLAN_NO_PACK, label="the other leaves alone")
    for name, members in sets.items():
        for equal in (True, False):
            label = f"d3 {'IN' if equal else 'NOT IN'} {name}"
            leaves = [D2_EQ, SET(D3, members, equal), D4_GE]
            a = both(host, leaves, HOT, label=label)
            if len(members) <= 8:      # a short list: the VH_F_IN plan with the same fields (bit-serial comparisons on the same planes)
                same_bits(a, ask(host, [D2_EQ, SET(D3, members, equal, kind="in"), D4_GE], HOT, label=label + " as VH_F_IN"), label + ": against VH_F_IN")
            if name == "beyond alone":
                # IN passes nothing. NOT IN would pass every row the other leaves pass — but segment skipping comes first, and it asks of IN
                # and NOT IN alike whether some member lies within the segment's min / max (the reference's SegmentSkipBuilder does not
                # look at the polarity; segment_passes, vhh_plan.h): no segment is scanned, which is what the oracle says too
                assert a.passed_recs == 0 and a.scanned_segments == 0, (label, a.passed_recs, a.scanned_segments)
            if name == "in range and beyond" and not equal:      # (here the members beyond the field are clipped in a scan that does run)
                assert a.scanned_segments == 3 and 0 < a.passed_recs < base.passed_recs, (label, a.passed_recs, base.passed_recs)
            if name == "every value of the field":
                assert a.passed_recs == (base.passed_recs if equal else 0), (label, a.passed_recs, base.passed_recs)
    assert base.passed_recs > 0


# ---- 2. the forms underneath: grouped records and clustered planes serve the set plan under their own rules
def test_grouped_records_and_clustered_planes(host):
    warm(host)
    members = list(range(0, 1000, 3)) + [1024]
    for equal in (True, False):
        leaves = [EQ(D2, 1), SET(D3, members, equal), D4_GE]
        label = f"d3 {'IN' if equal else 'NOT IN'} 335 members"
        c = both(host, leaves, HOT, label=label + " clustered")
        assert c.packed and c.grouped_payload and c.grouped_planes, (label, hex(c.flags))
        g = both(host, leaves, HOT | capi.PLAN_NO_GPLANES, label=label + " row-order planes")
        assert g.grouped_payload and not g.grouped_planes, (label, hex(g.flags))
        r = both(host, leaves, HOT | capi.PLAN_NO_GROUPED, label=label + " row-order records")
        assert r.packed and not r.grouped_payload and not r.grouped_planes, (label, hex(r.flags))
        a = both(host, leaves, PART | JIT | capi.PLAN_NO_PACK, label=label + " arenas")
        assert not a.packed and not a.grouped_payload
        for other, name in ((g, "row-order planes"), (r, "row-order records"), (a, "the arenas")):
            same_bits(c, other, f"{label}: clustered planes against {name}")
        assert 0 < c.passed_recs
    # a set leaf on the grouping column is not the `==` leaf the grouped forms go by; beside that leaf it is one more reader of the column
    s = both(host, [SET(D2, [1]), REL(3, capi.OP_LT, "lt", 447), D4_GE], HOT, label="a set on d2, no == leaf")
    assert not s.grouped_payload and not s.grouped_planes, hex(s.flags)
    s = both(host, [EQ(D2, 1), SET(D2, [1, 3]), D4_GE], HOT, label="a set on d2 beside its == leaf")
    assert s.grouped_payload and not s.grouped_planes, hex(s.flags)


# ---- 3. field widths: 1, 5, 6 and 10 bits run on the planes, 11 bits does not
def test_field_widths(host):
    mods = {D2: 2, D3: 32, D4: 64, 5: 2048}           # d0 holds 0 .. 999 as generated: 10 bits
    for s, seg in enumerate(host.tab.segments):
        for col, m in mods.items():
            seg["d"][col][:] %= m
        seg["d"][5][7] = 2047                          # (the 11-bit field's last value is held)
        host.sync(s, 0, ROWS)
    assert int(held(host, 0).max()) >= 512 and int(held(host, 5).max()) == 2047
    host.dt.predpack([0, D2, D3, D4], sliced=True)
    host.dt.predpack([D2, 5], sliced=True)
    flags = PART | JIT | capi.PLAN_NO_PACK
    cases = [(D2, 1, [1]), (D2, 1, [1, 2, 3]), (D3, 5, [0, 7, 30, 31, 32, 99]), (D4, 6, [0, 31, 32, 33, 63, 64]),
             (0, 10, list(range(1, 1000, 7)) + [1023, 1024]), (0, 10, list(range(990, 1000)))]
    for snap in (None, [ROWS, 1234, 0]):
        for col, bits, members in cases:
            other = REL(4, capi.OP_GE, "ge", 20) if col != D4 else REL(3, capi.OP_LT, "lt", 20)
            for equal in (True, False):
                a = both(host, [SET(col, members, equal), other], flags, seg_rows=snap, label=f"a {bits}-bit field, {'IN' if equal else 'NOT IN'} {members[:6]}")
                assert 0 < a.passed_recs < a.scanned_recs
        for equal in (True, False):                    # 11 bits: beyond VH_INSET_TRUTH_BITS — the lookup per row answers, from the arenas
            a = both(host, [SET(5, list(range(0, 2048, 16)) + [1023, 2047, 2048], equal), EQ(D2, 1)], flags, seg_rows=snap, label="an 11-bit field", sliced=False)
            assert 0 < a.passed_recs < a.scanned_recs
        # ... and one wide set leaf keeps the whole plan off the planes, its narrow set leaves included
        both(host, [SET(5, [3, 2047]), SET(D2, [1])], flags, seg_rows=snap, label="an 11-bit and a 1-bit set", sliced=False)
    # the ordinary leaves of those columns still run bit-serially on the same planes
    assert ask(host, [REL(5, capi.OP_LT, "lt", 1000), EQ(D2, 1)], flags, label="11 bits, relational").sliced


# ---- 4. VH_MAX_SETS set leaves in one plan, nested
def test_four_set_leaves_nested(host):
    warm(host)
    # (about 3 % of the rows pass, as with C3: a plan that passes many rows streams its payload beside byte planes instead — a rows form)
    A, B = SET(D2, [1, 5]), SET(D3, range(0, 1000, 8))
    Cn, D = SET(D4, list(range(100, 900)) + [4096], equal=False), SET(D3, [31, 32, 33, 500, 999, 1023])
    filt = [A[0], B[0], ("and", 2), Cn[0], D[0], ("and", 2), ("or", 2)]
    q = dict(host.w.query, filter={"op": "or", "filters": [{"op": "and", "filters": [A[1], B[1]]}, {"op": "and", "filters": [Cn[1], D[1]]}]})
    from viyadb_amd.executor import AggPlan
    p = host.w.plan
    want = vo.scan_aggregate(vo.parse_query(host.tab, q))
    got = {}
    for flags in (HOT, HOT | NO_SLICED):
        res = host.dt.query_agg(AggPlan(filter=filt, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint))
        compare(res, want, f"(A & B) | (NOT IN C & D) flags={flags:#x}")
        got[flags] = res
    a, b = got[HOT], got[HOT | NO_SLICED]
    assert a.jit and a.sliced and a.inset and a.inset_sliced and not a.grouped_payload, hex(a.flags)
    assert b.inset and not b.sliced and not b.inset_sliced, hex(b.flags)
    same_bits(a, b, "four set leaves: bit planes against the lookup per row")
    assert 0 < a.passed_recs < a.scanned_recs


# ---- 5. a value outgrows its field: nothing reads a stale truth table
def test_a_value_outgrows_its_field(host):
    warm(host)
    members = [3, 300, 1024]
    leaves = [EQ(D2, 1), SET(D3, members), D4_GE]
    before = both(host, leaves, HOT, label="before")
    seg = host.tab.segments[1]
    assert not (seg["d"][D2][4100] == 1 and int(seg["d"][D3][4100]) in members and seg["d"][D4][4100] >= 553)
    seg["d"][D2][4100], seg["d"][D3][4100], seg["d"][D4][4100] = 1, 1024, 900      # (a row of the ragged last tile)
    host.sync(1, 4100, 1)
    # the projection no longer holds the column's values: dropped at the next look; the plan falls back to the lookup per row
    after = both(host, leaves, HOT, label="after d3 = 1024, projection voided", sliced=False)
    assert after.passed_recs == before.passed_recs + 1, (before.passed_recs, after.passed_recs)
    # rebuilt, d3 takes 11 bits: beyond the limit, so the set plan keeps the lookup — the relational plan is back on the planes
    host.dt.predpack([D2, D3, D4], sliced=True)
    again = both(host, leaves, HOT, label="after d3 = 1024, projection rebuilt at 11 bits", sliced=False)
    same_bits(after, again, "voided against rebuilt")
    assert ask(host, [EQ(D2, 1), REL(3, capi.OP_LT, "lt", 447), D4_GE], HOT, label="C3 on the rebuilt planes").sliced
    # ... and a NOT IN of the new value alone leaves that row out
    # (with a member every segment holds: one that only segment 1 holds would skip the others, for NOT IN as for IN — segment_passes)
    n = both(host, [EQ(D2, 1), SET(D3, [1024, 5], equal=False), D4_GE], HOT, label="NOT IN {1024, 5}", sliced=False)
    want = sum(int(np.count_nonzero((sg["d"][D2][:ROWS] == 1) & (sg["d"][D4][:ROWS] >= 553) & ~np.isin(sg["d"][D3][:ROWS], [1024, 5]))) for sg in host.tab.segments)
    assert n.passed_recs == want and n.scanned_segments == 3, (n.passed_recs, want)


# ---- 6. one code object whatever the list
def test_one_code_object_whatever_the_list(host):
    warm(host)
    kernels = set()
    for members in ([447], [1, 2, 3, 5, 8, 13, 21, 34], list(range(0, 1000, 2)) + list(range(1, 200, 2))):
        assert len(members) in (1, 8, 600)
        kernels.add(both(host, [EQ(D2, 1), SET(D3, members), D4_GE], HOT, label=f"{len(members)} members").kernel)
    assert len(kernels) == 1, kernels


# ---- 7. the automatic builder gives such a plan bit-sliced planes, and the listing counts its reads
def test_automatic_builds(host):
    import os
    leaves = [EQ(D2, 1), SET(D3, range(5, 900, 3)), D4_GE]
    flags = PART | JIT | capi.PLAN_FORCE_PACK
    first = ask(host, leaves, flags, label="first sighting")
    assert first.inset and not first.sliced and not first.inset_sliced, hex(first.flags)
    n = int(os.environ.get("VH_AUTO_NARROW", "3"))
    for k in range(n + 1):
        res = ask(host, leaves, flags, label=f"sighting {k + 2}")
    assert res.sliced and res.inset_sliced, hex(res.flags)

    def sliced_layouts():
        return [x for x in host.dt.layouts()[0] if x.kind == capi.LAYOUT_PRED_SLICED]
    lay = sliced_layouts()
    assert len(lay) == 1 and lay[0].flags & capi.LAYOUT_AUTOMATIC and tuple(lay[0].cols[:lay[0].ncols]) == (D2, D3, D4), [(x.kind, x.flags) for x in lay]
    assert not any(x.kind == capi.LAYOUT_PRED_BYTES for x in host.dt.layouts()[0])      # (nothing asked for planes the plan no longer wants)
    uses = lay[0].uses
    assert uses >= 1
    ask(host, leaves, flags, label="one more")
    assert sliced_layouts()[0].uses > uses
