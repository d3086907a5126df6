"""vh_query_select on the bit-sliced predicate planes (select_count_sliced_kernel / select_emit_sliced_kernel over
viyadb_amd/csrc/vh_bits_eval.h). Tables are C3Host(3, 5000, 8192): 5000 rows are 156 plane words and 8 rows, two full 2048-row chunks
and one of 904. Every case asserts three things: the rows and all four counters against the oracle over the host's current arrays; the
same rows bit for bit against the same query under VH_PLAN_NO_SLICED (the arenas: the path every select took before); and the flags of
vh_rows_flags — bit 13 set where the planner's rule says the planes are read, clear elsewhere. Nothing here is compiled at run time:
the file runs under VH_JIT=off too, and the planes must be read there as well."""
import numpy as np
import pytest

from tests.test_gpu_layout_lifecycle import C3Host, D2, D3, D4
from tests.test_gpu_select import oracle_select
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
ROWS, CAP = 5000, 8192
ID = 6                                           # C3's row-id column: in no projection
NO_SLICED = capi.PLAN_NO_SLICED
ON_PLANES = capi.INFO_ON_PLANES      # vh_result_info.reserved: narrowed, a predicate projection, its bit-sliced form
SLICED = capi.INFO_SLICED
OPS = [("eq", capi.OP_EQ), ("ne", capi.OP_NE), ("lt", capi.OP_LT), ("le", capi.OP_LE), ("gt", capi.OP_GT), ("ge", capi.OP_GE)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _host():
    h = C3Host(3, ROWS, CAP)
    h.dt.predpack([D2, D3, D4], sliced=True)
    return h


@pytest.fixture(scope="module")
def shared():
    """One table for the cases that change nothing."""
    h = _host()
    yield h
    h.close()


@pytest.fixture
def host():
    h = _host()
    yield h
    h.close()


def REL(col, name, v):
    return ("rel", col, dict(OPS)[name], v), {"op": name, "column": "id" if col == ID else f"d{col}", "value": str(v)}


def SET(col, values, equal=True, kind="inset"):
    f = {"op": "in", "column": f"d{col}", "values": [str(v) for v in values]}
    return (kind, col, equal, [int(v) for v in values]), f if equal else {"op": "not", "filter": f}


def AND(*leaves):
    return [l[0] for l in leaves] + [("and", len(leaves))], {"op": "and", "filters": [l[1] for l in leaves]}


C3 = AND(REL(D2, "eq", 1), REL(D3, "lt", 447), REL(D4, "ge", 553))
ALL = list(range(12))


def check(h, filt, cols, skip=0, limit=0, seg_rows=None, flags=0, sliced=True, label=""):
    """The select against the oracle, against its twin under VH_PLAN_NO_SLICED, and the path each took. -> (RowsInfo, flags)."""
    plan, qfilter = filt
    q = {k: v for k, v in h.w.query.items() if k != "filter"}
    if qfilter is not None:
        q["filter"] = qfilter
    want, stats = oracle_select(h.tab, q, cols, skip, limit, seg_rows)
    label = f"{label} skip={skip} limit={limit} snapshot={seg_rows} flags={flags:#x}"
    got, info, path = h.dt.query_select_ex(plan, cols, skip=skip, limit=limit, seg_rows=seg_rows, flags=flags)
    assert bool(path & SLICED) == sliced, (label, hex(path))
    assert (path & ON_PLANES) == (ON_PLANES if sliced else 0), (label, hex(path))
    twin, tinfo, tpath = h.dt.query_select_ex(plan, cols, skip=skip, limit=limit, seg_rows=seg_rows, flags=flags | NO_SLICED)
    assert not tpath & ON_PLANES, (label, hex(tpath))
    for res, i in ((got, info), (twin, tinfo)):
        assert (i.nrows, i.scanned_recs, i.scanned_segments, i.passed_recs) == \
               (stats["output_recs"], stats["scanned_recs"], stats["scanned_segments"], stats["passed_recs"]), label
        for c, (a, b) in zip(cols, zip(res, want)):
            assert len(a) == len(b) and (not len(b) or np.array_equal(a, b.astype(a.dtype))), (label, c)
    for a, b in zip(got, twin):
        assert a.dtype == b.dtype and np.array_equal(a, b), label
    return info, path


def c3_mask(seg, rows):
    d = seg["d"]
    return (d[D2][:rows] == 1) & (d[D3][:rows] < 447) & (d[D4][:rows] >= 553)


# ---- 1. windows (fails without the feature: no select reads the planes, vh_rows_flags does not exist)
def test_windows(shared):
    h = shared
    m = c3_mask(h.tab.segments[0], ROWS)
    word, chunk, seg = int(m[:32].sum()), int(m[:2048].sum()), int(m.sum())
    assert 0 < chunk < seg
    rng = np.random.default_rng(7)
    total = 3 * seg
    windows = [(0, 0), (0, 10), (17, 0), (5, 3), (10 ** 9, 0)]
    windows += [(int(rng.integers(0, total + 40)), int(rng.integers(0, 60))) for _ in range(20)]
    windows += [(max(0, n + d), lim) for n in (word, chunk, seg) for d in (-1, 0, 1) for lim in (0, 2)]
    passed = None
    for skip, limit in windows:
        info, _ = check(h, C3, ALL, skip, limit, label="C3")
        assert passed is None or info.passed_recs == passed
        passed = info.passed_recs
    assert passed > 0


# ---- 2. snapshots of the middle segment: nothing at or beyond seg_rows passes, the word that straddles it is masked
def test_snapshots(shared):
    for n in (0, 1, 31, 32, 33, 2047, 2048, 2049, 4999):
        snap = [ROWS, n, ROWS]
        check(shared, C3, ALL, 0, 0, seg_rows=snap, label="C3")
        check(shared, AND(REL(D3, "ne", 1023)), [D3, ID], 3, 0, seg_rows=snap, label="every row passes")      # (the planes' bits beyond the snapshot are those of real rows)


# ---- 3. every relation on d3 (a 10-bit field holding 0 .. 999), literals inside the field, at its ends and beyond it
def test_relops(shared):
    some = none = 0
    for name, _ in OPS:
        for lit in (0, 446, 447, 1023, 1024, 2 ** 32 - 1):
            info, _ = check(shared, AND(REL(D3, name, lit)), [D3, ID], 0, 0, label=f"d3 {name} {lit}")
            some += info.passed_recs > 0
            none += info.passed_recs == 0
    assert some and none


# ---- 4. IN / NOT IN of three values, as VH_F_IN and as VH_F_INSET
def test_in_lists(shared):
    for equal in (True, False):
        for kind in ("in", "inset"):
            info, path = check(shared, AND(SET(D3, [5, 446, 999], equal, kind)), [D3, ID], 0, 0, label=f"d3 {'IN' if equal else 'NOT IN'} as {kind}")
            assert 0 < info.passed_recs < info.scanned_recs
            want = (capi.INFO_INSET | capi.INFO_INSET_SLICED) if kind == "inset" else 0
            assert path & (capi.INFO_INSET | capi.INFO_INSET_SLICED | capi.INFO_INSET_SEARCH) == want, hex(path)
    # the twin's bits with a set leaf: a lookup per row (bit 22), no truth table (bit 25)
    _, _, tpath = shared.dt.query_select_ex(AND(SET(D3, [5, 446, 999]))[0], [D3], flags=NO_SLICED)
    assert tpath & capi.INFO_INSET and not tpath & (capi.INFO_INSET_SLICED | SLICED), hex(tpath)
    _, _, spath = shared.dt.query_select_ex(AND(SET(D3, [5, 446, 999]))[0], [D3], flags=NO_SLICED | capi.PLAN_SET_SEARCH)
    assert spath & capi.INFO_INSET and spath & capi.INFO_INSET_SEARCH, hex(spath)


# ---- 5. filter shapes: a nest (the operand stack) and a single leaf
def test_filter_shapes(shared):
    a, b, c = REL(D2, "eq", 1), REL(D3, "lt", 100), REL(D4, "ge", 553)
    nest = ([a[0], b[0], ("or", 2), c[0], ("and", 2)], {"op": "and", "filters": [{"op": "or", "filters": [a[1], b[1]]}, c[1]]})
    info, _ = check(shared, nest, ALL, 4, 0, label="(d2 == 1 | d3 < 100) & d4 >= 553")
    assert 0 < info.passed_recs < info.scanned_recs
    leaf = ([a[0]], a[1])
    info, _ = check(shared, leaf, ALL, 0, 100, label="d2 == 1")
    assert 0 < info.passed_recs < info.scanned_recs
    deep = ([a[0], b[0], c[0], ("or", 2), ("and", 2), SET(D3, [7, 8, 9])[0], ("or", 2)],
            {"op": "or", "filters": [{"op": "and", "filters": [a[1], {"op": "or", "filters": [b[1], c[1]]}]}, SET(D3, [7, 8, 9])[1]]})
    check(shared, deep, [D2, D3, D4, ID], 0, 0, label="(d2 == 1 & (d3 < 100 | d4 >= 553)) | d3 IN {7, 8, 9}")


# ---- 6. eligibility: the arenas answer, with the flag clear and the rows right
def test_eligibility(shared):
    check(shared, AND(REL(D2, "eq", 1), REL(ID, "lt", 9000)), ALL, 2, 0, sliced=False, label="a leaf on id")
    check(shared, ([], None), [D2, ID], 4990, 20, sliced=False, label="no filter")
    for flag in (NO_SLICED, capi.PLAN_NO_PREDPACK, capi.PLAN_NO_NARROW):
        check(shared, C3, ALL, 1, 0, flags=flag, sliced=False, label="C3")
    # ... and the path does not hang on the compiled scan's switches
    for flag in (capi.PLAN_NO_JIT, capi.PLAN_NO_FAST, capi.PLAN_NO_JIT | capi.PLAN_NO_FAST):
        check(shared, C3, ALL, 1, 0, flags=flag, sliced=True, label="C3")


def planes(h):
    return [x for x in h.dt.layouts()[0] if x.kind in (capi.LAYOUT_PRED_BYTES, capi.LAYOUT_PRED_SLICED)]


def test_no_projection():
    h = C3Host(3, ROWS, CAP)
    try:
        check(h, C3, ALL, 0, 0, sliced=False, label="C3, no projection")
        assert not planes(h)                               # ... and the select built none
        h.dt.predpack([D2, D3, D4], sliced=False)          # byte planes are not what these kernels read
        check(h, C3, ALL, 0, 0, sliced=False, label="C3, byte planes only")
        h.dt.predpack([D2, D3], sliced=True)               # a bit-sliced projection that lacks one of the filter's columns
        check(h, C3, ALL, 0, 0, sliced=False, label="C3, planes of d2 and d3 only")
        check(h, AND(REL(D2, "eq", 1), REL(D3, "lt", 447)), ALL, 0, 0, sliced=True, label="d2 and d3 alone")
        assert len(planes(h)) == 2
    finally:
        h.close()


def test_a_set_leaf_on_an_11_bit_field(host):
    for s, seg in enumerate(host.tab.segments):
        seg["d"][5][:] %= 2048
        seg["d"][5][7] = 2047                              # (the 11-bit field's last value is held)
        host.sync(s, 0, ROWS)
    host.dt.predpack([D2, 5], sliced=True)
    wide = SET(5, list(range(0, 2048, 16)) + [1023, 2047, 2048])
    check(host, AND(wide, REL(D2, "eq", 1)), ALL, 0, 0, sliced=False, label="a set leaf on 11 bits")
    check(host, AND(SET(5, [3, 2047]), SET(D2, [1])), [D2, 5, ID], 0, 0, sliced=False, label="an 11-bit and a 2-bit set")
    # the ordinary leaves of that column run on the same planes, and so does a set leaf on the narrow one
    info, _ = check(host, AND(REL(5, "lt", 1000), REL(D2, "eq", 1)), ALL, 0, 0, sliced=True, label="11 bits, relational")
    assert 0 < info.passed_recs < info.scanned_recs
    check(host, AND(REL(5, "ge", 2047), SET(D2, [1, 3])), [D2, 5, ID], 0, 0, sliced=True, label="11 bits relational, a 2-bit set")


# ---- 7. coherence: the planes follow the journal; a value that outgrows its field sends the select back to the arenas
def test_coherence(host):
    h = host
    before, _ = check(h, C3, ALL, 0, 0, label="before")
    h.change(1, 2040, 20)                                  # (rows on both sides of a chunk's end; their filter columns cross the literals)
    h.sync(1, 2040, 20)
    changed, _ = check(h, C3, ALL, 0, 0, label="after a change of 20 rows")
    want = sum(int(c3_mask(seg, seg["size"]).sum()) for seg in h.tab.segments)
    assert changed.passed_recs == want
    h.append(2, 100)
    grown, _ = check(h, C3, ALL, 3, 0, label="after 100 appended rows")
    assert grown.scanned_recs == before.scanned_recs + 100
    check(h, C3, ALL, 0, 0, seg_rows=[ROWS, ROWS, ROWS + 37], label="a snapshot inside the appended rows")
    seg = h.tab.segments[1]
    seg["d"][D2][4100], seg["d"][D3][4100], seg["d"][D4][4100] = 1, 5000, 900
    h.sync(1, 4100, 1)
    check(h, C3, ALL, 0, 0, sliced=False, label="d3 = 5000 outgrew its field")
    info, _ = check(h, AND(REL(D2, "eq", 1), REL(D3, "ge", 5000)), ALL, 0, 0, sliced=False, label="the row that outgrew it")
    assert info.passed_recs == 1


# ---- 8. the layout budget sees the use: one per select on the planes, none for a select that reads the arenas
def test_uses_are_counted(shared):
    def uses():
        lay = [x for x in shared.dt.layouts()[0] if x.kind == capi.LAYOUT_PRED_SLICED]
        assert len(lay) == 1
        return lay[0].uses
    n = uses()
    for k in range(3):
        _, _, path = shared.dt.query_select_ex(C3[0], [ID], limit=5)
        assert path & SLICED
        assert uses() == n + k + 1
    _, _, path = shared.dt.query_select_ex(C3[0], [ID], limit=5, flags=NO_SLICED)
    assert not path & SLICED and uses() == n + 3
    got, info = shared.dt.query_select(C3[0], [ID], limit=5)              # (the older entry point takes the same path)
    assert uses() == n + 4 and info.nrows == 5 + 2
