"""tests/plane_shapes.py without a GPU: that the tables tests/test_gpu_plane_shapes.py runs are what SHAPES claims for them — field widths
from the recorded maxima (vh_range_bits, minima >= 0), offsets in ascending column order, at most 32 planes per projection and fewer than
8 x the columns' bytes (predpack_describe), the filter's columns within VJ_MAX_NV —, that the planted rows are there at the stated bit
positions and segment 1's column is constant, and that the query set has the properties the GPU tests rely on: per column and relation
every verdict a relation can give, wrapping literals that pass exactly the rows of their wrapped value, negative literals that no row of a
signed column is below. The whole set is held against the CPU twin (oracle/cpu_twin.py), as tests/test_extremes_oracle.py holds its own.

Which verdicts a relation can give over a column that holds more than one value, every literal that fits it among them: `eq` never passes
every row and `ne` never none; `le` passes none and `gt` every row only for a literal below the lowest value, which an unsigned type does not
have (its "-1" is its maximum); `lt` passes every row and `ge` none only for a literal above the top value, which a field that fills its type
(`c`, `d`, and `i` at 2^31 - 1) does not have; `eq` passes none and `ne` every row only for a literal of either kind. Everything else must
occur, and test_every_relation_gives_every_verdict_it_can asserts the exact sets."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from oracle.cpu_twin import Twin
from tests import plane_shapes as S
from tests.parity import compare

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")
COLUMNS = [(sh, c) for sh in S.SHAPES for c in S.SHAPES[sh].filt]
_tables = {}


def table_of(name):
    if name not in _tables:
        _tables[name] = S.ShapeTable(name)
    return _tables[name]


@pytest.fixture(scope="module", params=list(S.SHAPES))
def table(request):
    return table_of(request.param)


def range_bits(lo, hi):                 # vh_range_bits: 0 = no field (a negative value)
    return 0 if lo < 0 else max(1, int(hi).bit_length())


def narrow_width(t, hi):                # vh_range_narrow_width: what a uint column's narrow copy would take
    return 0 if t != "uint" else 1 if hi < 256 else 2 if hi < 65536 else 0


def recorded(table, name):
    """(lowest, top) of the column over the rows the segments hold; a dimension's from the recorded SegmentStats."""
    i = table.index[name]
    if i < table.ndims:
        return (min(int(seg["dmin"][i]) for seg in table.tab.segments), max(int(seg["dmax"][i]) for seg in table.tab.segments))
    return (min(int(table.named(s)[name][:S.ROWS].min()) for s in range(S.NSEG)), max(int(table.named(s)[name][:S.ROWS].max()) for s in range(S.NSEG)))


def test_field_widths_offsets_and_the_build_rule(table):
    sh = table.shape
    for n, t, lo, hi, _ in table.cols:
        assert recorded(table, n) == (lo, hi), n
    for proj in sh.projs:
        idx = [table.index[n] for n, _, _ in proj]
        assert idx == sorted(idx) and len(set(idx)) == len(idx), proj          # fields lie in ascending column index
        used = plain = 0
        for n, bits, off in proj:
            _, t, lo, hi, _ = S.column(table.name, n)
            assert range_bits(*recorded(table, n)) == bits and off == used, (n, bits, off, used)
            used += bits
            plain += narrow_width(t, hi) or vo.NumType(t).size
        assert used <= 32 and used < 8 * plain, (proj, used, plain)            # predpack_describe builds it
    for n in sh.filt:
        assert any(n in [c for c, _, _ in p] for p in sh.projs)
    for leaves in (sh.conj, sh.nest, sh.across, *[((n, "eq", "0"),) for n in sh.filt]):
        cols = {n for n, _, _ in leaves}
        assert sum(4 * vo.NumType(S.column(table.name, n)[1]).size for n in cols) <= S.MAX_NV, leaves
    for which in ("conj", "nest"):                                             # one projection holds every column of the filters that must run on the planes
        cols = {n for n, _, _ in getattr(sh, which)}
        assert any(cols <= {c for c, _, _ in p} for p in sh.projs), which
    if sh.across:
        cols = {n for n, _, _ in sh.across}
        assert not any(cols <= {c for c, _, _ in p} for p in sh.projs)
        assert sum(S.planes_of(table.name, n) for n in cols) > 32               # ... and none could: predpack_describe declines more than 32 planes


def test_the_stated_geometry():
    """What the shapes are for, restated from the issue's table."""
    want = {"bytes": {"a": (7, 0), "b": (1, 7), "c": (16, 8), "d": (8, 24)}, "int31": {"i": (31, 0), "b": (1, 31)},
            "mixed8": {"l": (17, 0), "u": (15, 17)}}
    for name, fields in want.items():
        assert {n: (b, o) for n, b, o in S.SHAPES[name].projs[0]} == fields
    assert [p for p in S.SHAPES["long32"].projs[:2]] == [(("l", 32, 0),), (("u", 32, 0),)]
    f, v1, v2 = S.SHAPES["values"].projs
    assert f == (("f", 10, 0),) and [(n, b) for n, b, _ in v1] == [("g", 4), ("h", 9), ("mx", 10), ("sm", 8)] and [(n, b) for n, b, _ in v2] == [("g", 4), ("lm", 27)]
    types = {(sh, n): t for sh in S.SHAPES for n, t, _, _, _ in S.columns(sh)}
    assert types[("bytes", "c")] == "ushort" and types[("int31", "i")] == "int" and types[("long32", "l")] == "long" and types[("long32", "u")] == "ulong"
    assert types[("values", "mx")] == "ushort" and types[("values", "sm")] == "int" and types[("values", "lm")] == "long" and types[("values", "g")] == "ubyte"
    assert (9 - 3 + 1, (9 - 3 + 1) * 300) == (7, 2100)                         # ids of GROUP BY g (the loop sink) and of (g, h) (the row sink)


def test_planted_rows(table):
    sh = table.shape
    assert [seg["size"] for seg in table.tab.segments] == [S.ROWS] * S.NSEG and S.ROWS - 2 * S.CHUNK == 904 and S.ROWS % 32 == 8
    first = sh.filt[0]
    assert (table.named(1)[first] == S.column(table.name, first)[3]).all()      # segment 1 holds the first filter column's top value alone
    for c in sh.filt:
        held, near = S.planted_values(table.name, c)
        assert len(held) <= 8 and len(held) + len(near) <= 24, (c, held, near)
        _, t, lo, hi, _ = S.column(table.name, c)
        for lit in S.literals(table.name, c):                                   # every literal a row can hold is held
            assert not lo <= S.as_held(t, lit) <= hi or S.as_held(t, lit) in held, (c, lit)
        for s in range(S.NSEG):
            mine = [(row, v) for seg, row, v in table.planted[c] if seg == s]
            if s == 1 and c == first:
                assert not mine
                continue
            arr = table.named(s)[c]
            assert all(int(arr[row]) == v for row, v in mine), (c, s)
            for i, v in enumerate(held + near):
                rows = [row for row, w in mine if w == v]
                assert len(rows) == (3 if i < 8 else 2) and min(rows) >= 32, (c, v, rows)
                assert rows[0] % 32 == 0 and rows[1] % 32 == 31 and rows[0] // 32 != rows[1] // 32 and max(rows[:2]) < 2 * S.CHUNK, (c, v, rows)
                assert i >= 8 or S.ROWS - 8 <= rows[2] < S.ROWS, (c, v, rows)
            assert sorted({row // S.CHUNK for row, _ in mine}) == [0, 1, 2]      # all three chunks hold planted rows


def test_no_literal_is_left_out_silently():
    found = {}
    for sh, c in COLUMNS:
        t = S.column(sh, c)[1]
        bad = []
        for lit in S.literal_candidates(sh, c):
            try:
                vo.NumType(t).parse(lit)
            except vo.InvalidArgument:
                bad.append(lit)
        if bad:
            found[(sh, c)] = tuple(bad)
        assert len(S.literals(sh, c)) >= 8 or S.planes_of(sh, c) == 1, (sh, c, S.literals(sh, c))
    assert found == S.REJECTED
    assert set(S.literals("bytes", "a")) >= {"0", "1", "63", "64", "126", "127", "128", "255", "-1", "256", "383"}
    assert set(S.literals("int31", "i")) >= {str(2 ** 30 - 1), str(2 ** 30), str(2 ** 31 - 2), str(2 ** 31 - 1), "-1", str(-2 ** 31)}
    assert set(S.literals("long32", "l")) >= {str(2 ** 32 - 1), str(2 ** 32), str(2 ** 63 - 1), "-1", str(-2 ** 63), str(2 ** 32 + 5)}
    assert set(S.literals("long32", "u")) >= {str(2 ** 32 - 1), str(2 ** 32), str(2 ** 64 - 1), "-1", str(2 ** 63)}


def int_mask(col, op, w):
    """(col op w) for a column of values below 2^62 and any Python integer w."""
    if abs(w) >= 2 ** 62:
        below = w < 0                                                          # the literal lies below every value / above every value
        return np.full(len(col), {"eq": False, "ne": True, "lt": not below, "le": not below, "gt": below, "ge": below}[op])
    return S.NP_OPS[op](col.astype(np.int64), np.int64(w))


def passing(table, flt):
    return [table.mask(flt, s) for s in range(S.NSEG)]


@pytest.mark.parametrize("sh, c", COLUMNS, ids=lambda x: x)
def test_every_relation_gives_every_verdict_it_can(sh, c):
    table = table_of(sh)
    signed = np.iinfo(vo.NumType(S.column(sh, c)[1]).dtype).min < 0
    seen = {op: set() for op in S.OPS}
    for case in S.column_cases(sh, c):
        if case.kind != "rel":
            continue
        st = table.want(case.query)
        seen[case.op].add("none" if st.passed_recs == 0 else "all" if st.passed_recs == S.NSEG * S.ROWS else "some")
    above = {"x"} if S.column(sh, c)[3] < np.iinfo(vo.NumType(S.column(sh, c)[1]).dtype).max else set()      # the type has a value above the column's top
    below = {"x"} if signed else set()                                                                        # ... below its lowest
    pick = lambda verdict, when: {verdict} if when else set()
    can = {"eq": {"some"} | pick("none", above or below), "ne": {"some"} | pick("all", above or below),
           "lt": {"some", "none"} | pick("all", above), "ge": {"some", "all"} | pick("none", above),
           "le": {"some", "all"} | pick("none", below), "gt": {"some", "none"} | pick("all", below)}
    assert seen == can, (sh, c, seen)


@pytest.mark.parametrize("sh, c", COLUMNS, ids=lambda x: x)
def test_wrapping_and_negative_literals(sh, c):
    """A literal passes exactly the rows its value in the element type passes, row by row against plain integer comparisons: "256" on a
    ubyte is 0, "-1" on an unsigned type its maximum, a negative literal of a signed type lies below every row, 2^32 + 5 on a long is not 5."""
    table = table_of(sh)
    _, t, lo, hi, _ = S.column(sh, c)
    info = np.iinfo(vo.NumType(t).dtype)
    checked = 0
    for lit in S.literals(sh, c):
        w = S.as_held(t, lit)
        assert int(info.min) <= w <= int(info.max)
        special = w != int(lit) or w < 0 or lit in S.WRAPS.get(t, ())
        for op in S.OPS:
            flt = {"op": op, "column": c, "value": lit}
            got = passing(table, flt)
            for s in range(S.NSEG):
                assert np.array_equal(got[s], int_mask(table.named(s)[c][:S.ROWS], op, w)), (sh, c, op, lit, s)
            n = sum(int(m.sum()) for m in got)
            if w < 0:
                assert n == (0 if op in ("eq", "lt", "le") else S.NSEG * S.ROWS), (sh, c, op, lit, n)
            if w != int(lit) and op == "eq":
                assert (n > 0) == (lo <= w <= hi), (sh, c, lit, w, n)          # a wrapped literal that lands in the range meets its planted rows
        checked += special
    assert checked >= (1 if t in ("uint",) else 2), (sh, c, checked)
    nb = S.planes_of(sh, c)
    for lit in S.literals(sh, c):                                              # the decoys: the literal's low `planes` bits are held, the literal is not
        w, low = S.as_held(t, lit), int(lit) % (1 << nb)
        if w != low and lo <= low <= hi and not lo <= w <= hi:
            assert table.want({"op": "eq", "column": c, "value": lit}).passed_recs == 0
            assert table.want({"op": "eq", "column": c, "value": str(low)}).passed_recs > 0, (sh, c, lit, low)


def test_a_decoy_for_every_truncation():
    """The literals whose low bits a reader could mistake for a held value: each shape's wide columns have one."""
    for sh, c, lit, low in (("long32", "l", str(2 ** 32 + 5), 5), ("long32", "u", str(2 ** 63), 0), ("bytes", "a", "128", 0), ("int31", "i", "-1", 2 ** 31 - 1),
                            ("mixed8", "l", str(2 ** 32 + 5), 5), ("values", "f", "1024", 0)):
        t = S.column(sh, c)[1]
        assert int(lit) % (1 << S.planes_of(sh, c)) == low and S.as_held(t, lit) != low
        assert low in S.planted_values(sh, c)[0]


def test_segment_one_is_skipped_by_the_literal(table):
    c = table.shape.filt[0]
    top = S.column(table.name, c)[3]
    assert table.want({"op": "eq", "column": c, "value": str(top)}).scanned_segments == S.NSEG
    assert table.want({"op": "eq", "column": c, "value": "0"}).scanned_segments == S.NSEG - 1
    assert table.want({"op": "lt", "column": c, "value": str(top)}).scanned_segments == S.NSEG       # (the reference skips on dmin <= literal)
    assert table.want({"op": "le", "column": c, "value": str(top - 1)}).scanned_segments == S.NSEG - 1
    assert table.want(S.composite(table.name, "and").query).passed_recs > 0


def test_composites_pass_some_rows(table):
    for which in ("and", "nest") + (("across",) if table.shape.across else ()):
        case = S.composite(table.name, which)
        st = table.want(case.query)
        print(f"{case.label}: {st.passed_recs} of {st.scanned_recs} rows, {st.scanned_segments} segments")
        assert 0.01 < st.passed_recs / st.scanned_recs < 0.75, case.label
        per_word = [int(table.mask(case, 0)[:32].sum()), int(table.mask(case, 0)[:S.CHUNK].sum()), int(table.mask(case, 0).sum())]
        assert per_word[0] < per_word[1] < per_word[2]                         # the select's windows at the word's, the chunk's and the segment's survivors differ


@pytest.mark.parametrize("sh, c", COLUMNS + [(sh, None) for sh in S.SHAPES], ids=lambda x: x or "composites")
def test_the_query_set_against_the_cpu_twin(sh, c):
    """One twin per filter shape (literals are arguments, not part of the compiled text); every case of the set through it."""
    table = table_of(sh)
    cases = [x for x in S.filters(sh) if x.column == c and x.kind != "inset"]      # (a set leaf is the IN list's query)
    assert cases
    for case in cases:
        q = table.query(case.query)
        st = vo.scan_aggregate(vo.parse_query(table.tab, q))
        got = Twin(table.tab, q).run()
        got.passed_recs = st.passed_recs                                        # (the twin keeps no such counter)
        compare(got, st, case.label)
