"""Tables for the readers of the bit-sliced predicate planes at fields other than C3's (viyadb_amd/csrc/vh_bits_eval.h: vh_bits_literal,
vh_bits_lt_eq, vh_bits_eq; vh_bits_agg.h; predslice_kernel in vh_small_kernels.h; the planner's bits_prog_fill and segment_passes in
vhh_plan.h): a shape names its columns in column order — which is the order of their fields in a projection — with element types and value
ranges, so that every field's width and offset come out as SHAPES says (vh_range_bits of the recorded maximum; fields in ascending column
index; predpack_describe builds a projection of at most 32 planes that has fewer planes than 8 x the columns' bytes).

Every table is 3 segments of 5 000 mirrored rows in arrays of 8 192 — two full 2048-row chunks and one of 904, the last plane word holding 8
rows — and carries, behind the shape's own columns, a `uint` column k (0 .. 99), a `long_sum` metric v (0 .. 1000) and a count (1 .. 3): what
the aggregates group and sum that is not under test. Values are uniform in the stated range, one generator stream per segment, then planted:

  * rows 0 and 1 of segments 0 and 2 hold every column's top value and its lowest: the recorded ranges give the stated widths;
  * segment 1 holds ONE value of the shape's first filter column, its top value: whether the segment is skipped by its min / max is decided by
    the literal under test. (That column's rows of segment 1 are therefore not planted: the constant wins.)
  * for every literal of a filter column's set that a row can hold (as the element type holds it — "256" on a ubyte is 0 —, and, a decoy, its low
    `planes` bits: 2^32 + 5 on a 32-plane field is 5), and for the two neighbours of each, three rows per segment hold the value: one at bit 0 of
    a plane word, one at bit 31 of another, one among rows 4992 .. 4999. The word of 8 rows has 8 places: the held literals take them first
    (at most 7 per column here), their neighbours what is left. A row never holds a value beyond the column's stated range.

What differs from the shapes as first stated, and why:
  * the four shapes other than `values` have 32 planes in their filter projection and no room for a metric beside it, not even one of one
    plane. The aggregate on the planes keeps its values in a projection of their own, V = [v, count] (10 + 2 planes), which every shape other
    than `values` gets: the filter is read off F by the interpreter under test, the sums off V.
  * `long32`'s two columns lie in two projections (32 + 32 planes), so a filter over both has no projection that holds its columns. Its AND
    over all filter columns is therefore a DECLINED case, and the AND and the nest that must run on the planes read `l` alone.
  * no literal of these sets is refused by vo.NumType(t).parse: 2^planes and the type's maximum are in a set only "where the type holds them",
    and what is left parses. REJECTED is empty and tests/test_plane_shapes_oracle.py holds it to that.

A literal reaches the plan as the 64 bits std::sto* returned, before the C cast: the column's own type is in the low bytes, as db::AnyNum
carries it, and what lies above (256 on a ubyte, the sign extension of -1 on an int) is for the reader's element-type switch to drop.

ShapeTable is the host side alone (tests/test_plane_shapes_oracle.py checks, without a GPU, that the tables are what this says); ShapeHost
mirrors it and builds the projections with dt.predpack(cols, sliced=True)."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import viya_oracle as vo
from viyadb_amd import capi

NSEG, ROWS, CAP, CHUNK = 3, 5000, 8192, 2048
OPS = {"lt": capi.OP_LT, "le": capi.OP_LE, "gt": capi.OP_GT, "ge": capi.OP_GE, "eq": capi.OP_EQ, "ne": capi.OP_NE}
NP_OPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}
INSET_TRUTH_BITS = 10                                     # VH_INSET_TRUTH_BITS (vh_inset.h)
MAX_NV = 96                                               # VJ_MAX_NV (vh_jit.h): sum over a filter's columns of 4 x element size
COMMON_DIMS = (("k", "uint", 0, 99),)
COMMON_METS = (("v", "long_sum", 0, 1000), ("count", "count", 1, 3))
VPROJ = (("v", 10, 0), ("count", 2, 10))                  # the plane aggregate's values on the shapes whose filter projection is full


@dataclass(frozen=True)
class Shape:
    dims: Tuple[Tuple[str, str, int, int], ...]           # (name, element type, lowest, top value), in column order; k follows
    mets: Tuple[Tuple[str, str, int, int], ...] = ()      # (name, metric type, lowest, top value); v and count follow
    projs: Tuple[Tuple[Tuple[str, int, int], ...], ...] = ()      # every projection: (column, planes, offset) in field order
    filt: Tuple[str, ...] = ()                            # the filter columns; the first is constant in segment 1
    conj: Tuple[Tuple[str, str, str], ...] = ()           # the flat AND on the planes: (column, relation, literal)
    nest: Tuple[Tuple[str, str, str], ...] = ()           # (x & y) | z
    across: Tuple[Tuple[str, str, str], ...] = ()         # an AND whose columns no one projection holds (DECLINED)


SHAPES: Dict[str, Shape] = {
    "bytes": Shape(dims=(("a", "ubyte", 0, 127), ("b", "ubyte", 0, 1), ("c", "ushort", 0, 65535), ("d", "ubyte", 0, 255)),
                   projs=((("a", 7, 0), ("b", 1, 7), ("c", 16, 8), ("d", 8, 24)), VPROJ), filt=("a", "b", "c", "d"),
                   conj=(("a", "lt", "64"), ("b", "eq", "1"), ("c", "ge", "32768"), ("d", "ne", "255")),
                   nest=(("a", "lt", "64"), ("b", "eq", "1"), ("d", "eq", "255"))),
    "int31": Shape(dims=(("i", "int", 0, 2 ** 31 - 1), ("b", "ubyte", 0, 1)),
                   projs=((("i", 31, 0), ("b", 1, 31)), VPROJ), filt=("i", "b"),
                   conj=(("i", "ge", str(2 ** 30)), ("b", "eq", "1")),
                   nest=(("i", "lt", str(2 ** 30)), ("b", "eq", "1"), ("i", "eq", str(2 ** 31 - 1)))),
    "long32": Shape(dims=(("l", "long", 0, 2 ** 32 - 1), ("u", "ulong", 0, 2 ** 32 - 1)),
                    projs=((("l", 32, 0),), (("u", 32, 0),), VPROJ), filt=("l", "u"),
                    conj=(("l", "ge", str(2 ** 31)), ("l", "lt", str(2 ** 32 - 1))),
                    nest=(("l", "lt", str(2 ** 31)), ("l", "ge", "5"), ("l", "eq", str(2 ** 32 - 1))),
                    across=(("l", "ge", str(2 ** 31)), ("u", "lt", str(2 ** 31)))),
    "mixed8": Shape(dims=(("l", "long", 0, 131071), ("u", "ulong", 0, 32767)),
                    projs=((("l", 17, 0), ("u", 15, 17)), VPROJ), filt=("l", "u"),
                    conj=(("l", "lt", "65536"), ("u", "ge", "16384")),
                    nest=(("l", "lt", "65536"), ("u", "ge", "16384"), ("u", "eq", "0"))),
    "values": Shape(dims=(("f", "ushort", 0, 999), ("g", "ubyte", 3, 9), ("h", "ushort", 0, 299)),
                    mets=(("mx", "ushort_max", 0, 1023), ("sm", "int_sum", 0, 255), ("lm", "long_max", 0, 2 ** 27 - 1)),
                    projs=((("f", 10, 0),), (("g", 4, 0), ("h", 9, 4), ("mx", 10, 13), ("sm", 8, 23)), (("g", 4, 0), ("lm", 27, 4))), filt=("f",),
                    conj=(("f", "lt", "512"), ("f", "ne", "0")),
                    nest=(("f", "ge", "511"), ("f", "le", "512"), ("f", "eq", "999"))),
}

# Literals that wrap in the element type (uint-sized fields have none: nothing above the type reaches a uint's literal but "-1").
# long: 2^32 + 5 does not wrap in the type — it is what a reader that keeps 32 bits of the literal takes for 5; ulong: 2^63 is what a
# reader that decodes the literal as signed takes for a negative number.
WRAPS = {"ubyte": ("256", "383"), "ushort": ("65536", "65537"), "long": (str(2 ** 32 + 5),), "ulong": (str(2 ** 63),)}
# (shape, column) -> the literals of its set that vo.NumType(t).parse refuses, by name. None today (see the module docstring).
REJECTED: Dict[Tuple[str, str], Tuple[str, ...]] = {}


def columns(shape: str):
    """[(name, element type, lowest, top, is a dimension)] in storage order: the shape's dimensions, k, the shape's metrics, v, count."""
    sh = SHAPES[shape]
    out = [(n, t, lo, hi, True) for n, t, lo, hi in sh.dims + COMMON_DIMS]
    for n, t, lo, hi in sh.mets + COMMON_METS:
        out.append((n, "uint" if t == "count" else t.partition("_")[0], lo, hi, False))
    return out


def index_of(shape: str) -> Dict[str, int]:
    return {c[0]: i for i, c in enumerate(columns(shape))}


def column(shape: str, name: str):
    return next(c for c in columns(shape) if c[0] == name)


def planes_of(shape: str, name: str) -> int:
    return next(b for p in SHAPES[shape].projs for n, b, _ in p if n == name)


def literal_candidates(shape: str, name: str) -> List[str]:
    """The set as the rule states it, before parse has its say."""
    t, nb = column(shape, name)[1], planes_of(shape, name)
    info = np.iinfo(vo.NumType(t).dtype)
    vals = [0, 1, 2 ** (nb - 1) - 1, 2 ** (nb - 1), 2 ** nb - 2, 2 ** nb - 1] + [v for v in (2 ** nb, int(info.max)) if v <= int(info.max)]
    out = [str(v) for v in vals] + ["-1"] + ([str(int(info.min))] if info.min < 0 else []) + list(WRAPS.get(t, ()))
    return list(dict.fromkeys(out))


def literals(shape: str, name: str) -> List[str]:
    """Query strings for the column: the candidates vo.NumType(t).parse accepts (REJECTED lists the others)."""
    return [s for s in literal_candidates(shape, name) if s not in REJECTED.get((shape, name), ())]


def as_held(t: str, lit: str) -> int:
    """The literal as a value of element type t: what std::sto* and the C cast make of it."""
    return int(vo.NumType(t).parse(lit))


def planted_values(shape: str, name: str) -> Tuple[List[int], List[int]]:
    """(the held literals — as the type holds them, and the decoys: their low `planes` bits —, their neighbours), within the column's range."""
    _, t, lo, hi, _ = column(shape, name)
    nb = planes_of(shape, name)
    held: List[int] = []
    for s in literals(shape, name):
        for v in (as_held(t, s), int(s) % (1 << nb)):
            if lo <= v <= hi and v not in held:
                held.append(v)
    near: List[int] = []
    for v in held:
        for w in (v - 1, v + 1):
            if lo <= w <= hi and w not in held and w not in near:
                near.append(w)
    return held, near


def planted_rows(i: int) -> Tuple[int, int, Optional[int]]:
    """Rows of a column's i-th planted value: bit 0 of one plane word, bit 31 of another (alternating between the first two chunks), and a
    place in the word of 8 rows while there is one."""
    assert i < 24
    return 32 * (2 + 2 * i) + CHUNK * (i % 2), 32 * (3 + 2 * i) + 31 + CHUNK * ((i + 1) % 2), (ROWS - 8 + i if i < 8 else None)


def anynum(t: str, lit: str) -> capi.AnyNum:
    """The plan's literal: the 64 bits of std::sto* (the type's value in the low bytes; above them whatever the conversion left)."""
    a = capi.AnyNum()
    a.u64 = vo._stoi_family(lit, vo.NUMERIC_TYPES[t][3]) & (2 ** 64 - 1)
    return a


@dataclass
class Case:
    kind: str                     # "rel" | "in" | "inset" | "and" | "nest" | "across"
    column: Optional[str]         # the column under test (None: a composite)
    op: str                       # the relation, "in" / "not in", or ""
    lits: Tuple[str, ...]
    nodes: list                   # the plan's postfix program
    query: dict                   # the oracle's filter
    label: str


def _rel(shape, name, op, lit):
    t = column(shape, name)[1]
    return ("rel", index_of(shape)[name], OPS[op], anynum(t, lit)), {"op": op, "column": name, "value": lit}


def _set(shape, name, lits, equal, kind):
    t = column(shape, name)[1]
    f = {"op": "in", "column": name, "values": list(lits)}
    return (kind, index_of(shape)[name], equal, [anynum(t, s) for s in lits]), f if equal else {"op": "not", "filter": f}


def in_list(shape: str, name: str) -> Tuple[str, str, str]:
    """Three literals: one held, one beyond the field (where the field fills the type: a literal that wraps, or the type's minimum), one
    negative or wrapping."""
    t, nb = column(shape, name)[1], planes_of(shape, name)
    info = np.iinfo(vo.NumType(t).dtype)
    wraps = WRAPS.get(t, ())
    beyond = str(2 ** nb) if 2 ** nb <= int(info.max) else wraps[0] if wraps else str(int(info.min))
    last = "-1" if info.min < 0 or not wraps else wraps[-1]
    return str(2 ** (nb - 1) - 1), beyond, last


def composite(shape: str, which: str) -> Case:
    sh = SHAPES[shape]
    leaves = [_rel(shape, *l) for l in getattr(sh, {"and": "conj", "nest": "nest", "across": "across"}[which])]
    text = " ".join(f"{n} {op} {lit}" for n, op, lit in getattr(sh, {"and": "conj", "nest": "nest", "across": "across"}[which]))
    if which == "nest":
        x, y, z = leaves
        return Case("nest", None, "", (), [x[0], y[0], ("and", 2), z[0], ("or", 2)],
                    {"op": "or", "filters": [{"op": "and", "filters": [x[1], y[1]]}, z[1]]}, f"{shape}: (x & y) | z of {text}")
    return Case(which, None, "", (), [l[0] for l in leaves] + [("and", len(leaves))], {"op": "and", "filters": [l[1] for l in leaves]},
                f"{shape}: AND of {text}")


def column_cases(shape: str, name: str) -> List[Case]:
    """Every literal under the six relations; IN / NOT IN of three literals; the same lists as a set leaf (on the planes where the field
    has at most INSET_TRUTH_BITS planes, DECLINED on a wider one)."""
    out = []
    for lit in literals(shape, name):
        for op in OPS:
            nodes, q = _rel(shape, name, op, lit)
            out.append(Case("rel", name, op, (lit,), [nodes], q, f"{shape}: {name} {op} {lit}"))
    lits = in_list(shape, name)
    for equal in (True, False):
        for kind in ("in", "inset"):
            nodes, q = _set(shape, name, lits, equal, kind)
            out.append(Case(kind, name, "in" if equal else "not in", lits, [nodes], q, f"{shape}: {name} {'IN' if equal else 'NOT IN'} {lits} as {kind}"))
    return out


def filters(shape: str) -> List[Case]:
    sh = SHAPES[shape]
    out = [c for name in sh.filt for c in column_cases(shape, name)] + [composite(shape, "and"), composite(shape, "nest")]
    return out + ([composite(shape, "across")] if sh.across else [])


# The kinds of case the planner keeps off the planes, each with the line that says so. A declined case still runs: flags and kernel are its
# twin's, the answer the oracle's. Every other case must report that it ran on the planes.
DECLINED = {
    "a set leaf on a field wider than VH_INSET_TRUTH_BITS":
        "vhh_plan.h, QueryBuild::shape_filter: `if (ps && has_set && !sets_fit_planes(...)) ps = nullptr;` — sets_fit_planes: "
        "`if (b < 1 || b > VH_INSET_TRUTH_BITS) return false;`",
    "a filter whose columns no one projection holds":
        "vhh_plan.h, QueryBuild::shape_filter: `VhPredPack* ps = all_cols ? predpack_usable(t, pp_cols, 1) : nullptr;` — vhh_derived.h, "
        "predpack_usable: `if (!std::includes(pp->cols.begin(), pp->cols.end(), cols.begin(), cols.end())) continue;`, and no projection of l "
        "and u can be built: predpack_describe, `if (used > 32) return VH_OK;`",
}


def declined(shape: str, case: Case) -> Optional[str]:
    """The DECLINED entry the case falls under, or None: it must run on the planes."""
    if case.kind == "inset" and planes_of(shape, case.column) > INSET_TRUTH_BITS:
        return "a set leaf on a field wider than VH_INSET_TRUTH_BITS"
    if case.kind == "across":
        return "a filter whose columns no one projection holds"
    return None


class ShapeTable:
    """The oracle's table of a shape, generated and planted; `planted[column]` lists (segment, row, value)."""

    def __init__(self, name, seed=42):
        self.name, self.shape, self.seed = name, SHAPES[name], seed
        sh = self.shape
        dims = [{"name": n, "type": t} for n, t, _, _ in sh.dims + COMMON_DIMS]
        mets = [{"name": n, "type": t} for n, t, _, _ in sh.mets + COMMON_METS]
        self.tab = vo.Table({"name": "shape", "segment_size": CAP, "dimensions": dims, "metrics": mets})
        self.cols = columns(name)
        self.index = index_of(name)
        self.ndims = len(dims)
        self.planted: Dict[str, list] = {c: [] for c in sh.filt}
        for s in range(NSEG):
            d, m = self.generate(np.random.default_rng([seed, s]), CAP)
            seg = self.tab.add_segment_arrays(d, m, None, ROWS)
            arr = self.named(s)
            if s == 1:
                arr[sh.filt[0]][:] = column(name, sh.filt[0])[3]
            else:
                for n, _, lo, hi, _ in self.cols:
                    arr[n][0], arr[n][1] = hi, lo
            for c in sh.filt:
                if s == 1 and c == sh.filt[0]:
                    continue
                held, near = planted_values(name, c)
                for i, v in enumerate(held + near):
                    for row in planted_rows(i):
                        if row is not None:
                            arr[c][row] = v
                            self.planted[c].append((s, row, v))
            self.restat(seg)

    def generate(self, rng, n):
        """n rows of every column from the shape's generator: uniform in the stated ranges."""
        out = [rng.integers(lo, hi, n, endpoint=True, dtype=np.int64 if hi < 2 ** 62 else np.uint64).astype(vo.NumType(t).dtype) for _, t, lo, hi, _ in self.cols]
        return out[:self.ndims], out[self.ndims:]

    def named(self, s):
        seg = self.tab.segments[s]
        return {n: (seg["d"][i] if i < self.ndims else seg["m"][i - self.ndims]) for n, i in self.index.items()}

    def restat(self, seg):
        """SegmentStats of the rows the segment holds now (tests/test_gpu_sync_batch.restat)."""
        n = seg["size"]
        for d in self.tab.dims:
            col = seg["d"][d.index][:n]
            seg["dmax"][d.index], seg["dmin"][d.index] = col.max(), col.min()

    def query(self, flt, dims=("k",), metrics=("v", "count")):
        q = {"type": "aggregate", "table": "shape", "dimensions": list(dims), "metrics": list(metrics)}
        if flt is not None:
            q["filter"] = flt
        return q

    def want(self, flt, dims=("k",), metrics=("v", "count"), seg_rows=None):
        return vo.scan_aggregate(vo.parse_query(self.tab, self.query(flt, dims, metrics)), seg_rows=seg_rows)

    def mask(self, case_or_filter, s, rows=ROWS):
        """The rows of segment s below `rows` that pass, by the oracle's own evaluation of the filter."""
        flt = case_or_filter.query if isinstance(case_or_filter, Case) else case_or_filter
        seg = self.tab.segments[s]
        m = vo.eval_filter(self.tab, vo.make_filter(flt), lambda c: (seg["d"] if c.is_dim else seg["m"])[c.index][:rows])
        return np.ones(rows, dtype=bool) if m is None else np.asarray(m, dtype=bool)


class ShapeHost(ShapeTable):
    """The table mirrored — rows reach the device by vh_table_sync_batch from the host arrays — with its projections built."""

    def __init__(self, name, seed=42, build=True):
        super().__init__(name, seed)
        from tests.planner import col_descs
        from viyadb_amd.executor import DeviceTable
        self.dt = DeviceTable(col_descs(self.tab), CAP, reserve_segments=NSEG)
        self.dt.sync_batch([(s, 0, ROWS, ROWS, self.columns(s), 0) for s in range(NSEG)])
        for proj in (self.shape.projs if build else ()):
            before = len(self.sliced_layouts())
            self.dt.predpack([self.index[n] for n, _, _ in proj], sliced=True)
            assert len(self.sliced_layouts()) == before + 1, (name, proj)

    def sliced_layouts(self):
        return [x for x in self.dt.layouts()[0] if x.kind == capi.LAYOUT_PRED_SLICED]

    def columns(self, s):
        seg = self.tab.segments[s]
        return list(seg["d"]) + list(seg["m"])

    def sync(self, s, first, n):
        """Send rows [first, first + n) of segment s as they stand in the host arrays."""
        seg = self.tab.segments[s]
        self.restat(seg)
        self.dt.sync_batch([(s, first, n, seg["size"], self.columns(s), 0)])

    def close(self):
        self.dt.close()
