"""Tables for the clustered scan at geometries other than C3's (viyadb_amd/csrc/vh_grouped.h, group_bits_kernel, vj_scan's clustered
branch, the generator's plane map, QueryBuild::choose_grouped): a shape names its filter columns in column order — which is the order of
their fields in the bit-sliced predicate projection — with element types and value ranges, so that the grouping field's offset and width,
the number of other planes, the word group G and the sub field's offset come out as SHAPES says. The payload is C3's 29-bit record in
every shape (GROUP BY k0, k1; SUM v, COUNT) and is not under test.

Every table is 3 segments of 5 000 mirrored rows (two full tiles and one of 904) in arrays of 8 192, values uniform in the stated range
(one generator stream per segment), then planted:

  * rows 0 .. 2 n - 1 of segments 0 and 2 hold every filter column's top value and its 0, so the recorded ranges give the stated widths;
  * one in-range grouping value is held by no row (mapped to its neighbour in the whole arrays, rows to be appended included);
  * segment 1 holds the main filter's grouping value alone;
  * for every sub column, in every segment, three rows that pass the main filter's other leaves hold 0 and four hold 2^bits - 1, the last
    of them in the tile of 904 rows: both ends of the field are keys of the data.

ShapeTable is the host side alone (tests/test_cluster_shapes_oracle.py checks, without a GPU, that the tables are what this says);
ShapeHost mirrors it, with the surface of tests/test_gpu_layout_lifecycle.C3Host. ask / same_bits / four_forms / twins are the helpers of
tests/test_gpu_gplanes.py and tests/test_gpu_subsort.py with the query and the plan's payload taken from the host (`h.query`, `h.base`)."""
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

from oracle import viya_oracle as vo
from tests.parity import compare, sort_rows
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan, GroupSpec

PART, JIT, PACK = 64, capi.PLAN_FORCE_JIT, capi.PLAN_FORCE_PACK
HOT = PART | JIT | PACK
NSEG, ROWS, CAP, TILE = 3, 5000, 8192, 2048
OPS = {"lt": capi.OP_LT, "le": capi.OP_LE, "gt": capi.OP_GT, "ge": capi.OP_GE, "eq": capi.OP_EQ, "ne": capi.OP_NE}
_NP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}
PAYLOAD = (("k0", "uint", 999), ("k1", "uint", 99))          # ... and the metrics v (long_sum, 0 .. 1000) and count (1 .. 3)


@dataclass(frozen=True)
class Shape:
    cols: Tuple[Tuple[str, str, int], ...]       # the filter columns in column order: (name, element type, top value)
    v: int                                       # the main filter: g == v & the range leaves below
    leaves: Tuple[Tuple[str, str, int], ...]     # (column, relation, literal)
    bits: Dict[str, int]                         # the fields' widths
    subs: Tuple[str, ...] = ()                   # the columns a form is sub-sorted by in some case (the planner takes the first range leaf's)
    absent: Optional[Tuple[int, int]] = None     # (the grouping value no row holds, the neighbour that took its rows)
    grouped: bool = True                         # the planner's rule: g's field has at most 4 bits
    goff: int = 0                                # g's field in the row-order word
    planes: int = 0                              # the other columns' planes
    G: int = 0                                   # dwords of a word group
    sub_off: Dict[str, int] = field(default_factory=dict)      # a sub column's field in the squeezed word


SHAPES = {
    "middle": Shape(cols=(("a", "uint", 99), ("g", "ubyte", 5), ("b", "ushort", 1999)), v=2, leaves=(("a", "lt", 40), ("b", "ge", 1000)),
                    bits={"a": 7, "g": 3, "b": 11}, subs=("a", "b"), absent=(3, 4), goff=7, planes=18, G=20, sub_off={"a": 0, "b": 7}),
    "top": Shape(cols=(("a", "uint", 65535), ("b", "ushort", 4095), ("g", "ulong", 15)), v=5, leaves=(("a", "lt", 30000), ("b", "ge", 2048)),
                 bits={"a": 16, "b": 12, "g": 4}, subs=("a",), absent=(9, 10), goff=28, planes=28, G=28, sub_off={"a": 0}),
    "wide": Shape(cols=(("g", "ubyte", 1), ("a", "ushort", 32767), ("b", "uint", 65535)), v=1, leaves=(("b", "lt", 20000), ("a", "ge", 20000)),
                  bits={"g": 1, "a": 15, "b": 16}, subs=("b", "a"), goff=0, planes=31, G=32, sub_off={"b": 15, "a": 0}),
    "one": Shape(cols=(("g", "uint", 1), ("a", "uint", 1)), v=1, leaves=(("a", "lt", 1),),
                 bits={"g": 1, "a": 1}, subs=("a",), goff=0, planes=1, G=4, sub_off={"a": 0}),
    "signed": Shape(cols=(("a", "int", 999), ("g", "long", 3), ("b", "ulong", 999)), v=1, leaves=(("a", "lt", 400), ("b", "ge", 500)),
                    bits={"a": 10, "g": 2, "b": 10}, subs=("a",), absent=(2, 3), goff=10, planes=20, G=20, sub_off={"a": 0}),
    "five": Shape(cols=(("g", "uint", 16), ("a", "uint", 999)), v=3, leaves=(("a", "lt", 300),),
                  bits={"g": 5, "a": 10}, absent=(7, 8), grouped=False),
    "seventeen": Shape(cols=(("g", "uint", 3), ("w", "uint", 131071)), v=1, leaves=(("w", "lt", 26000),),
                       bits={"g": 2, "w": 17}, absent=(2, 3), goff=0, planes=17, G=20),
}


def leaf_mask(cols, leaves, n):
    """The rows below n that pass every (column, relation, literal) of `leaves`, over a segment's arrays by name."""
    m = np.ones(n, dtype=bool)
    for name, op, lit in leaves:
        m &= _NP[op](cols[name][:n].astype(np.int64), lit)
    return m


class ShapeTable:
    """The oracle's table of a shape, generated and planted; `planted[sub]` lists (segment, row, value) of the sub-field ends."""

    def __init__(self, name, seed=42):
        self.name, self.shape, self.seed = name, SHAPES[name], seed
        sh = self.shape
        dims = [{"name": n, "type": t} for n, t, _ in sh.cols + PAYLOAD]
        mets = [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}]
        self.tab = vo.Table({"name": "shape", "segment_size": CAP, "dimensions": dims, "metrics": mets})
        self.index = {n: i for i, (n, _, _) in enumerate(sh.cols + PAYLOAD)}
        self.index.update(v=len(dims), count=len(dims) + 1)
        self.planted = {s: [] for s in sh.subs}
        for s in range(NSEG):
            d, m = self.generate(np.random.default_rng([seed, s]), CAP)
            seg = self.tab.add_segment_arrays(d, m, None, ROWS)
            cols = self.named(s)
            if s == 1:
                cols["g"][:] = sh.v
            else:
                for i, (n, _, top) in enumerate(sh.cols + PAYLOAD):
                    cols[n][2 * i], cols[n][2 * i + 1] = top, 0
            reserved = 2 * len(sh.cols + PAYLOAD)
            for sub in sh.subs:
                others = [("g", "eq", sh.v)] + [l for l in sh.leaves if l[0] != sub]
                free = leaf_mask(cols, others, ROWS)
                free[:reserved] = False
                for _, row, _ in (p for q in self.planted.values() for p in q if p[0] == s):
                    free[row] = False
                at = np.flatnonzero(free)
                ends = [(int(r), 0) for r in at[:6:2]] + [(int(r), (1 << sh.bits[sub]) - 1) for r in list(at[1:6:2]) + [at[-1]]]
                for row, val in ends:
                    cols[sub][row] = val
                    self.planted[sub].append((s, row, val))
            self.restat(seg)
        self.groups = [GroupSpec(self.index["k0"]), GroupSpec(self.index["k1"])]
        self.metrics = [self.index["v"], self.index["count"]]
        self.query = {"type": "aggregate", "table": "shape", "dimensions": ["k0", "k1"], "metrics": ["v", "count"],
                      "filter": {"op": "and", "filters": [l[1] for l in self.main()]}}
        self.base = self.plan(0)

    def generate(self, rng, n):
        """n rows of every column from the shape's generator: uniform in the stated ranges, the absent grouping value mapped to its neighbour."""
        sh = self.shape
        d = [rng.integers(0, top, n, endpoint=True).astype(vo.NUMERIC_TYPES[t][0]) for _, t, top in sh.cols + PAYLOAD]
        if sh.absent:
            g = d[self.index["g"]]
            g[g == sh.absent[0]] = sh.absent[1]
        return d, [rng.integers(0, 1000, n, endpoint=True).astype(np.int64), rng.integers(1, 3, n, endpoint=True).astype(np.uint32)]

    def named(self, s):
        seg = self.tab.segments[s]
        return {n: (seg["d"][i] if i < len(seg["d"]) else seg["m"][i - len(seg["d"])]) for n, i in self.index.items()}

    def restat(self, seg):
        """SegmentStats of the rows the segment holds now (tests/test_gpu_sync_batch.restat)."""
        n = seg["size"]
        for d in self.tab.dims:
            col = seg["d"][d.index][:n]
            seg["dmax"][d.index], seg["dmin"][d.index] = col.max(), col.min()

    def rel(self, name, op, lit):
        return ("rel", self.index[name], OPS[op], lit), {"op": op, "column": name, "value": str(lit)}

    def main(self, sub=None, v=None, leaf=None):
        """The main filter's leaves: g == v first, then the range leaves — `sub`'s first of them, so that a form built for the plan is
        sub-sorted by it; `leaf` = (relation, literal) stands in for the sub column's own."""
        sh = self.shape
        rest = sorted(sh.leaves, key=lambda l: l[0] != (sub or (sh.subs[0] if sh.subs else None)))
        rest = [(n, *leaf) if leaf and n == sub else (n, op, lit) for n, op, lit in rest]
        return [self.rel("g", "eq", sh.v if v is None else v)] + [self.rel(*l) for l in rest]

    def plan(self, flags, sub=None):
        return AggPlan(filter=[l[0] for l in self.main(sub)] + [("and", 1 + len(self.shape.leaves))], groups=self.groups, metrics=self.metrics,
                       flags=flags, groups_hint=100_000)

    def want(self, leaves, seg_rows=None, node="and"):
        q = dict(self.query, filter={"op": node, "filters": [l[1] for l in leaves]})
        return vo.scan_aggregate(vo.parse_query(self.tab, q), seg_rows=seg_rows)


class ShapeHost(ShapeTable):
    """The table mirrored: rows reach the device by vh_table_sync_batch from the host arrays, as C3Host's do."""

    def __init__(self, name, seed=42):
        super().__init__(name, seed)
        from tests.planner import col_descs
        from viyadb_amd.executor import DeviceTable
        self.dt = DeviceTable(col_descs(self.tab), CAP, reserve_segments=NSEG)
        self.dt.sync_batch([(s, 0, ROWS, ROWS, self.columns(s), 0) for s in range(NSEG)])

    def columns(self, s):
        seg = self.tab.segments[s]
        return list(seg["d"]) + list(seg["m"])

    def sync(self, s, first, n):
        """Send rows [first, first + n) of segment s as they stand in the host arrays."""
        seg = self.tab.segments[s]
        self.restat(seg)
        self.dt.sync_batch([(s, first, n, seg["size"], self.columns(s), 0)])

    def regenerate(self, s, first, n, rng):
        """Rows [first, first + n) of segment s drawn again from the shape's generator (every column: the filter columns move across the literals)."""
        d, m = self.generate(rng, n)
        seg = self.tab.segments[s]
        for dst, src in zip(list(seg["d"]) + list(seg["m"]), d + m):
            dst[first:first + n] = src

    def append(self, s, n):
        seg = self.tab.segments[s]
        first = seg["size"]
        seg["size"] = first + n
        self.sync(s, first, n)

    def close(self):
        self.dt.close()


# ---- the comparisons of tests/test_gpu_gplanes.py and tests/test_gpu_subsort.py, for any host that has `tab`, `dt`, `query` and `base`
def ask(h, leaves, flags, seg_rows=None, label="", node="and"):
    filt = [l[0] for l in leaves] + [(node, len(leaves))]
    q = dict(h.query, filter={"op": node, "filters": [l[1] for l in leaves]})
    p = h.base
    res = h.dt.query_agg(AggPlan(filter=filt, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint, seg_rows=seg_rows))
    compare(res, vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows), f"{label} flags={flags:#x} snapshot={seg_rows}")
    return res


def same_bits(a, b, label):
    pa, pb = sort_rows(a.keys, a.states), sort_rows(b.keys, b.states)
    assert a.passed_recs == b.passed_recs, label
    for x, y in zip(a.keys + a.states, b.keys + b.states):
        assert x.dtype == y.dtype and x.dtype.kind in "iu" and np.array_equal(x[pa], y[pb]), label


def four_forms(h, leaves, seg_rows=None, label="", planes=True, grouped=True, extra=0):
    """`extra`: plan flags every form gets beside its own."""
    c = ask(h, leaves, HOT | extra, seg_rows, label + " clustered")
    assert c.jit and c.sliced and c.packed and c.pack_bits and c.pack_rec_bytes == 4, (label, hex(c.flags), c.kernel)
    assert c.grouped_payload == grouped and c.grouped_planes == (planes and grouped), (label, hex(c.flags))
    g = ask(h, leaves, HOT | extra | capi.PLAN_NO_GPLANES, seg_rows, label + " row-order planes")
    assert g.grouped_payload == grouped and not g.grouped_planes, (label, hex(g.flags))
    r = ask(h, leaves, HOT | extra | capi.PLAN_NO_GROUPED, seg_rows, label + " row-order records")
    assert r.packed and r.sliced and not r.grouped_payload and not r.grouped_planes, (label, hex(r.flags))
    a = ask(h, leaves, PART | JIT | extra | capi.PLAN_NO_PACK, seg_rows, label + " arenas")
    assert not a.packed and not a.grouped_payload and not a.grouped_planes, (label, hex(a.flags))
    for other, name in ((g, "row-order planes"), (r, "row-order records"), (a, "the arenas")):
        same_bits(c, other, f"{label}: clustered planes against {name}")
    return c


def twins(h, leaves, seg_rows=None, label="", trim=True, grouped=True, node="and", extra=0):
    """The query on the sub-sorted form and its VH_PLAN_NO_GROUPED twin: both against the oracle, bit for bit against each other, bit 28.
    `extra`: plan flags both legs get beside the flagship's."""
    c = ask(h, leaves, HOT | extra, seg_rows, label + " sub-sorted", node)
    assert c.jit and c.packed and c.pack_bits and c.pack_rec_bytes == 4, (label, hex(c.flags), c.kernel)
    assert c.grouped_payload == grouped and c.grouped_planes == grouped and c.sub_trimmed == (grouped and trim), (label, hex(c.flags))
    assert bool(c.flags & capi.INFO_SUBTRIM) == c.sub_trimmed
    r = ask(h, leaves, HOT | extra | capi.PLAN_NO_GROUPED, seg_rows, label + " row order", node)
    assert not r.grouped_payload and not r.grouped_planes and not r.sub_trimmed, (label, hex(r.flags))
    same_bits(c, r, label)
    return c
