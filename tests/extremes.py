"""Edge-value tables and a high-precision check of floating sums.

The typed tables of the other tests keep their values in a narrow band (dimensions in [-60, 60], floats multiples of 1/8), where every
width the planner reads off the recorded min / max is small and every float sum is exact. This module builds small tables whose values
sit at the limits of their types instead:

  integers  min, min + 1, -1, 0, 1, 2^k - 1 and 2^k for k in {7, 8, 15, 16, 31, 32, 62, 63} (clipped to the type), max - 1, max;
  floats    +-0.0, +-smallest and +-largest subnormal, +-FLT_MIN / DBL_MIN, 1 and 1 +- 1 ulp, +-FLT_MAX / DBL_MAX, +-inf and
            non-dyadic values of mixed sign and magnitude (0.1 * k), whose sums cancel.

NaN is left out on purpose. The reference updates MIN / MAX with std::min / std::max and keeps SegmentStats with the same comparisons
(its store's Metrics::Update and SegmentStats): with a NaN among the values the answer depends on the order the rows arrive in, so no
order-free answer exists to compare a GPU result with. For the same reason no test asserts the sign of a zero MIN or MAX.

edge_table() lays the rows out so that the degenerate cases are reached:
  segment 0  every dimension cycles through its type's edge set (different strides per column);
  segment 1  one value per dimension: the type's minimum for integers, -0.0 for floats;
  segment 2  one value per dimension: the type's maximum for integers, +inf for floats;
  segment 3  integers cycle again (other strides), floats hold +0.0 only.
The metrics depend on the group column `g` (its value modulo NKIND picks a kind of group, see _float_metric / _int_metric): mixed edge values,
negative floats only (the reference's float MAX identity is FLT_MIN, so these groups answer FLT_MIN), subnormals only, identity values
only, integer sums that wrap, infinities, opposite infinities (a NaN sum), and the largest finite values of the table.

check_float_sums() is the check for float SUM / AVG states: per group, |got - exact| <= gamma(n - 1) * sum(|x|) + ulp(exact) / 2, with
the exact sum taken over fractions. Every other state (keys, counts, integers, MIN / MAX) still goes through parity.compare, bit for bit.
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction

import numpy as np

from oracle import viya_oracle as vo
from tests.parity import compare

TYPES = ["byte", "ubyte", "short", "ushort", "int", "uint", "long", "ulong", "float", "double"]
INT_TYPES = TYPES[:8]
FLOAT_TYPES = ["float", "double"]
FILTERABLE = [t for t in TYPES if t not in ("byte", "short")]      # the reference cannot compile a filter on byte / short columns
AGGS = ("sum", "min", "max", "avg")
SEG_ROWS = 8192
NKIND = 8


def np_type(t: str):
    return np.dtype(vo.NUMERIC_TYPES[t][0])


def int_edges(t: str):
    info = np.iinfo(np_type(t))
    lo, hi = int(info.min), int(info.max)
    vals = {lo, lo + 1, -1, 0, 1, hi - 1, hi}
    for k in (7, 8, 15, 16, 31, 32, 62, 63):
        vals |= {(1 << k) - 1, 1 << k}
    return sorted(v for v in vals if lo <= v <= hi)


def float_specials(t: str):
    dt = np_type(t)
    fi = np.finfo(dt)
    sub_min = dt.type(fi.smallest_subnormal)
    sub_max = np.nextafter(dt.type(fi.tiny), dt.type(0))
    one = dt.type(1)
    return {"zero": dt.type(0.0), "nzero": dt.type(-0.0), "sub_min": sub_min, "sub_max": sub_max, "tiny": dt.type(fi.tiny),
            "one_dn": np.nextafter(one, dt.type(0)), "one": one, "one_up": np.nextafter(one, dt.type(2)), "max": dt.type(fi.max),
            "inf": dt.type(np.inf)}


def float_edges(t: str):
    s = float_specials(t)
    out = [s["zero"], s["nzero"], s["one_dn"], s["one"], s["one_up"], s["inf"], -s["inf"]]
    for k in ("sub_min", "sub_max", "tiny", "max"):
        out += [s[k], -s[k]]
    out += [np_type(t).type(0.1 * k) for k in (-7, -3, 1, 3, 9)]
    return out


def edges(t: str) -> np.ndarray:
    return np.array(float_edges(t), dtype=np_type(t)) if t in FLOAT_TYPES else _int_array(t, int_edges(t))


def _int_array(t, vals):
    """Python ints -> the type's array (values are in range)."""
    return np.array([int(v) for v in vals], dtype=object).astype(np_type(t))


def _tile(arr, n, stride, offset=0):
    idx = (np.arange(n, dtype=np.int64) * stride + offset) % len(arr)
    return arr[idx]


def _dim_column(t, seg, n):
    dt = np_type(t)
    strides = {t: p for t, p in zip(TYPES, (3, 5, 7, 11, 13, 17, 19, 23, 29, 31))}
    if t in FLOAT_TYPES:
        if seg == 1:
            return np.full(n, -0.0, dtype=dt)
        if seg == 2:
            return np.full(n, np.inf, dtype=dt)
        if seg == 3:
            return np.zeros(n, dtype=dt)
        return _tile(edges(t), n, strides[t])
    e = _int_array(t, int_edges(t))
    if seg == 1:
        return np.full(n, np.iinfo(dt).min, dtype=dt)
    if seg == 2:
        return np.full(n, np.iinfo(dt).max, dtype=dt)
    return _tile(e, n, strides[t], 0 if seg == 0 else 5)


def _float_metric(t, agg, kind, i, rng, first):
    """One float metric value per row of a kind of group (i: the row's index among its group's rows in this segment)."""
    dt = np_type(t)
    s = float_specials(t)
    n = len(i)
    mixed = (0.1 * (((i * 7) % 61) - 30) * 10.0 ** ((i % 5) - 2)).astype(dt)            # non-dyadic, both signs, 1e-3 .. 1e2: cancels
    if kind == 1:                                                                       # negative only: MAX answers the identity FLT_MIN
        return (-0.1 * (1 + (i % 37))).astype(dt)
    if kind == 2:                                                                       # subnormals only (sums exact in any order)
        v = (s["sub_min"] * (1 + (i % 13))).astype(dt)
        v[i % 5 == 4] = s["sub_max"]
        v[i % 11 == 10] *= -1
        return v
    if kind == 3:                                                                       # identity values (MIN: FLT_MAX, MAX: FLT_MIN)
        if agg == "min":
            return np.full(n, s["max"], dtype=dt)
        if agg == "max":
            return np.full(n, s["tiny"], dtype=dt)
        return np.where(i % 3 == 0, s["one_up"], np.where(i % 3 == 1, s["one_dn"], -s["one"])).astype(dt)
    if kind == 4:                                                                       # big and small together: catastrophic cancellation
        v = mixed.copy()
        v[i % 4 == 0] = dt.type(1e7 / 3)
        v[i % 4 == 1] = dt.type(-1e7 / 3)
        return v
    if kind == 5:                                                                       # infinities of one sign, the largest finite values
        v = mixed.copy()
        v[i % 17 == 0] = s["inf"]
        if agg in ("min", "max"):
            v[i % 17 == 1] = -s["inf"]
            v[i % 17 == 2] = s["max"]
            v[i % 17 == 3] = -s["max"]
        return v
    if kind == 6:                                                                       # opposite infinities: the sum is NaN in any order
        v = mixed.copy()
        v[i % 29 == 0] = s["inf"]
        v[i % 29 == 1] = -s["inf"]
        return v
    if kind == 7:                                                                       # tiny and one-ulp values; once per table the
        v = np.where(i % 4 == 0, s["tiny"], np.where(i % 4 == 1, -s["tiny"], np.where(i % 4 == 2, s["one_up"], s["zero"]))).astype(dt)
        if first and agg in ("sum", "avg") and n > 1:                                   # largest finite addends (Σ|x| stays below max / 2)
            v[0] = s["max"] / dt.type(4)
            v[1] = -s["max"] / dt.type(8)
        return v
    v = mixed.copy()                                                                    # kind 0: every edge value (sums: no inf, no max)
    if agg in ("min", "max"):
        return _tile(edges(t), n, 3, 1)
    v[i % 9 == 0] = s["sub_max"]
    v[i % 9 == 1] = -s["sub_min"]
    v[i % 9 == 2] = s["nzero"]
    return v


def _int_metric(t, agg, kind, i):
    dt = np_type(t)
    info = np.iinfo(dt)
    e = _int_array(t, int_edges(t))
    n = len(i)
    if kind == 3:                                                                       # identity values only
        if agg == "min":
            return np.full(n, info.max, dtype=dt)
        if agg == "max":
            return np.full(n, info.min, dtype=dt)
        return np.zeros(n, dtype=dt)
    if kind == 4 and agg in ("sum", "avg"):                                             # sums that wrap past the type's range
        return np.full(n, info.max, dtype=dt) - (i % 3).astype(dt)
    if kind == 2:
        return ((i % 5) + 1).astype(dt)
    return _tile(e, n, 3 + 2 * kind, kind)


def edge_table(nseg: int = 4, rows: int = SEG_ROWS, seg_size: int = SEG_ROWS) -> vo.Table:
    """The edge table described in the module docstring: a dimension per type, `g` (ushort), COUNT and t_sum / t_min / t_max / t_avg
    per type."""
    assert nseg <= 4 and rows <= seg_size <= 65536
    dims = [{"name": "d_" + t, "type": t} for t in TYPES] + [{"name": "g", "type": "ushort"}]
    mets = [{"name": "count", "type": "count"}] + [{"name": f"{t}_{a}", "type": f"{t}_{a}"} for t in TYPES for a in AGGS]
    tab = vo.Table({"name": "x", "segment_size": seg_size, "dimensions": dims, "metrics": mets})
    rng = np.random.default_rng(5)
    for s in range(nseg):
        g = (np.arange(rows) % (2 * NKIND)).astype(np.uint16)
        d = [_dim_column(t, s, rows) for t in TYPES] + [g]
        kind = g.astype(np.int64) % NKIND
        pos = np.arange(rows) // (2 * NKIND)                                             # the row's index among its group's rows
        m = [np.ones(rows, dtype=np.uint32)]
        for t in TYPES:
            for a in AGGS:
                col = np.zeros(rows, dtype=np_type(t))
                for k in range(NKIND):
                    sel = np.nonzero(kind == k)[0]
                    idx = pos[sel] + (g[sel] >= NKIND) * 1000
                    col[sel] = _float_metric(t, a, k, idx, rng, first=(s == 0 and k == 7)) if t in FLOAT_TYPES else _int_metric(t, a, k, idx)
                m.append(col)
        tab.add_segment_arrays(d, m, None, rows)
    return tab


# ------------------------------------------------------------------------------------------------------------------------------------
# floating sums, checked against the exact sum
# ------------------------------------------------------------------------------------------------------------------------------------
def _unit(dtype) -> Fraction:
    return Fraction(1, 1 << (24 if np.dtype(dtype).itemsize == 4 else 53))


def sum_within_bound(values: np.ndarray, got, dtype) -> (bool, str):
    """Is `got` a sum of `values` in SOME order of the state type's additions? Finite values: |got - exact| <= gamma(n - 1) * S + ulp(exact)
    / 2, with S = sum(|x|) and gamma(k) = k u / (1 - k u) (recursive summation in any order and any tree, Higham 4.2). With an infinity among
    the values the answer is order-free (S < max / 2 holds for the finite part): +inf, -inf, or NaN for both; compared exactly."""
    dtype = np.dtype(dtype)
    vals = np.asarray(values, dtype=dtype)
    got = dtype.type(got)
    pinf, ninf = bool(np.any(vals == np.inf)), bool(np.any(vals == -np.inf))
    assert not np.any(np.isnan(vals)), "NaN addends have no order-free sum"
    if pinf or ninf:
        want = dtype.type(np.nan) if pinf and ninf else dtype.type(np.inf if pinf else -np.inf)
        ok = (np.isnan(want) and np.isnan(got)) or got == want
        return ok, f"got {got!r} want {want!r} (infinite addends)"
    fin = [Fraction(float(x)) for x in vals]
    exact = sum(fin, Fraction(0))
    S = sum((abs(x) for x in fin), Fraction(0))
    fmax = Fraction(float(np.finfo(dtype).max))
    assert S < fmax / 2, "a finite group whose sum could overflow in some order: no order-free bound"
    if not np.isfinite(got):
        return False, f"got {got!r}, exact {float(exact)!r}"
    n = len(fin)
    u = _unit(dtype)
    k = max(n - 1, 0)
    gamma = k * u / (1 - k * u)
    rounded = dtype.type(float(exact))
    half_ulp = Fraction(float(np.spacing(abs(rounded)) if np.isfinite(rounded) else np.spacing(np.finfo(dtype).max))) / 2
    err = abs(Fraction(float(got)) - exact)
    bound = gamma * S + half_ulp
    return err <= bound, f"got {float(got)!r} exact {float(exact)!r} |err| {float(err):.6g} > bound {float(bound):.6g} (n={n}, S={float(S):.6g})"


def group_addends(tab: vo.Table, aq: vo.AggQuery, now=None, seg_rows=None):
    """{group key tuple: [array of the addends of metric position j] for every metric position} over the rows the query passes — the
    reference's scan (segment skipping included) without the additions."""
    out = {}
    nd = len(aq.dim_cols)
    for si, seg in enumerate(tab.segments):
        size = seg["size"] if seg_rows is None else int(seg_rows[si])
        if not vo.segment_skip(tab, aq.filter, seg):
            continue

        def getcol(c, seg=seg, size=size):
            return seg["d"][c.index][:size] if c.is_dim else seg["m"][c.index][:size]
        r = vo.eval_filter(tab, aq.filter, getcol)
        idx = np.arange(size) if r is None else np.nonzero(r)[0]
        keys = [seg["d"][oc.col.index][:size][idx] for oc in aq.dim_cols]
        vals = [seg["m"][oc.col.index][:size][idx] if not oc.col.is_dim else None for oc in aq.metric_cols]
        for row in range(len(idx)):
            key = tuple(k[row].item() for k in keys) if nd else ()
            ent = out.get(key)
            if ent is None:
                ent = out[key] = [[] for _ in aq.metric_cols]
            for j, v in enumerate(vals):
                if v is not None:
                    ent[j].append(v[row])
    return out


def float_sum_positions(aq: vo.AggQuery):
    return [j for j, oc in enumerate(aq.metric_cols) if oc.col.agg in ("sum", "avg") and oc.col.num_type.fp]


def check_float_sums(keys, states, aq, addends, label="", positions=None):
    """keys / states: a result's key columns and metric states (GPU or oracle, any row order). Every float SUM / AVG state must be a sum of
    its group's addends within sum_within_bound."""
    positions = float_sum_positions(aq) if positions is None else positions
    n = len(states[0]) if states else (len(keys[0]) if keys else 0)
    assert n == len(addends), f"{label}: {n} groups, the addends make {len(addends)}"
    for row in range(n):
        key = tuple(k[row].item() for k in keys)
        assert key in addends, f"{label}: group {key} is not the oracle's"
        for j in positions:
            vals = np.array(addends[key][j], dtype=aq.metric_cols[j].col.num_type.dtype)
            ok, why = sum_within_bound(vals, states[j][row], states[j].dtype)
            assert ok, f"{label} state[{j}] ({aq.metric_cols[j].col.name}) group {key}: {why}"


def _without(obj, positions):
    keep = [j for j in range(len(obj.states)) if j not in positions]
    return dataclasses.replace(obj, states=[obj.states[j] for j in keep]) if dataclasses.is_dataclass(obj) else obj


def compare_edges(res, st, tab, aq, label="", now=None, seg_rows=None):
    """parity.compare on everything but the float SUM / AVG states (bit for bit, as everywhere), those against the exact sums."""
    pos = float_sum_positions(aq)
    if not pos:
        compare(res, st, label)
        return
    compare(_without(res, pos), _without(st, pos), label)
    check_float_sums(res.keys, res.states, aq, group_addends(tab, aq, now, seg_rows), label, pos)


# ------------------------------------------------------------------------------------------------------------------------------------
# the query set (shared by the GPU tests and the oracle's own check against the CPU twin)
# ------------------------------------------------------------------------------------------------------------------------------------
def F(op, col, val):
    return {"op": op, "column": col, "value": str(val)}


def lit_str(t, v) -> str:
    if t in FLOAT_TYPES:
        v = float(v)
        return "-0.0" if v == 0 and math.copysign(1, v) < 0 else ("inf" if v == math.inf else "-inf" if v == -math.inf else repr(v))
    return str(int(v))


def literals(t):
    """Edge literals of type t (as query strings), plus the ones the reference wraps through stoul (256 on ubyte, -1 on uint)."""
    out = []
    for v in edges(t):
        try:
            vo.NumType(t).parse(lit_str(t, v))
        except vo.OutOfRange:          # std::stod throws on a double subnormal: the reference rejects the query
            continue
        out.append(lit_str(t, v))
    if t == "ubyte":
        out.append("256")
    if t == "uint":
        out.append("-1")
    return out


OPS = ["eq", "ne", "lt", "le", "gt", "ge", "in", "not in"]


def pred_filter(t, op, lits):
    col = "d_" + t
    if op in ("in", "not in"):
        f = {"op": "in", "column": col, "values": list(lits)}
        return f if op == "in" else {"op": "not", "filter": f}
    return F(op, col, lits[0])


def pred_query(t, op, lits):
    return {"type": "aggregate", "table": "x", "dimensions": ["g"], "metrics": ["count", "long_sum", f"{t}_max"], "filter": pred_filter(t, op, lits)}


def pred_literal_sets(t, op):
    lits = literals(t)
    if op in ("in", "not in"):
        return [lits[:3], lits[-3:], lits[len(lits) // 2:len(lits) // 2 + 2]]
    return [[x] for x in lits]


def metric_query(t, dims=("g",), filt=None, aggs=AGGS):
    q = {"type": "aggregate", "table": "x", "dimensions": list(dims), "metrics": ["count"] + [f"{t}_{a}" for a in aggs]}
    if filt is not None:
        q["filter"] = filt
    return q


# Hash keys are packed by ELEMENT width (never by recorded range), in query order, a column never straddling two 64-bit words: the
# smallest key past one word is 72 bits — 65 cannot occur.
KEY_SETS = [["d_long"], ["d_ulong"], ["d_float"], ["d_double"], ["d_byte", "d_ubyte"],
            ["d_int", "d_uint"],                         # 64 bits: exactly one word
            ["d_uint", "d_int"],                         # 64, the other order
            ["d_ulong", "d_byte"],                       # 72: the smallest two-word key
            ["d_long", "d_int", "d_ubyte"],              # 104: two words
            ["d_long", "d_int", "d_ubyte", "d_byte"]]    # 112: two words


def key_words(tab, dims):
    """64-bit words the hash path packs these key columns into (the planner's rule above)."""
    words, used = 1, 0
    for d in dims:
        bits = tab.dimension(d).num_type.size * 8
        if used + bits > 64:
            words, used = words + 1, 0
        used += bits
    return words


def key_query(dims, metrics=("count", "long_sum", "ulong_sum", "int_min", "ulong_max", "double_max", "float_min")):
    return {"type": "aggregate", "table": "x", "dimensions": list(dims), "metrics": list(metrics)}
