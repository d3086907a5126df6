"""Device top-N (topk_keys / topk_hist / topk_pick / topk_compact, viyadb_amd/csrc/vh_topk_key.h) at value extremes,
ties and formatter-equal floats, through the C ABI and end to end, judged by the oracle alone.

The contract is a SUPERSET: no group that the reference could place inside the first `skip + limit` rows may be dropped — the
host only ever sees what the device kept. Per case: format every group's sort value with oracle.viya_oracle.fmt_num, order with
_cmp_strings (pinned by tests/test_numcmp_golden.py); `required` = every group that is not strictly worse than the K-th. Then
  (a) required is a subset of the returned ids;  (b) no id twice, returned == len(ids), ngroups == the oracle's;
  (c) every kept row carries the oracle's keys and states bit for bit, hidden count included;
  (d) nothing is over-kept without cause: the returned set IS `required` for integers of at most 17 digits and for float values
      outside the crafted clusters; otherwise at most the groups of the K-th value's own crafted cluster come on top (a count from
      the table's construction, not from the key function). Filler values lie far from every crafted one: integers in another
      digit class, floats on a coarse grid whose points are >= 2^20 ulps from each other and from every crafted value (so that
      filler rows tie exactly or not at all).

One row per `id`, so that a group's MAX / MIN / SUM is exactly the crafted number.

Kept out of every sorted query: NaN (the reference's std::sort comparator is then no strict order), sub-normal doubles, and
DBL_MIN / DBL_MAX: std::stod throws on their "%.15g" text, which the oracle models (tests/test_numcmp_golden.py). The last two are
the identities of a double MAX / MIN (store.cc:107-110), so a double MAX column holds positive values only here and a double MIN
column no +inf; the dimension and the SUM carry both signs, both zeros and both infinities."""
import dataclasses

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.planner import capi_anynum, mirror_table, plan_from_query

pytestmark = pytest.mark.gpu
NOW = 1496570140
N = 72_000                      # ids = groups; two ragged segments
SEG_ROWS = (41_000, 31_000)
HINT = 100_000                  # keeps the hash table, hence the output arrays, above the 65 536 rows from which top-N is active
INT_TYPES = ["byte", "ubyte", "short", "ushort", "int", "uint", "long", "ulong"]
FLOAT_TYPES = ["float", "double"]
DBL_TEXT_MAX = float("1.79769313486231e+308")      # the largest "%.15g" text that std::stod reads
RADIX_CENTRES = (256 * 500, 65536 * 3, 65536 * 256 * 2)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _dt(t):
    return np.dtype(vo.NUMERIC_TYPES[t][0])


# ------------------------------------------------------------------------------------------------------------- crafted values
def _place(rng, n, filler, crafted):
    """n values: `crafted` (a list of (values, cluster id or -1)) at random ids, `filler` elsewhere. -> values, cluster per id."""
    vals = filler.copy()
    cluster = np.full(n, -1, dtype=np.int64)
    total = sum(len(v) for v, _ in crafted)
    assert total <= n
    ids = rng.permutation(n)[:total]
    o = 0
    for v, c in crafted:
        vals[ids[o:o + len(v)]] = v
        cluster[ids[o:o + len(v)]] = c
        o += len(v)
    return vals, cluster


def int_column(t, rng):
    """Digit-class edges, the type's extremes, radix-byte boundaries, and for 64-bit types runs of 130 neighbours in the 18-, 19-
    and 20-digit classes (each run a cluster: its keys drop the low 6 bits); filler with at most 16 digits for those."""
    dt = _dt(t)
    info = np.iinfo(dt)
    edges = {0, info.min, info.max}
    d = 0
    while 10 ** d <= info.max:
        for m in (10 ** d, 10 ** (d + 1) - 1):
            edges.update(v for v in (m, -m) if info.min <= v <= info.max)
        d += 1
    crafted = [(np.array(sorted(edges), dtype=object).astype(dt), -1)]
    if info.bits >= 32:          # consecutive values around multiples of 256, 65536 and 2^25, inside one digit class
        for centre in RADIX_CENTRES:
            crafted.append((np.arange(centre - 40, centre + 41).astype(dt), -1))
    if info.bits == 64:
        c = 0
        for nd in (18, 19, 20):
            lo, hi = 10 ** (nd - 1), min(10 ** nd - 1, info.max)
            if lo > info.max:
                continue
            for start in (lo, lo + (hi - lo) // 3 * 2 + 37, hi - 129):
                run = np.array(list(range(start, start + 130)), dtype=object)
                crafted.append((run.astype(dt), c))
                if info.min < 0:
                    crafted.append(((-run).astype(dt), c + 1))
                c += 2
        if info.min < 0:          # INT64_MIN and its neighbours: next to -(INT64_MAX - 129 .. INT64_MAX), the run before — one cluster
            crafted.append((np.array(list(range(info.min, info.min + 130)), dtype=object).astype(dt), c - 1))
        filler = (rng.integers(0, 10 ** 16, N) * (rng.choice([-1, 1], N) if info.min < 0 else 1)).astype(dt)
    else:
        filler = rng.integers(info.min, info.max, N, endpoint=True).astype(dt)
    return _place(rng, N, filler, crafted)


def same_text_run(x, dt):
    """Every value of the type that prints the text of x, plus the first value on either side (which prints another)."""
    x = dt.type(x)
    text = vo.fmt_num(x)
    down, up = dt.type(-np.inf), dt.type(np.inf)
    lo = x
    while vo.fmt_num(np.nextafter(lo, down)) == text:
        lo = np.nextafter(lo, down)
    run = [np.nextafter(lo, down), lo]
    while vo.fmt_num(run[-1]) == text:
        run.append(np.nextafter(run[-1], up))
    return np.array(run, dtype=dt)


def float_grid(dt):
    return np.unique(np.array([s * u * 10.0 ** e for s in (-1, 1) for u in (2, 3, 4, 5, 6, 7) for e in range(-3, 16)]).astype(dt))


def float_column(t, rng, ties=0):
    """Runs of values that print one text ("%.15g": up to 87 ulps wide, "%g": up to 163) just above each power of ten 10^-3..10^15
    with the neighbour on either side, both signs (each run a cluster); +-0 five times each, +-inf, the largest values; `ties`
    groups sharing 2.5; filler from a coarse grid."""
    dt = _dt(t)
    head = "1.00000000000001" if t == "double" else "1.00001"
    crafted = []
    widest = 0
    for c, e in enumerate(range(-3, 16)):
        run = same_text_run(float("%se%d" % (head, e)), dt)
        widest = max(widest, len(run) - 2)
        crafted += [(run, 2 * c), (-run, 2 * c + 1)]
    assert widest == (88 if t == "double" else 164)          # 87 / 163 ulps between the ends of the widest run
    big = [DBL_TEXT_MAX, -DBL_TEXT_MAX] if t == "double" else [np.finfo(np.float32).max, -np.finfo(np.float32).max]
    crafted.append((np.array([0.0] * 5 + [-0.0] * 5, dtype=dt), -1))
    crafted.append((np.array([np.inf, np.inf, big[0]], dtype=dt), 102))          # the largest finite value is inf's neighbour in bit patterns
    crafted.append((np.array([-np.inf, big[1]], dtype=dt), 103))
    if t == "float":          # neighbours that print different texts: where "%g" turns to 1e+06, and where floats stop holding odd integers
        crafted.append((np.array([999999.5, 999999.4375, 999999.375], dtype=dt), 100))
        crafted.append((np.array([2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2], dtype=dt), 101))
    if ties:
        crafted.append((np.full(ties, 2.5, dtype=dt), -1))
    grid = float_grid(dt)
    return _place(rng, N, grid[rng.integers(0, len(grid), N)], crafted)


class Family:
    """An oracle table and its device mirror: dimension `id` (one row each), per type a dimension d_<t> and metrics <t>_max / _min
    / _sum (/ _avg) holding the same crafted column — for a float type's MAX without what is not positive, for its MIN without +inf
    (2.0, a filler value, stands there instead: see the module's text)."""

    def __init__(self, types, seed, n=N, seg_rows=SEG_ROWS, columns=None, hidden_count=False, extra_metrics=()):
        rng = np.random.default_rng(seed)
        self.n, self.types, self._cols = n, types, {}
        for t in types:
            if columns:
                self._cols[t] = columns[t]
            elif t in FLOAT_TYPES:
                self._cols[t] = float_column(t, rng, ties=40_000 if t == "double" else 0)
            else:
                self._cols[t] = int_column(t, rng)
        dims = [{"name": "id", "type": "uint"}] + [{"name": "d_" + t, "type": t} for t in types] + [{"name": "sel", "type": "ushort"}]
        # `sel < 1`, `< 2`, `< 3` let 10, 100 and 66 000 ids through, spread over the whole id range (no segment, no id range drops out)
        self.sel = np.full(n, 3, dtype=np.uint16)
        perm = rng.permutation(n)
        self.sel[perm[:66_000]], self.sel[perm[:100]], self.sel[perm[:10]] = 2, 1, 0
        mets = [] if hidden_count else [{"name": "count", "type": "count"}]
        self.aggs = ("max", "min", "sum") + tuple(extra_metrics)
        for t in types:
            mets += [{"name": f"{t}_{a}", "type": f"{t}_{a}"} for a in self.aggs]
        self.tab = vo.Table({"name": "t", "segment_size": max(seg_rows) + 9_000, "dimensions": dims, "metrics": mets})
        self.counts = rng.integers(1, 6, n).astype(np.uint32)          # the `count` metric's column (or the hidden count)
        o = 0
        for rows in seg_rows:
            sl = slice(o, o + rows)
            d = [np.arange(o, o + rows, dtype=np.uint32)] + [self.col(t, "dim")[0][sl] for t in types] + [self.sel[sl]]
            m = [] if hidden_count else [self.counts[sl]]
            for t in types:
                m += [self.col(t, a)[0][sl] for a in self.aggs]
            self.tab.add_segment_arrays(d, m, self.counts[sl].astype(np.uint64) if hidden_count else None, rows)
            o += rows
        assert o == n
        self.dt = mirror_table(self.tab)
        self._scans, self._ranks = {}, {}

    def col(self, t, source):
        """-> (values, cluster) of type t's column as `source` (dim / max / min / sum / avg) holds it, by id."""
        v, c = self._cols[t]
        if t in FLOAT_TYPES and source in ("max", "min"):
            keep = v > 0 if source == "max" else ~(np.isinf(v) & (v > 0))
            return np.where(keep, v, v.dtype.type(2.0)), np.where(keep, c, -1)
        return v, c

    def close(self):
        self.dt.close()

    def scan(self, dims, metrics, flt=None):
        key = (tuple(dims), tuple(metrics), repr(flt))
        if key not in self._scans:
            q = {"type": "aggregate", "table": "t", "dimensions": list(dims), "metrics": list(metrics)}
            if flt:
                q["filter"] = flt
            aq = vo.parse_query(self.tab, q)
            self._scans[key] = (aq, vo.scan_aggregate(aq, now=NOW))
        return self._scans[key]

    def ranks(self, dims, metrics, top_col, flt=None):
        key = (tuple(dims), tuple(metrics), top_col, repr(flt))
        if key not in self._ranks:
            _, st = self.scan(dims, metrics, flt)
            self._ranks[key] = reference_ranks((list(st.keys) + list(st.states))[top_col])
        return self._ranks[key]


@pytest.fixture(scope="module")
def ints():
    f = Family(INT_TYPES, seed=11)
    yield f
    f.close()


@pytest.fixture(scope="module")
def floats():
    f = Family(FLOAT_TYPES, seed=12, hidden_count=True, extra_metrics=("avg",))
    yield f
    f.close()


# ------------------------------------------------------------------------------------------------------------ the oracle's side
def reference_ranks(vals):
    """Dense rank per value in the reference's ASCENDING order (equal rank: neither is smaller), from fmt_num and _cmp_strings:
    values are ordered by what the comparator compares (stod of the text / length, then text), and the comparator itself then
    confirms the order between all neighbours — which, for a strict weak order, confirms all of it."""
    vals = np.ascontiguousarray(vals)
    is_f = vals.dtype.kind == "f"
    uniq, inv = np.unique(vals.view("u%d" % vals.dtype.itemsize) if is_f else vals, return_inverse=True)      # bit patterns: -0 and +0 stay apart
    texts = [vo.fmt_num(v) for v in (uniq.view(vals.dtype) if is_f else uniq)]
    ks = [vo._stod(s) for s in texts] if is_f else [(len(s), s) for s in texts]
    order = sorted(range(len(ks)), key=lambda i: ks[i])
    lt = vo._cmp_strings("float" if is_f else "integer", True)
    gt = vo._cmp_strings("float" if is_f else "integer", False)
    rank_u = np.zeros(len(ks), dtype=np.int64)
    r = 0
    for a, b in zip(order, order[1:]):
        assert not lt(texts[b], texts[a]) and not gt(texts[a], texts[b])
        up = lt(texts[a], texts[b])
        assert up == gt(texts[b], texts[a])
        r += up
        rank_u[b] = r
    return rank_u[inv.reshape(-1)]


def k_at(ranks, i, desc):
    """The K for which group i ties with the K-th: 1 + the groups strictly better than it."""
    return 1 + int((ranks > ranks[i]).sum() if desc else (ranks < ranks[i]).sum())


_OPS = {"lt": (np.less, 2), "le": (np.less_equal, 3), "gt": (np.greater, 4), "ge": (np.greater_equal, 5)}


def check_top_n(fam, dims, metrics, top_col, desc, k, cluster=None, flags=0, flt=None, having=None):
    """Runs one top-N plan and holds it to (a)-(d). `having`: (result column, op name, value) — numeric, applied to the oracle's
    groups before ranking. Returns (kept ids, required ids, the oracle's groups)."""
    aq, st = fam.scan(dims, metrics, flt)
    cols = list(st.keys) + list(st.states)
    names = [oc.col.name for oc in aq.dim_cols] + [oc.col.name for oc in aq.metric_cols]
    vals = cols[top_col]
    alive = np.ones(st.ngroups, dtype=bool)
    plan = plan_from_query(fam.tab, aq, now=NOW, flags=flags, groups_hint=HINT)
    if having:
        hc, op, hv = having
        alive = _OPS[op][0](cols[hc], hv)
        plan.having = [("rel", hc, _OPS[op][1], capi_anynum(fam.tab.column(names[hc]), hv))]
    plan = dataclasses.replace(plan, top=(top_col, desc, k))
    res = fam.dt.query_agg(plan)
    ids = st.keys[0]
    live = np.nonzero(alive)[0]
    lr = fam.ranks(dims, metrics, top_col, flt)[live]
    kth_cluster = -1
    if k >= len(live):
        required = live
    else:
        kth = np.sort(lr)[::-1][k - 1] if desc else np.sort(lr)[k - 1]
        required = live[lr >= kth] if desc else live[lr <= kth]
        if cluster is not None:
            kth_cluster = int(cluster[ids[live[lr == kth]]].max())
    got = np.asarray(res.keys[0]).astype(np.int64)
    label = (dims, metrics, top_col, "desc" if desc else "asc", k, flags, flt, having)
    print("top-N %s: groups %d, alive %d, required %d, returned %d" % (label, st.ngroups, len(live), len(required), res.returned))
    # (b)
    assert res.ngroups == st.ngroups, label
    assert res.returned == len(got) and len(np.unique(got)) == len(got), label
    # (a)
    missing = np.setdiff1d(ids[required].astype(np.int64), got)
    assert len(missing) == 0, (label, "dropped %d required groups, e.g. ids %s with values %s" % (
        len(missing), missing[:5], [vo.fmt_num(v) for v in vals[np.isin(ids, missing[:5])]]))
    # (c)
    pos = np.full(max(int(ids.max()), int(got.max())) + 1, -1, dtype=np.int64)
    pos[ids] = np.arange(len(ids))
    idx = pos[got]
    assert (idx >= 0).all() and alive[idx].all(), label
    for j, (a, b) in enumerate(zip(list(res.keys) + list(res.states), cols)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b[idx])
        if a.dtype != b.dtype and a.dtype.kind == b.dtype.kind and a.dtype.kind in "iu":
            b = b.astype(a.dtype)
        assert a.dtype == b.dtype, (label, j, a.dtype, b.dtype)
        bits = "u%d" % a.dtype.itemsize
        same = a.view(bits) == b.view(bits)
        if a.dtype.kind == "f" and (j < len(st.keys) or names[j].endswith(("_sum", "_avg"))):
            # the sign of a zero is pinned for MAX / MIN states only: a running sum from +0.0 turns -0.0 into +0.0 where the oracle's
            # reduceat keeps it, and a float group key's -0.0 == 0.0 (KeyEqual compares field-wise), which the device stores as +0.0
            same |= (a == 0) & (b == 0)
        assert same.all(), (label, "column %d (%s)" % (j, names[j]), a[~same][:3], b[~same][:3])
    if st.hidden_count is not None:
        assert res.hidden_count is not None and np.array_equal(np.asarray(res.hidden_count), st.hidden_count[idx]), label
    # (d)
    extra = int((cluster[ids[live]] == kth_cluster).sum()) if kth_cluster >= 0 else 0
    assert len(got) <= len(required) + extra, (label, len(got), len(required), extra)
    if kth_cluster < 0:
        assert len(got) == len(required), (label, len(got), len(required))
    if len(required) + extra < st.ngroups and st.ngroups > 65536:
        assert res.returned < res.ngroups, label          # top-N ran on the device
    return got, ids[required], st


def _source(t, source, second="count"):
    """-> dims, metrics, top_col for sorting on type t's crafted column as a metric or as a dimension."""
    if source == "dim":
        return ["id", "d_" + t], [second], 1
    return ["id"], [f"{t}_{source}", second], 1


KS = (1, 2, 10, 1000, N - 1, N, N + 1, 10 * N)


# ----------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("source", ["max", "min", "dim"])
@pytest.mark.parametrize("t", INT_TYPES)
def test_integer_types_and_sources(ints, t, source, desc):
    """Every integer type as MAX / MIN metric and as a dimension (topk_src_is_key), both directions, K from 1 to beyond n. From n
    on every row comes back."""
    dims, metrics, col = _source(t, source)
    for k in KS:
        got, req, st = check_top_n(ints, dims, metrics, col, desc, k, cluster=ints.col(t, source)[1])
        assert k < N or len(got) == N


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("source", ["max", "min", "sum", "dim"])
@pytest.mark.parametrize("t", FLOAT_TYPES)
def test_float_types_and_sources(floats, t, source, desc):
    """The same for float and double, on a table whose AVG metric brings the hidden count along."""
    dims, metrics, col = _source(t, source, second=t + "_avg")
    for k in KS:
        got, req, st = check_top_n(floats, dims, metrics, col, desc, k, cluster=floats.col(t, source)[1])
        assert k < N or len(got) == N


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("metric", ["ulong_sum", "long_sum", "count"])
def test_sum_and_count_metrics(ints, metric, desc):
    """SUM of one row per group = the crafted value (20-digit sums included); COUNT from the crafted count column: five distinct
    values, so every K lands inside a tie of ~14 000 groups."""
    t = metric.split("_")[0]
    for k in (1, 1000, N - 1, N):
        check_top_n(ints, ["id"], [metric, "int_max"], 1, desc, k, cluster=ints.col(t, "sum")[1] if t != "count" else None)


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
def test_kth_inside_a_large_tie(floats, desc):
    """40 000 groups share the K-th value, K at the start, in the middle and at the end of them: all 40 000 are required each time,
    and nothing below them comes along."""
    dims, metrics = ["id"], ["double_sum", "double_avg"]
    _, st = floats.scan(dims, metrics)
    tied = np.nonzero(st.states[0] == 2.5)[0]
    assert len(tied) == 40_000
    k0 = k_at(floats.ranks(dims, metrics, 1), tied[0], desc)
    for k in (k0, k0 + 20_000, k0 + 39_999):
        got, req, _ = check_top_n(floats, dims, metrics, 1, desc, k, cluster=floats.col("double", "sum")[1])
        assert len(req) == 40_000 + k0 - 1 and len(got) == len(req)


def test_every_group_equal():
    col = {"uint": (np.full(N, 4_000_000_000, dtype=np.uint32), np.full(N, -1)), "double": (np.full(N, -0.0), np.full(N, -1))}
    fam = Family(["uint", "double"], seed=1, columns=col)
    try:
        for metric in ("uint_max", "double_min"):
            for desc in (True, False):
                for k in (1, 500, N):
                    got, _, _ = check_top_n(fam, ["id"], [metric, "count"], 1, desc, k)
                    assert len(got) == N
    finally:
        fam.close()


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("t", FLOAT_TYPES)
def test_formatter_equal_runs_straddle_the_kth(floats, t, desc):
    """The K-th row inside a run of values that print one text (so tie in the reference), with K at the first place the tie
    occupies, in its middle and at its last: the whole run is required, the member 87 ulps (double) / 163 ulps (float) from the
    one the device ranks K-th included; the run's outer neighbours, which print another text, make the tie's edges."""
    dims, metrics, col = ["id"], [t + "_min", t + "_avg"], 1
    _, st = floats.scan(dims, metrics)
    ranks = floats.ranks(dims, metrics, col)
    cluster = floats.col(t, "min")[1]
    cl = cluster[st.keys[0]]
    for c in (0, 1, 6, 7, 12, 13, 36, 37):          # runs above 10^-3, 10^0, 10^3 and 10^15, positive and negative
        members = np.nonzero(cl == c)[0]
        inside = members[ranks[members] == np.bincount(ranks[members]).argmax()]
        assert len(inside) == len(members) - 2 >= 8
        k = k_at(ranks, inside[0], desc)
        for kk in (k, k + len(inside) // 2, k + len(inside) - 1):
            got, req, _ = check_top_n(floats, dims, metrics, col, desc, kk, cluster=cluster)
            assert np.isin(st.keys[0][inside], got).all()


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("t", FLOAT_TYPES)
def test_zeros_and_infinities(floats, t, desc):
    """+0.0 and -0.0 print "0" and "-0" and tie through stod: with the K-th among them, all ten are required. +-inf are the extremes."""
    dims, metrics, col = ["id", "d_" + t], [t + "_avg"], 1
    _, st = floats.scan(dims, metrics)
    vals = st.keys[1]
    ranks = floats.ranks(dims, metrics, col)
    cluster = floats.col(t, "dim")[1]
    zeros = np.nonzero(vals == 0)[0]
    assert len(zeros) == 10 and np.signbit(vals[zeros]).sum() == 5
    k = k_at(ranks, zeros[0], desc)
    for kk in (k, k + 4, k + 9):
        got, req, _ = check_top_n(floats, dims, metrics, col, desc, kk, cluster=cluster)
        assert np.isin(st.keys[0][zeros], got).all() and len(req) == k + 9
    inf = np.nonzero(np.isinf(vals) & ((vals > 0) == desc))[0]
    got, req, _ = check_top_n(floats, dims, metrics, col, desc, 1, cluster=cluster)
    assert sorted(req) == sorted(st.keys[0][inf]) and len(inf) == (2 if desc else 1)          # (their finite neighbour may come along: one cluster)


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("t", ["int", "uint", "long"])
def test_kth_key_at_radix_byte_boundaries(ints, t, desc):
    """K stepping over consecutive values around multiples of 256, 65536 and 2^25: the K-th key's low bytes pass 0xFF.. -> 0x00..
    with the neighbours on the other side of the carry (a wrong hand-over between two radix-select passes shows here)."""
    dims, metrics, col = ["id"], [t + "_max", "count"], 1
    _, st = ints.scan(dims, metrics)
    vals = st.states[0]
    ranks = ints.ranks(dims, metrics, col)
    for centre in RADIX_CENTRES:
        for v in range(centre - 3, centre + 3):
            i = int(np.nonzero(vals == v)[0][0])
            check_top_n(ints, dims, metrics, col, desc, k_at(ranks, i, desc), cluster=ints.col(t, "max")[1])


@pytest.mark.parametrize("passing", [10, 100, 66_000])
def test_row_count_known_only_on_the_device(ints, floats, passing):
    """A filter lets few ids through while the output arrays stay large: the number of rows to rank is only in device memory.
    K below, at and above it."""
    flt = {"op": "lt", "column": "sel", "value": str({10: 1, 100: 2, 66_000: 3}[passing])}
    for fam, metrics, t in ((ints, ["long_max", "count"], "long"), (floats, ["double_min", "double_avg"], "double")):
        for desc in (True, False):
            for k in (1, passing // 2, passing - 1, passing, passing + 1, 10 * passing):
                got, req, st = check_top_n(fam, ["id"], metrics, 1, desc, k, cluster=fam.col(t, metrics[0][-3:])[1], flt=flt)
                assert st.ngroups == passing and (k < passing or len(got) == passing)


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
def test_behind_having_on_the_device(ints, floats, desc):
    """A HAVING that removes the best rows (unsigned integers and doubles order numerically, so a numeric bound cuts the head of
    the ranking): top-N must rank what is left."""
    for fam, t in ((ints, "uint"), (floats, "double")):
        dims, metrics = ["id"], ([t + "_max", "count"] if fam is ints else [t + "_max", t + "_avg"])
        _, st = fam.scan(dims, metrics)
        vals = st.states[0]
        srt = np.sort(vals)
        for cut in (10, 1000):
            hv = (1, "lt", srt[-cut]) if desc else (1, "gt", srt[cut - 1])
            removed = st.keys[0][vals >= srt[-cut]] if desc else st.keys[0][vals <= srt[cut - 1]]
            assert cut <= len(removed) < N // 2
            for k in (1, cut, 5000):
                got, req, _ = check_top_n(fam, dims, metrics, 1, desc, k, cluster=fam.col(t, "max")[1], having=hv)
                assert not np.isin(removed, got).any()


@pytest.mark.parametrize("flags", [0, 1, 64, 1 | 2048, 1 | (1 << 18) | (1 << 20)])
def test_table_organisations(ints, floats, flags):
    """The same superset whichever way the groups were built and emitted: the plan's organisation flags, among them hashed
    partitioning (whose groups reach the output through the list of records)."""
    for fam, t, metrics in ((ints, "long", ["long_max", "count"]), (floats, "double", ["double_min", "double_avg"])):
        for desc in (True, False):
            for k in (1, 1000, N - 1):
                check_top_n(fam, ["id"], metrics, 1, desc, k, cluster=fam.col(t, metrics[0][-3:])[1], flags=flags)
            check_top_n(fam, ["id", "d_" + t], metrics[1:], 1, desc, 1000, cluster=fam.col(t, "dim")[1], flags=flags)


def test_streamed_result():
    """A result region beyond 8 MB with >= 300 000 rows kept: the rows leave through the streamed, packed copy."""
    n = 400_000
    rng = np.random.default_rng(31)
    grid = float_grid(np.dtype(np.float64))
    col = {"long": ((rng.integers(0, 10 ** 16, n) * rng.choice([-1, 1], n)).astype(np.int64), np.full(n, -1)),
           "double": (grid[rng.integers(0, len(grid), n)], np.full(n, -1))}
    fam = Family(["long", "double"], seed=2, n=n, seg_rows=(150_000, 130_000, 120_000), columns=col)
    try:
        metrics = ["long_max", "long_min", "long_sum", "double_min", "double_sum", "count"]
        assert n * (4 + 8 * 5 + 4) > (8 << 20)
        for desc in (True, False):
            got, req, _ = check_top_n(fam, ["id"], metrics, 1, desc, 300_000)
            assert len(got) >= 300_000
            got, req, _ = check_top_n(fam, ["id"], metrics, 4, desc, 320_000)          # double_min: ties of ~1 750 groups per grid point
            assert len(got) >= 320_000
    finally:
        fam.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
def _pair(tconf, rows):
    from viyadb_amd import hostdb
    gdb = hostdb.Database({"tables": [tconf]})
    odb = vo.Database({"tables": [tconf]})
    gdb.load(tconf["name"], rows)
    odb.table(tconf["name"]).load(rows)
    return gdb, odb


def _both_ways(monkeypatch, gdb, odb, q):
    want, ost = odb.query(q)
    out = {}
    for host_only in ("", "1"):
        if host_only:
            monkeypatch.setenv("VIYA_HOST_TOPN", "1")
        else:
            monkeypatch.delenv("VIYA_HOST_TOPN", raising=False)
        got, gst = gdb.query(q)
        out[host_only] = got
        print("sorted query %s (VIYA_HOST_TOPN=%r): got %s, oracle %s" % ({k: q[k] for k in ("sort", "limit", "skip") if k in q}, host_only, got[:3], want[:3]))
        assert gst["aggregated_recs"] == ost["aggregated_recs"] and gst["output_recs"] == ost["output_recs"]
    assert out[""] == want, ("device top-N", q.get("sort"), out[""][:3], want[:3])
    assert out["1"] == want, ("host order", q.get("sort"), out["1"][:3], want[:3])


E2E_IDS = 75_000


def _e2e_rows(special, filler):
    """One row per id; `special`: {id: [metric strings]}; every other id gets `filler`."""
    return [[str(i)] + (special.get(i) or filler) for i in range(E2E_IDS)]


@pytest.mark.parametrize("kind,hi,lo", [("double", "1000.0000000000149", "1000.000000000005"), ("float", "1000.01495361328125", "1000.00500488281250")])
def test_formatter_tie_end_to_end(monkeypatch, kind, hi, lo):
    """Two groups whose SUMs differ (87 ulps for the double pair, 163 for the float pair) but print one text: they tie on `revenue`,
    and the second sort column decides. A device that drops the numerically lower one returns the wrong id."""
    dt = np.dtype(np.float64 if kind == "double" else np.float32)
    a, b = np.array([hi], dtype=dt), np.array([lo], dtype=dt)
    assert vo.fmt_num(a[0]) == vo.fmt_num(b[0])
    assert int(a.view("u%d" % dt.itemsize)[0]) - int(b.view("u%d" % dt.itemsize)[0]) == (87 if kind == "double" else 163)
    tconf = {"name": "events", "segment_size": 40000, "dimensions": [{"name": "id", "type": "uint"}],
             "metrics": [{"name": "revenue", "type": kind + "_sum"}, {"name": "count", "type": "count"}]}
    # descending: the upper value sits at the larger id; ascending: the same with every value negated
    for sign, asc in (("", False), ("-", True)):
        rows = _e2e_rows({70_001: [sign + hi], 5: [sign + lo], 6: [sign + "999.5"]}, [sign + "3.5"])
        gdb, odb = _pair(tconf, rows)
        try:
            base = {"type": "aggregate", "table": "events", "dimensions": ["id"], "metrics": ["revenue", "count"],
                    "sort": [{"column": "revenue", "ascending": asc}, {"column": "id", "ascending": True}]}
            want, _ = odb.query(dict(base, limit=1))
            assert want[0][0] == "5"          # the tie on revenue goes to the smaller id
            _both_ways(monkeypatch, gdb, odb, dict(base, limit=1))
            _both_ways(monkeypatch, gdb, odb, dict(base, limit=1, skip=1))
            _both_ways(monkeypatch, gdb, odb, dict(base, limit=3))
        finally:
            gdb.close()


def test_long_integers_and_string_order_end_to_end(monkeypatch):
    """19-digit long_max / 20-digit ulong_max values that share a key (they differ in the low 6 bits only) with the order made
    total by a second sort column, and the reference's -5 > 3, -10 > 99."""
    tconf = {"name": "events", "segment_size": 40000, "dimensions": [{"name": "id", "type": "uint"}],
             "metrics": [{"name": "best", "type": "long_max"}, {"name": "top", "type": "ulong_max"}, {"name": "small", "type": "int_max"}]}
    special = {}
    for j in range(40):
        special[60_000 + j] = [str(9223372036854775807 - 63 + j), str(18446744073709551615 - 63 + (j * 7) % 40), "7"]
        special[100 + j] = [str(-9223372036854775808 + j), str(10 ** 19 + j), "7"]
    special[7] = ["-5", "5", "-5"]
    special[8] = ["3", "3", "3"]
    special[9] = ["-10", "10", "-10"]
    special[10] = ["99", "99", "99"]
    gdb, odb = _pair(tconf, _e2e_rows(special, ["1", "1", "1"]))
    try:
        base = {"type": "aggregate", "table": "events", "dimensions": ["id"], "metrics": ["best", "top", "small"]}
        for col in ("best", "top", "small"):
            for asc in (False, True):
                for extra in ({"limit": 1}, {"limit": 10}, {"limit": 5, "skip": 37}, {"limit": 50, "skip": 60}):
                    _both_ways(monkeypatch, gdb, odb, dict(base, sort=[{"column": col, "ascending": asc}, {"column": "id", "ascending": not asc}], **extra))
        want, _ = odb.query(dict(base, sort=[{"column": "small"}, {"column": "id"}], limit=4))
        assert [r[3] for r in want] == ["-10", "99", "-5", "7"]
    finally:
        gdb.close()
