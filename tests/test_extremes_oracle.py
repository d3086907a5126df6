"""The oracle at the extremes (no GPU): on the edge table every query of tests/test_gpu_extremes.py's set must give the numpy oracle's
groups and the CPU twin's (the reference-style C++, compiled with g++: native wrap-around and std::min / std::max) — float SUM / AVG
through the exact-sum bound, everything else bit for bit — and the float-sum check must accept sequential sums and reject a wrong one."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from oracle.cpu_twin import Twin
from tests import extremes as X
from tests.parity import compare

# Queries the twin is not asked: none of the set today. (Filters on byte / short columns do not compile in the reference: the set has
# none, and test_byte_short_filters_are_refused pins that the oracle refuses them.)
TWIN_CANNOT = {}


@pytest.fixture(scope="module")
def tab():
    return X.edge_table()


def _twin_vs_oracle(tab, q, label):
    aq = vo.parse_query(tab, q)
    st = vo.scan_aggregate(aq)
    tw = Twin(tab, q)
    got = tw.run()
    got.passed_recs = st.passed_recs                    # (the twin keeps no such counter)
    pos = X.float_sum_positions(aq)
    adds = X.group_addends(tab, aq)
    X.check_float_sums(st.keys, st.states, aq, adds, label + " oracle", pos)
    X.check_float_sums(got.keys, got.states, aq, adds, label + " twin", pos)
    compare(X._without(got, pos), X._without(st, pos), label)
    return tw


def test_edge_table_shape(tab):
    """Degenerate segments hold one value; every edge value of every type is in segment 0."""
    assert len(tab.segments) == 4
    for t in X.TYPES:
        d = tab.dimension("d_" + t).index
        seg = tab.segments
        assert len(np.unique(seg[1]["d"][d])) == 1 and len(np.unique(seg[2]["d"][d])) == 1
        e = X.edges(t)
        assert np.isin(e, seg[0]["d"][d]).all() if t not in X.FLOAT_TYPES else len(np.unique(seg[0]["d"][d])) == len(np.unique(e))
    f = tab.dimension("d_float").index
    assert np.all(np.signbit(tab.segments[1]["d"][f])) and not np.any(np.signbit(tab.segments[3]["d"][f]))
    assert np.all(np.isposinf(tab.segments[2]["d"][f]))


@pytest.mark.parametrize("t", X.FILTERABLE)
def test_predicates_twin(tab, t):
    """One twin per (type, operator) shape; every edge literal through it (literals are arguments, not part of the compiled text)."""
    for op in X.OPS:
        for lits in X.pred_literal_sets(t, op):
            q = X.pred_query(t, op, lits)
            assert str(q) not in TWIN_CANNOT
            _twin_vs_oracle(tab, q, f"{t} {op} {lits}")


def test_wrapped_literals(tab):
    """stoul wraps: "256" on ubyte is 0, "-1" on uint is UINT32_MAX (and matches the rows holding it)."""
    assert vo.NumType("ubyte").parse("256") == 0
    assert vo.NumType("uint").parse("-1") == 2 ** 32 - 1
    st = vo.scan_aggregate(vo.parse_query(tab, X.pred_query("uint", "eq", ["-1"])))
    assert st.passed_recs > 0


def test_byte_short_filters_are_refused(tab):
    for t in ("byte", "short"):
        with pytest.raises(vo.Unsupported):
            vo.scan_aggregate(vo.parse_query(tab, X.pred_query(t, "eq", ["0"])))


@pytest.mark.parametrize("t", X.TYPES)
def test_metrics_twin(tab, t):
    """SUM / MIN / MAX / AVG of each type per kind of group: wrapping sums, identity-only groups, negative floats (MAX answers FLT_MIN),
    subnormals, infinities."""
    _twin_vs_oracle(tab, X.metric_query(t), t)
    _twin_vs_oracle(tab, X.metric_query(t, filt=X.F("gt", "d_ulong", "0")), t + " filtered")


@pytest.mark.parametrize("dims", X.KEY_SETS, ids=lambda d: "+".join(d))
def test_keys_twin(tab, dims):
    """Extreme keys: ±0.0 one group, ±inf, subnormals, INT64_MIN..INT64_MAX, u64 keys ≥ 2^63."""
    _twin_vs_oracle(tab, X.key_query(dims), "+".join(dims))


def test_identity_quirk_and_signed_zero_groups(tab):
    aq = vo.parse_query(tab, X.metric_query("float"))
    st = vo.scan_aggregate(aq)
    g = list(st.keys[0])
    assert st.states[3][g.index(1)] == np.float32(vo.FLT_MIN)            # negative floats only: MAX is the identity FLT_MIN
    assert st.states[3][g.index(2)] == np.float32(vo.FLT_MIN)            # positive subnormals are below it too
    assert st.states[2][g.index(2)] == -X.float_specials("float")["sub_max"]
    st = vo.scan_aggregate(vo.parse_query(tab, X.key_query(["d_float"])))
    k = st.keys[0]
    assert np.sum(k == 0) == 1                                           # +0.0 and -0.0 are one group
    assert np.isposinf(k).any() and np.isneginf(k).any()
    assert ((np.abs(k) < np.finfo(np.float32).tiny) & (k != 0)).sum() == 4


def test_wrapping_sums(tab):
    for t in ("uint", "long", "ulong"):
        st = vo.scan_aggregate(vo.parse_query(tab, X.metric_query(t)))
        rows = {int(g): i for i, g in enumerate(st.keys[0])}                   # (this query's own group order)
        seg_adds = X.group_addends(tab, vo.parse_query(tab, X.metric_query(t)))
        vals = seg_adds[(4,)][1]
        bits = np.dtype(X.np_type(t)).itemsize * 8
        exact = sum(int(v) for v in vals)
        assert exact >= 2 ** (bits - (1 if t == "long" else 0))                 # the exact sum is past the type's range ...
        want = exact % 2 ** bits
        got = int(st.states[1][rows[4]]) % 2 ** bits
        assert got == want                                                     # ... and the oracle wraps it


# -------------------------------------------------------------------------------------------------- the float-sum check itself
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_check_accepts_sequential_and_rejects_wrong_sums(tab, dtype):
    t = "float" if dtype == np.float32 else "double"
    aq = vo.parse_query(tab, X.metric_query(t))
    adds = X.group_addends(tab, aq)
    checked = 0
    for key, per in adds.items():
        vals = np.array(per[1], dtype=dtype)
        seq = dtype(0)
        for v in vals:                                       # the reference's loop: one += per row, in row order
            seq = dtype(seq + v)
        for order in (vals, vals[::-1], np.sort(vals)):
            s = dtype(0)
            for v in order:
                s = dtype(s + v)
            ok, why = X.sum_within_bound(vals, s, dtype)
            assert ok, (key, why)
        if not np.all(np.isfinite(vals)):
            continue
        # a row dropped or added twice: rejected wherever that row is not lost in the rounding of the others
        big = int(np.argmax(np.abs(vals)))
        for wrong in (seq - vals[big], seq + vals[big]):
            if abs(float(vals[big])) > 4 * len(vals) * float(np.finfo(dtype).eps) * float(np.sum(np.abs(vals.astype(np.float64)))) + float(np.spacing(abs(seq))):
                ok, _ = X.sum_within_bound(vals, dtype(wrong), dtype)
                assert not ok, (key, vals[big], wrong)
                checked += 1
    assert checked >= 8
    # subnormals flushed to zero are caught
    sub = np.array([X.float_specials(t)["sub_max"]] * 100, dtype=dtype)
    assert X.sum_within_bound(sub, dtype(100) * sub[0], dtype)[0]
    assert not X.sum_within_bound(sub, dtype(0), dtype)[0]
    # infinities: exact, NaN equal to NaN
    inf = np.array([1, np.inf, -2], dtype=dtype)
    assert X.sum_within_bound(inf, dtype(np.inf), dtype)[0] and not X.sum_within_bound(inf, dtype(1e30), dtype)[0]
    nan = np.array([np.inf, -np.inf, 3], dtype=dtype)
    assert X.sum_within_bound(nan, dtype(np.nan), dtype)[0] and not X.sum_within_bound(nan, dtype(np.inf), dtype)[0]
