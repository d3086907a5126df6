"""HAVING on the oracle's side and as plan nodes: shared by the tests that push a HAVING down to the emission kernels.

keep_mask() follows vo.post_aggregate: the same ComparisonBuilder semantics on the aggregated tuples (post_agg.cc:77-83) — comparisons in
the result column's own type, an AVG compares its raw sum (the state as it is), a bitset its cardinality in the bitset's integer type.
having_nodes() builds the postfix nodes executor.AggPlan.having takes, `col` being the result column (group i, or ngroups + metric j).

Literals on byte / short columns: the reference cannot compile a comparison on them (vo.decode_value raises Unsupported; its generated code
calls AnyNum getters that do not exist). The device compares them like every other integer type, so both sides here parse the literal with
the column's own NumType instead of refusing — the typed comparison is the only sensible meaning, and tests/having_host.cc holds the device
code to it for these two types as well."""
from __future__ import annotations

import numpy as np

from oracle import viya_oracle as vo
from tests.planner import capi_anynum

OPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5}


def decode(tab, col, value):
    try:
        return vo.decode_value(tab, col, value)
    except vo.Unsupported:
        return col.num_type.parse(value)


def result_columns(aq, st):
    """{column name: the array HAVING sees} as vo.post_aggregate's getcol picks them."""
    cols = {oc.col.name: st.keys[k] for k, oc in enumerate(aq.dim_cols)}
    for k, oc in enumerate(aq.metric_cols):
        s = st.states[k]
        if oc.col.agg == "bitset":
            s = s.astype(np.uint64 if oc.col.num_type.size == 8 else np.uint32)
        cols[oc.col.name] = s
    return cols


def keep_mask(tab, aq, st):
    """Which of the oracle's groups pass aq.having (all of them without one)."""
    n = st.ngroups
    if aq.having is None:
        return np.ones(n, dtype=bool)
    cols = result_columns(aq, st)
    r = vo.eval_filter(tab, aq.having, lambda c: cols[c.name], decode)      # (the oracle's own ComparisonBuilder, with the literal decoding above)
    return np.ones(n, dtype=bool) if r is None else np.broadcast_to(np.asarray(r, dtype=bool), (n,)).copy()


def apply_keep(st, keep):
    """The oracle's state with only the kept groups (in place, like the test that first did this); returns st."""
    st.keys = [k[keep] for k in st.keys]
    st.states = [s[keep] for s in st.states]
    if st.hidden_count is not None:
        st.hidden_count = st.hidden_count[keep]
    return st


def having_nodes(tab, aq, having=None):
    """aq.having (or `having`, a parsed filter) as AggPlan.having nodes."""
    names = [oc.col.name for oc in aq.dim_cols] + [oc.col.name for oc in aq.metric_cols]
    nodes = []

    def walk(f):
        if isinstance(f, vo.Empty):
            nodes.append(("true",))
        elif isinstance(f, vo.Rel):
            c = tab.column(f.column)
            nodes.append(("rel", names.index(f.column), OPS[f.op], capi_anynum(c, decode(tab, c, f.value))))
        elif isinstance(f, vo.In):
            c = tab.column(f.column)
            nodes.append(("in", names.index(f.column), f.equal, [capi_anynum(c, decode(tab, c, v)) for v in f.values]))
        else:
            for ch in f.filters:
                walk(ch)
            nodes.append((f.op, len(f.filters)))
    walk(aq.having if having is None else having)
    return nodes
