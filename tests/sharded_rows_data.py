"""Tables for tests/test_gpu_sharded_rows.py: one table's segments split between ranks as contiguous blocks. Every segment is
generated from its GLOBAL index alone, so a rank's shard and one table holding all segments hold the same bytes in the same
storage order (rank, local segment, row). Segment sizes are ragged (full, partial, a few rows, not multiples of the wave step)."""
import numpy as np

from oracle import viya_oracle as vo

SEG = 3000
SIZES = [3000, 1200, 2999, 17, 3000, 2500, 800, 1999]
TABLE = {"name": "t", "segment_size": SEG,
         "dimensions": [{"name": "a", "type": "uint"}, {"name": "k", "type": "uint"}, {"name": "f", "type": "uint"}],
         "metrics": [{"name": "v", "type": "long_sum"}, {"name": "count", "type": "count"}, {"name": "users", "type": "bitset"}]}
COLS = [0, 1, 2, 3, 4, 5]          # storage order: a, k, f, v, count, users (a bitset: its per-row cardinality)
FILTER = {"op": "lt", "column": "f", "value": "40"}
BITSET_FILTER = {"op": "and", "filters": [{"op": "lt", "column": "f", "value": "70"}, {"op": "gt", "column": "users", "value": "2"}]}

# scenario -> the global segments of rank 0 and of rank 1 (rank 1's always follow rank 0's)
SPLITS = {
    "ragged": (range(0, 3), range(3, 8)),
    "rank1_empty": (range(0, 8), range(8, 8)),
    "rank0_empty": (range(0, 0), range(0, 8)),
}


def _segment(g, no_pass=False):
    r = np.random.default_rng([1234, g])
    n = SIZES[g]
    a = r.integers(0, 10 + 8 * g, n).astype(np.uint32)                   # later segments bring values of their own: first occurrences in every block
    k = (np.arange(n, dtype=np.uint32) + np.uint32(g * 100000))           # position-revealing: segment and row
    f = r.integers(0, 100, n).astype(np.uint32)
    if no_pass:
        f = f + np.uint32(100)                                             # nothing passes f < 40 or f < 70
    v = r.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
    c = r.integers(1, 4, n).astype(np.uint32)
    users = [set(int(x) for x in r.integers(0, 50, int(r.integers(0, 6)))) for _ in range(n)]
    return [a, k, f], [v, c, users], n


def build(segments, no_pass_from=None):
    """oracle Table holding the given global segments, in order; segments >= no_pass_from hold no passing row."""
    t = vo.Table(TABLE)
    for g in segments:
        d, m, n = _segment(g, no_pass_from is not None and g >= no_pass_from)
        t.add_segment_arrays(d, m, None, n)
    return t


def shard(name, rank):
    segs = SPLITS["ragged" if name == "rank1_nopass" else name][rank]
    return build(segs, no_pass_from=3 if name == "rank1_nopass" else None)


def whole(name):
    return build(range(len(SIZES)), no_pass_from=3 if name == "rank1_nopass" else None)


def oracle_select(t, flt, skip, limit):
    """(one numpy array per COLS column, stats) of one table's select."""
    aq = vo.parse_query(t, {"type": "aggregate", "table": "t", "dimensions": [], "metrics": [], "filter": flt})
    aq.skip, aq.limit = skip, limit
    picked, stats = vo.scan_select(aq)
    out = []
    for c in COLS:
        vals = []
        for si, i in picked:
            seg = t.segments[si]
            vals.append(seg["d"][c][i] if c < 3 else (len(seg["m"][c - 3][i]) if c == 5 else seg["m"][c - 3][i]))
        out.append(np.array(vals))
    return out, stats
