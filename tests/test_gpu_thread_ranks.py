"""vh_query_agg_sharded and vh_query_select_sharded at 3, 4 and 8 ranks on one GPU: the ranks are threads of this process, each with its
own device table and its own communicator over callbacks (tests/thread_ranks.py). Everything the two-process tests of
test_gpu_distributed.py and test_gpu_sharded_rows.py run at W = 2 runs here at the world sizes where `x % nparts`, up to W owners per
block, ranks without segments below a rank and W x mode in the verdict differ from their W = 2 selves. RCCL itself is not covered here
(test_gpu_distributed.py::test_one_rank_through_rccl).

Every case is one run_ranks call: each rank mirrors its shard, runs the same plan twice (the first agreement, then the cached / steady
state) and returns numpy arrays. Aggregates are compared with the oracle over the union of the shards (test_gpu_distributed._check: keys,
integer states and counters bit for bit, float sums within its rtol of 1e-9); selects with sharded_rows_data.oracle_select over one table
holding every rank's segments in rank order. Shards are two segments of at most 5 000 rows per rank."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import shard_scenarios
from tests import sharded_rows_data as D
from tests.planner import mirror_table, plan_from_query
from tests.test_gpu_distributed import _check
from tests.thread_ranks import run_ranks
from viyadb_amd import capi, distributed

pytestmark = pytest.mark.gpu
NOW = 1496570140
ROWS = 5000
HASH = capi.PLAN_FORCE_HASH
RECORDS = capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HASH_RECORDS
HP = capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_HPART | capi.PLAN_FORCE_JIT
ORGANISATIONS = [(0, None), (capi.PLAN_FORCE_GLOBAL, "dense_global"), (capi.PLAN_FORCE_PART, "dense_part"), (HASH, "hash"), (RECORDS, "hash")]


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


class Got(dict):
    """One rank's result of one run, in the shape test_gpu_distributed._check reads (an .npz of the two-process tests)."""

    def __init__(self, res, calls):
        super().__init__({"arr_%d" % i: a for i, a in enumerate(res.keys + res.states)})
        self.update(nk=len(res.keys), returned=res.returned, ngroups=res.ngroups, path=res.path, scanned=res.scanned_recs,
                    passed=res.passed_recs, retries=res.retries)
        self.calls = calls

    @property
    def files(self):
        return list(self.keys())


_ORACLE = {}


def scenario_oracle(name, world, metrics=None, **kw):
    """The oracle over the union of the ranks' shards, computed once per scenario."""
    key = (name, world, tuple(metrics or ()), tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple, set, frozenset)) else v) for k, v in kw.items())))
    if key not in _ORACLE:
        tab, q, _, _ = shard_scenarios.build(name, list(range(world)), world, rows=ROWS, **kw)
        if metrics:
            q = dict(q, metrics=list(metrics))
        _ORACLE[key] = (tab, q, vo.scan_aggregate(vo.parse_query(tab, q), now=NOW))
    tab, q, st = _ORACLE[key]
    return tab, q, vo.AggState(list(st.keys), list(st.states), st.hidden_count, st.scanned_recs, st.scanned_segments, st.passed_recs)   # (_check may filter its copy)


def sharded_runs(name, world, flags, root, metrics=None, change_plan=None, **kw):
    """-> runs[it][rank]: every rank's Got of the first and of the second run of one plan."""
    def rank_body(rank, comm):
        tab, q, flags0, hint = shard_scenarios.build(name, [rank], world, rows=ROWS, **kw)
        if metrics:
            q = dict(q, metrics=list(metrics))
        t = mirror_table(tab)
        try:
            plan = plan_from_query(tab, vo.parse_query(tab, q), now=NOW, flags=flags0 | flags, groups_hint=hint)
            if change_plan is not None:
                change_plan(plan)
            out = []
            for _ in range(2):
                res = distributed.sharded_query(t, plan, comm, root=root)
                if root >= 0:
                    assert (res.returned == 0) == (rank != root or res.ngroups == 0), (rank, res.returned)
                out.append(Got(res, dict(comm.transport.calls)))
            return out
        finally:
            t.close()
    per_rank = run_ranks(world, rank_body)
    return [[per_rank[r][it] for r in range(world)] for it in range(2)]


def check_runs(runs, st, root, path=None, having_keep=None):
    for gots in runs:
        holders = gots if root < 0 else [gots[root]]                       # (a dense query tells its group count where the groups are)
        assert all(int(g["ngroups"]) == st.ngroups for g in holders), [int(g["ngroups"]) for g in gots]
        copy = vo.AggState(list(st.keys), list(st.states), st.hidden_count, st.scanned_recs, st.scanned_segments, st.passed_recs)
        _check(gots, copy, root=root, having_keep=having_keep)
        assert len(set(str(g["path"]) for g in gots)) == 1, [str(g["path"]) for g in gots]       # all ranks report one path
        if path:
            assert str(gots[0]["path"]) == path, (str(gots[0]["path"]), path)


# ------------------------------------------------------------------------------------------------------------ aggregates
@pytest.mark.parametrize("last_root", [False, True], ids=["root0", "rootlast"])
@pytest.mark.parametrize("flags,path", ORGANISATIONS, ids=["planner", "dense_global", "dense_part", "hash", "records"])
@pytest.mark.parametrize("world", [3, 4, 8])
@pytest.mark.parametrize("name", ["uniform", "disjoint_ranges"])
def test_every_organisation_at_3_4_and_8_ranks(name, world, flags, path, last_root):
    """`disjoint_ranges` with 100 between the ranks' ranges of `a` instead of 1000: at these table sizes the agreed range of eight ranks
    is then still one the planner makes a dense table of (at most four ids per row to scan)."""
    root = world - 1 if last_root else 0
    kw = {"spread": 100} if name == "disjoint_ranges" else {}
    _, _, st = scenario_oracle(name, world, **kw)
    runs = sharded_runs(name, world, flags, root, **kw)
    check_runs(runs, st, root, path)
    if path is None:
        assert str(runs[0][0]["path"]).startswith("dense")


@pytest.mark.parametrize("flags,path", [(0, None), (HASH, "hash")], ids=["dense", "hash"])
@pytest.mark.parametrize("world,empty", [(3, (1,)), (3, (2,)), (3, (0, 2)), (4, (1,)), (4, (3,)), (4, (0, 2, 3))],
                         ids=["3-middle", "3-last", "3-all-but-one", "4-middle", "4-last", "4-all-but-one"])
def test_empty_shards(world, empty, flags, path):
    """Ranks without a single row: in the middle, at the end, and everywhere but on one rank (the root is then an empty rank)."""
    _, _, st = scenario_oracle("empty_shard", world, empty=empty)
    runs = sharded_runs("empty_shard", world, flags, 0, empty=empty)
    check_runs(runs, st, 0, path)
    if path is None:
        assert str(runs[0][0]["path"]).startswith("dense")


def test_one_rank_overflows_and_three_replan():
    _, _, st = scenario_oracle("one_rank_overflows", 3)
    runs = sharded_runs("one_rank_overflows", 3, 0, 0)
    check_runs(runs, st, 0, "hash")
    retries = [max(int(runs[it][r]["retries"]) for it in range(2)) for r in range(3)]
    assert retries[0] >= 1 and len(set(retries)) == 1, retries           # one rank's overflow re-plans all of them, as often


TYPED_ALL = ["count", "d", "imin", "lmax", "users"]
TYPED_HP = ["count", "imin", "users"]                                    # (the hashed partitioning takes at most 64 bits of states)


@pytest.mark.parametrize("root", [-1, 0])
@pytest.mark.parametrize("flags,metrics", [(HASH, TYPED_ALL), (RECORDS, TYPED_ALL), (HP, TYPED_HP)], ids=["hash", "records", "hpart"])
@pytest.mark.parametrize("world", [3, 8])
def test_signed_keys_and_count_distinct(world, flags, metrics, root):
    """Keys with negatives at two widths, every group on several ranks, ids that overlap between ranks: the merged count-distinct is the
    oracle's only if every rank's (group, id) pairs reached the group's owner. root = -1: the owners keep their rows — disjoint, and
    together the answer."""
    if flags == HP:
        from tests.conftest import JIT_OFF
        if JIT_OFF:
            pytest.skip("VH_JIT=off: the hashed partitioning needs the scan kernel compiled for the plan")
    _, _, st = scenario_oracle("typed", world, metrics=metrics)
    assert (st.keys[0] < 0).any() and (st.keys[1] < 0).any() and int(st.states[-1].max()) > 20
    runs = sharded_runs("typed", world, flags & ~HASH, root, metrics=metrics)     # (the scenario forces the hash organisation itself)
    check_runs(runs, st, root, "hash")
    if root < 0:
        for gots in runs:
            assert sum(int(g["returned"]) for g in gots) == st.ngroups


def partial_counts(world, col):
    """Per rank, {group key: the rank's partial state of metric `col`} of the `uniform` scenario."""
    out = []
    for rank in range(world):
        tab, q, _, _ = shard_scenarios.build("uniform", [rank], world, rows=ROWS)
        st = vo.scan_aggregate(vo.parse_query(tab, q), now=NOW)
        out.append({(int(a), int(b)): int(c) for a, b, c in zip(st.keys[0], st.keys[1], st.states[col])})
    return out


@pytest.mark.parametrize("flags,path", [(0, None), (HASH, "hash")], ids=["dense", "hash"])
def test_having_sees_merged_groups(flags, path):
    """HAVING count >= T with T above every count of every single rank's partial: no rank alone would keep any group."""
    world, root = 4, 3
    _, _, st = scenario_oracle("uniform", world)
    T = 1 + max(max(p.values()) for p in partial_counts(world, 1))
    keep = st.states[1] >= T
    assert 0 < int(keep.sum()) < st.ngroups, (T, int(keep.sum()))

    def having(plan):
        plan.having = [("rel", 2 + 1, capi.OP_GE, T)]                  # result column: two keys, then `count`
    runs = sharded_runs("uniform", world, flags, root, change_plan=having)
    check_runs(runs, st, root, path, having_keep=keep)


@pytest.mark.parametrize("flags,path", [(0, None), (HASH, "hash")], ids=["dense", "hash"])
def test_top_n_sees_merged_groups(flags, path):
    """Top 5 by count, descending: a superset of the groups that tie with or beat the fifth MERGED count, rows as the oracle has them. One of
    those groups is in no single rank's own top 5. (How much more than the top comes back is the library's choice: below 65 536 output
    slots it reads a result back whole.)"""
    world, root, k = 4, 0, 5
    _, _, st = scenario_oracle("uniform", world)
    kth = int(np.sort(st.states[1])[::-1][k - 1])
    must = {(int(a), int(b)) for a, b, c in zip(st.keys[0], st.keys[1], st.states[1]) if int(c) >= kth}
    parts = partial_counts(world, 1)
    kth_of = [sorted(p.values(), reverse=True)[k - 1] for p in parts]
    assert any(all(p.get(g, 0) < t for p, t in zip(parts, kth_of)) for g in must), "every merged top group is in some rank's own top 5"

    def top(plan):
        plan.top = (2 + 1, True, k)
    runs = sharded_runs("uniform", world, flags, root, change_plan=top)
    want = {(int(st.keys[0][i]), int(st.keys[1][i])): tuple(int(s[i]) for s in st.states) for i in range(st.ngroups)}
    for gots in runs:
        g = gots[root]
        arrs = [g["arr_%d" % i] for i in range(6)]
        got = {(int(arrs[0][i]), int(arrs[1][i])): tuple(int(a[i]) for a in arrs[2:]) for i in range(int(g["returned"]))}
        assert len(got) == int(g["returned"]) and must <= set(got), (sorted(must - set(got)), len(got))
        assert all(want[key] == row for key, row in got.items())
        assert all(int(o["returned"]) == 0 for r, o in enumerate(gots) if r != root)
        assert all(int(o["scanned"]) == st.scanned_recs and int(o["passed"]) == st.passed_recs for o in gots)
        if path:
            assert str(g["path"]) == path


def test_steady_state_needs_no_allgather():
    """The second run of an unchanged dense plan: the verdict and the state arrays are reduced, nothing is all-gathered."""
    _, _, st = scenario_oracle("uniform", 3)
    runs = sharded_runs("uniform", 3, 0, 0)
    check_runs(runs, st, 0)
    for rank in range(3):
        first, second = runs[0][rank].calls, runs[1][rank].calls
        assert first["allgather"] == 1 and second["allgather"] == 1, (rank, first, second)
        assert second["reduce"] > first["reduce"] >= 2 and second["alltoallv"] == 0, (rank, first, second)


# ------------------------------------------------------------------------------------------------------------ storage positions and select
def split_table(split, rank=None):
    """sharded_rows_data's global segments split between ranks: one rank's table, or the table holding all of them in rank order."""
    return D.build([g for r, segs in enumerate(split) if rank is None or r == rank for g in segs])


@pytest.mark.parametrize("flags", [0, HASH], ids=["dense", "hash"])
def test_first_occurrences_are_global_positions(flags):
    """VH_COL_ROWID at four ranks, rank 1 without segments: a rank's segment s is segment seg_base + s of the global storage order, seg_base
    counting the segments of ALL lower ranks — rank 1's none among them."""
    split = [[0, 1, 2], [], [3], [4, 5]]          # (ragged on purpose: ranks, segments per rank and segments below a rank all differ)
    whole = split_table(split)
    want = {}
    for g, seg in enumerate(whole.segments):                             # plain numpy: the first passing row of every `a`, in storage order
        n = seg["size"]
        a, f = seg["d"][0][:n], seg["d"][2][:n]
        for row in np.nonzero(f < 40)[0]:
            want.setdefault(int(a[row]), (g << 32) | int(row))
    assert {p >> 32 for p in want.values()} >= {0, 3, 4}                # first occurrences in the blocks of ranks 0, 2 and 3

    def rank_body(rank, comm):
        tab = split_table(split, rank)
        t = mirror_table(tab, reserve=max(1, len(tab.segments)))
        try:
            aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": ["a"], "metrics": ["count"], "filter": D.FILTER})
            plan = plan_from_query(tab, aq, flags=flags)
            plan.metrics = [capi.COL_ROWID]
            out = []
            for _ in range(2):
                res = distributed.sharded_query(t, plan, comm, root=0)
                out.append((dict(zip(res.keys[0].tolist(), [int(x) for x in res.states[0]])), res.path, res.passed_recs))
            return out
        finally:
            t.close()
    got = run_ranks(4, rank_body)
    for it in range(2):
        pairs, path, passed = got[0][it]
        assert pairs == want, (it, {k: (hex(pairs.get(k, 0)), hex(v)) for k, v in want.items() if pairs.get(k) != v})
        assert (path == "hash") == (flags == HASH), path
        assert all(got[r][it][0] == {} for r in range(1, 4))
        assert len({got[r][it][2] for r in range(4)}) == 1


SELECT_SPLITS = {3: [[0, 1, 2], [3, 4], [5, 6, 7]], 4: [[0, 1], [2, 3], [4, 5], [6, 7]]}
EMPTY_MIDDLE = {3: [[0, 1, 2, 3], [], [4, 5, 6, 7]], 4: [[0, 1], [], [2, 3, 4], [5, 6, 7]]}


@pytest.mark.parametrize("world", [3, 4])
def test_select_windows_at_3_and_4_ranks(world):
    split = SELECT_SPLITS[world]
    whole = split_table(split)
    passed_of = [D.oracle_select(split_table(split, r), D.FILTER, 0, 0)[1]["passed_recs"] for r in range(world)]
    total = sum(passed_of)
    into_rank2 = passed_of[0] + passed_of[1] + min(10, passed_of[2] - 1)
    assert passed_of[0] > 55 and passed_of[2] > 1
    # (split, filter, skip, limit, root)
    cases = [(split, D.FILTER, 0, 0, 0),                                 # no limit
             (split, D.FILTER, into_rank2, 0, 0),                        # the skip ends inside rank 2
             (split, D.FILTER, 5, 50, 0),                                # the limit is reached inside rank 0: every later segment of every rank sends its first passing row
             (EMPTY_MIDDLE[world], D.FILTER, 3, 0, 0),                   # a rank without segments in the middle
             (EMPTY_MIDDLE[world], D.FILTER, 5, 50, world - 1),
             (split, D.BITSET_FILTER, 7, 0, world - 1),                  # delivered on the last rank
             (split, D.FILTER, total + 5, 0, 0)]                         # a skip beyond everything

    def rank_body(rank, comm):
        out = []
        tables = {}
        try:
            for sp, flt, skip, limit, root in cases:
                key = id(sp)
                if key not in tables:
                    tab = split_table(sp, rank)
                    tables[key] = (tab, mirror_table(tab, reserve=max(1, len(tab.segments))))
                tab, t = tables[key]
                aq = vo.parse_query(tab, {"type": "aggregate", "table": "t", "dimensions": [], "metrics": [], "filter": flt})
                filt = plan_from_query(tab, aq).filter
                for _ in range(2):
                    cols, info = distributed.sharded_select(t, filt, D.COLS, comm, skip=skip, limit=limit, root=root)
                    out.append((cols, info.nrows, info.passed_recs, info.scanned_recs, info.scanned_segments))
            return out
        finally:
            for _, t in tables.values():
                t.close()
    got = run_ranks(world, rank_body)
    for i, (sp, flt, skip, limit, root) in enumerate(cases):
        want, st = D.oracle_select(split_table(sp), flt, skip, limit)
        if i == 2:
            assert st["output_recs"] == 50 + sum(len(s) for s in sp) - 1     # the first row of each of the other segments
        if i == 6:
            assert st["output_recs"] == 0
        for it in range(2):
            for rank in range(world):
                cols, nrows, passed, scanned, segments = got[rank][2 * i + it]
                assert (passed, scanned, segments) == (st["passed_recs"], st["scanned_recs"], st["scanned_segments"]), (i, it, rank)
                assert nrows == (st["output_recs"] if rank == root else 0), (i, it, rank, nrows, st["output_recs"])
                if rank == root:
                    for c, (a, b) in enumerate(zip(cols, want)):
                        assert len(a) == len(b) and np.array_equal(a.astype(np.int64), np.asarray(b).astype(np.int64)), (i, it, c)
