"""select and search over a table sharded across GPUs: vh_query_select_sharded, global storage positions (VH_COL_ROWID) in
vh_query_agg_sharded, and the host shim's select / search on a joined node. As in test_gpu_distributed.py, two ranks share
cuda:0 over the gloo callback transport and one rank goes through RCCL proper (world 1 with the protocol forced on); each
launch is a torch.distributed.run subprocess. Every expectation is the oracle over one table holding all ranks' segments in
rank order, or one device table / one database holding them."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import sharded_rows_data as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scenario -> [(filter, skip, limit, root)]
SELECTS = {
    "ragged": [(D.FILTER, 0, 0, 0),               # no limit
               (D.FILTER, 3500, 0, 0),            # the skip ends inside rank 1 (rank 0 passes ~2 900 rows)
               (D.FILTER, 5, 50, 0),              # the limit is reached inside rank 0: each later segment sends its first row
               (D.BITSET_FILTER, 7, 0, 1),        # a filter on a bitset metric, delivered on rank 1
               (D.FILTER, 10, 20, 1)],
    "rank1_empty": [(D.FILTER, 0, 30, 0), (D.FILTER, 0, 0, 1)],
    "rank0_empty": [(D.FILTER, 3, 40, 0), (D.FILTER, 0, 0, 0)],
    "rank1_nopass": [(D.FILTER, 0, 0, 0), (D.FILTER, 2, 10, 1)],
}
POSITION_FLAGS = (0, 1)                           # the dense organisation a small dimension gets, and VH_PLAN_FORCE_HASH

WORKER = textwrap.dedent('''
    import os, sys, json, time
    sys.path.insert(0, {root!r})
    import numpy as np, torch, torch.distributed as dist
    from viyadb_amd import capi, distributed, executor
    from oracle import viya_oracle as vo
    from tests import sharded_rows_data as D
    from tests.planner import mirror_table, plan_from_query
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    executor.init(0)
    comm = distributed.Comm.rccl(dist) if {backend!r} == "rccl" else distributed.Comm.gloo(dist)
    selects, flags_list = {selects!r}, {flags!r}
    out = {{}}
    for name, cases in selects.items():
        tab = D.shard(name, rank) if world > 1 else D.whole(name)
        t = mirror_table(tab, reserve=max(1, len(tab.segments)))
        for i, (flt, skip, limit, root) in enumerate(cases):
            aq = vo.parse_query(tab, {{"type": "aggregate", "table": "t", "dimensions": [], "metrics": [], "filter": flt}})
            filt = plan_from_query(tab, aq).filter
            root = min(root, world - 1)
            t0 = time.perf_counter()
            cols, info = distributed.sharded_select(t, filt, D.COLS, comm, skip=skip, limit=limit, root=root)
            ms = (time.perf_counter() - t0) * 1e3
            out["select/%s/%d" % (name, i)] = {{"cols": [c.tolist() for c in cols], "nrows": info.nrows, "passed": info.passed_recs,
                                               "scanned": info.scanned_recs, "segments": info.scanned_segments, "root": root, "ms": ms}}
        if name in ("ragged", "rank0_empty"):
            aq = vo.parse_query(tab, {{"type": "aggregate", "table": "t", "dimensions": ["a"], "metrics": ["count"], "filter": D.FILTER}})
            for flags in flags_list:
                plan = plan_from_query(tab, aq, flags=flags)
                plan.metrics = [capi.COL_ROWID]
                runs = []
                for it in range(2):                   # the second run takes the cached agreement (a dense one: the fused step)
                    t0 = time.perf_counter()
                    res = distributed.sharded_query(t, plan, comm, root=0)
                    runs.append(((time.perf_counter() - t0) * 1e3, sorted(zip(res.keys[0].tolist(), [int(x) for x in res.states[0]]))))
                out["search/%s/%d" % (name, flags)] = {{"pairs": runs[0][1], "pairs_again": runs[1][1], "path": res.path,
                                                      "passed": res.passed_recs, "scanned": res.scanned_recs, "ms": [r[0] for r in runs]}}
        t.close()
    torch.cuda.synchronize()
    json.dump(out, open({out!r} + ".%d.json" % rank, "w"))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()
''')


def _run(script, nproc, env=None):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
                        "127.0.0.1", "--master-port", str(port), str(script)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])


def _launch(tmp_path, backend, nproc, selects, flags, env=None):
    out = str(tmp_path / "res")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=out, backend=backend, selects=selects, flags=flags))
    _run(script, nproc, env)
    return [json.load(open(out + ".%d.json" % k)) for k in range(nproc)]


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return _launch(tmp_path_factory.mktemp("sharded_rows"), "gloo", 2, SELECTS, POSITION_FLAGS)


def _check_selects(gots, selects):
    for name, cases in selects.items():
        whole = D.whole(name)
        for i, (flt, skip, limit, root) in enumerate(cases):
            key = "select/%s/%d" % (name, i)
            want, st = D.oracle_select(whole, flt, skip, limit)
            root = gots[0][key]["root"]
            for k, g in enumerate(gots):
                r = g[key]
                assert (r["passed"], r["scanned"], r["segments"]) == (st["passed_recs"], st["scanned_recs"], st["scanned_segments"]), (key, k)
                assert r["nrows"] == (st["output_recs"] if k == root else 0), (key, k, r["nrows"], st["output_recs"])
            for c, (a, b) in enumerate(zip(gots[root][key]["cols"], want)):
                assert len(a) == len(b) and np.array_equal(np.array(a, dtype=np.int64), b.astype(np.int64)), (key, c)


def test_select_two_ranks(two_ranks):
    _check_selects(two_ranks, SELECTS)


def test_select_windows_cross_the_rank_boundary():
    """The scenarios above do what their comments say: the skip ends inside rank 1, the limit inside rank 0, rank 1's
    segments then each send one row, and a bitset column / filter is in play."""
    whole, r0 = D.whole("ragged"), D.shard("ragged", 0)
    _, s0 = D.oracle_select(r0, D.FILTER, 0, 0)
    _, sw = D.oracle_select(whole, D.FILTER, 0, 0)
    assert s0["passed_recs"] < 3500 < sw["passed_recs"]
    _, sl = D.oracle_select(whole, D.FILTER, 5, 50)
    assert sl["output_recs"] == 50 + (len(D.SIZES) - 1)
    want, sb = D.oracle_select(whole, D.BITSET_FILTER, 7, 0)
    assert sb["output_recs"] > 0 and np.all(want[5] > 2)


def _positions_single(flags):
    from oracle import viya_oracle as vo
    from tests.planner import mirror_table, plan_from_query
    from viyadb_amd import capi, executor
    executor.init(0)
    whole = D.whole("ragged")
    t = mirror_table(whole, reserve=len(whole.segments))
    try:
        aq = vo.parse_query(whole, {"type": "aggregate", "table": "t", "dimensions": ["a"], "metrics": ["count"], "filter": D.FILTER})
        plan = plan_from_query(whole, aq, flags=flags)
        plan.metrics = [capi.COL_ROWID]
        res = t.query_agg(plan)
        return dict(zip(res.keys[0].tolist(), [int(x) for x in res.states[0]])), res.passed_recs
    finally:
        t.close()


def _check_positions(gots, names):
    for flags in POSITION_FLAGS:
        want, passed = _positions_single(flags)
        assert any(p >> 32 >= 3 for p in want.values())           # some first occurrences lie in rank 1's block
        for name in names:
            g = gots[0]["search/%s/%d" % (name, flags)]
            got = dict((k, p) for k, p in g["pairs"])
            assert got == want, (name, flags, {k: (hex(got.get(k, 0)), hex(v)) for k, v in want.items() if got.get(k) != v})
            assert g["pairs_again"] == g["pairs"], (name, flags)
            assert g["passed"] == passed
            assert g["path"] == "hash" if flags == 1 else g["path"] != "hash", (flags, g["path"])
            for other in gots[1:]:
                assert other["search/%s/%d" % (name, flags)]["pairs"] == []


def test_search_positions_are_global(two_ranks):
    _check_positions(two_ranks, ["ragged", "rank0_empty"])


def test_one_rank_through_rccl(tmp_path):
    """select and global positions through RCCL itself (grouped ncclSend / ncclRecv, root sending to itself), one rank."""
    selects = {"ragged": SELECTS["ragged"][:3]}
    gots = _launch(tmp_path, "rccl", 1, selects, POSITION_FLAGS, env={"VH_TEST_SHARDED_WORLD1": "1"})
    _check_selects(gots, selects)
    _check_positions(gots, ["ragged"])


HOST_WORKER = textwrap.dedent('''
    import os, sys, json, time
    sys.path.insert(0, {root!r})
    import numpy as np, torch, torch.distributed as dist
    from viyadb_amd import distributed, executor, hostdb
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    executor.init(0)
    comm = distributed.Comm.gloo(dist)
    spec = json.load(open({spec!r}))
    db = hostdb.Database({{}}, device=0)
    db.create_table(spec["table"])
    db.load("events", spec["rows"][rank], now=spec["now"])
    db.join_node(comm)
    out = []
    for q in spec["queries"]:
        t0 = time.perf_counter()
        rows, stats = db.query(q, now=spec["now"])
        out.append({{"rows": rows, "ms": (time.perf_counter() - t0) * 1e3,
                    "stats": {{k: stats[k] for k in ("scanned_recs", "scanned_segments", "aggregated_recs", "output_recs")}}}})
    json.dump(out, open({out!r} + ".%d.json" % rank, "w"))
    dist.barrier()
    db.close()
    comm.close()
    dist.destroy_process_group()
''')


def test_cxx_database_select_and_search_all_ranks_rows(tmp_path):
    """The C++ host shim end to end over two ranks (Database::JoinNode -> GpuSelect / GpuSearch): rank 0 returns what ONE
    database holding all rows returns — select with filter, skip and limit; search on string, time and numeric dimensions
    with a limit reached early, so that every later segment of both ranks adds its first new matching value — and rank 1
    returns nothing."""
    import random
    from viyadb_amd import executor, hostdb
    now = 1496570140
    table = {"name": "events", "segment_size": 500,
             "dimensions": [{"name": "country"}, {"name": "event", "cardinality": 100}, {"name": "t", "type": "time"}, {"name": "n", "type": "uint"}],
             "metrics": [{"name": "count", "type": "count"}, {"name": "revenue", "type": "double_sum"}, {"name": "users", "type": "bitset"}]}
    countries, events = ["US", "RU", "IL", "KZ", "CH", "AZ", "DE", "FR", "NL", "BE"], ["open", "purchase", "refund", "donate"]

    def make_rows(n, rank):
        r = random.Random(21 + rank)
        # every rank first sees every string once, in the same order: the same dictionary codes everywhere. No two rows share
        # their dimensions (n is unique), so that one database holding all rows stores every row as its own record (no upsert)
        rows = [[c, e, str(now - 1), str(rank), "0.5", "7"] for c in countries for e in events]
        for i in range(n):
            rows.append([countries[(i // 300 + r.randrange(0, 2)) % len(countries)], r.choice(events), str(now - r.randrange(0, 900) * 3600),
                         str(2 * i + 2 + rank), str(r.randrange(0, 4000) / 8.0), str(r.randrange(0, 300))])
        return rows
    rows = [make_rows(3000 - 40, 0), make_rows(4100, 1)]         # rank 0 fills exactly 6 segments: rank 1's rows start a new one
    queries = [
        {"type": "select", "table": "events", "dimensions": ["country", "t", "n"], "metrics": ["count", "revenue", "users"],
         "filter": {"op": "ne", "column": "event", "value": "refund"}, "skip": 40, "limit": 30, "header": True},
        {"type": "select", "table": "events", "dimensions": ["event", "n"], "metrics": ["revenue"],
         "filter": {"op": "eq", "column": "country", "value": "DE"}, "skip": 600, "header": True},
        {"type": "search", "table": "events", "dimension": "country", "term": "", "limit": 2, "header": True},
        {"type": "search", "table": "events", "dimension": "t", "term": "1496", "limit": 3,
         "filter": {"op": "gt", "column": "n", "value": "10"}, "header": True},
        {"type": "search", "table": "events", "dimension": "n", "term": "1", "limit": 4, "header": True},
    ]
    spec = str(tmp_path / "spec.json")
    json.dump({"table": table, "rows": rows, "queries": queries, "now": now}, open(spec, "w"))
    out = str(tmp_path / "out")
    script = tmp_path / "worker.py"
    script.write_text(HOST_WORKER.format(root=ROOT, spec=spec, out=out))
    _run(script, 2)
    got = [json.load(open(out + ".%d.json" % k)) for k in range(2)]
    executor.init(0)
    db = hostdb.Database({}, device=0)
    try:
        db.create_table(table)
        db.load("events", rows[0], now=now)
        db.load("events", rows[1], now=now)
        for k, q in enumerate(queries):
            want, st = db.query(q, now=now)
            assert got[0][k]["rows"] == want, (k, got[0][k]["rows"][:4], want[:4])
            assert got[1][k]["rows"] == [], k
            for f in ("scanned_recs", "scanned_segments", "aggregated_recs", "output_recs"):
                assert got[0][k]["stats"][f] == st[f], (k, f, got[0][k]["stats"][f], st[f])
            if q["type"] == "search":          # the later-segment rule was exercised, on both ranks' segments
                assert len(want[-1]) > q["limit"], (k, want)
            else:
                assert len(want) > 1, k
    finally:
        db.close()
