"""The cases of tests/test_gpu_background_build.py, one per fresh process (`python -m tests.background_cases NAME`): the JIT cache directory is
read once per process, so "this shape was never compiled" is a fact only in a process that starts with an empty one. Every answer is compared
with oracle/viya_oracle.py for the snapshot the query took, at the project's bar (tests/parity.compare)."""
import os
import sys
import threading
import time

import numpy as np

from oracle import synth as osynth
from oracle import viya_oracle as vo
from tests.parity import compare
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, DeviceTable

J = capi.PLAN_FORCE_JIT
PENDING = capi.INFO_BUILD_PENDING
SEG = 250_000
WAIT_MS = 120_000      # a cap against a hang: two hundred times the 0.43 s recorded for this compile, not a measurement


class Twin:
    """A C3 table on the device and the same rows for the oracle, loaded from arrays this test owns (so that it can sync changes)."""

    def __init__(self, nseg=4, last_rows=SEG, background=False, seed=42):
        self.w = synth.c3(segment_rows=SEG)
        self.dt = DeviceTable([(c.kind, c.elem) for c in self.w.columns], SEG, nseg)
        self.cols = []
        for s in range(nseg):
            rows = SEG
            self.cols.append([osynth.gen_column(ci, capi.ELEM_NP[c.elem], c.gen, seed, s * SEG, rows) for ci, c in enumerate(self.w.columns)])
        self.rows = [SEG] * (nseg - 1) + [last_rows]
        for s in range(nseg):
            self.dt.sync_segment(s, self.cols[s], self.rows[s])
        if background:
            self.dt.set_build_mode(True)
        self.plan = AggPlan(filter=self.w.plan.filter, groups=self.w.plan.groups, metrics=self.w.plan.metrics, seg_rows=None, flags=J,
                            groups_hint=self.w.plan.groups_hint)

    def oracle(self, nseg=None, query=None):
        t = vo.Table(self.w.table_json())
        for s, cols in enumerate(self.cols[:nseg]):
            n = self.rows[s]
            dims = [a[:n].copy() for a, c in zip(cols, self.w.columns) if c.kind < 16]
            mets = [a[:n].copy() for a, c in zip(cols, self.w.columns) if c.kind >= 16]
            t.add_segment_arrays(dims, mets, None, n)
        return vo.scan_aggregate(vo.parse_query(t, query or self.w.query), now=getattr(self.w, "now", None))

    def query(self, label, st=None):
        res = self.dt.query_agg(self.plan)
        compare(res, st if st is not None else self.oracle(), label)
        return res

    def close(self):
        self.dt.close()


def hold(what):
    if what:
        os.environ["VH_TEST_BUILD_HOLD"] = what
    else:
        os.environ.pop("VH_TEST_BUILD_HOLD", None)


def jobs_ever(bi):
    return bi.jobs_queued + bi.jobs_running + bi.jobs_done + bi.jobs_failed + bi.jobs_cancelled


def history(tw, background):
    """Six queries, (background: the worker released and waited for,) one more. Returns the last query's flags."""
    st = tw.oracle()
    queued = []
    for i in range(6):
        res = tw.query(f"query {i}", st)
        bi = tw.dt.build_info()
        print(f"query {i}: flags {res.flags:#x} queued {bi.jobs_queued} running {bi.jobs_running} inline {bi.inline_builds}", flush=True)
        if background:
            assert not res.flags & capi.INFO_JIT, "a compiled kernel ran while the worker was held"
            assert res.flags & PENDING, f"query {i}: the pending bit is clear"
            assert bi.inline_builds == 0
            assert bi.jobs_queued >= 1
            queued.append(bi.jobs_queued)
    if background:
        assert queued[5] == queued[4] == queued[3], f"jobs keep being queued for one shape: {queued}"      # (the third query asks for the layouts; from then on nothing new)
        hold(None)
        bi = tw.dt.build_wait(WAIT_MS)
        print(f"after the wait: done {bi.jobs_done} failed {bi.jobs_failed} compiled {bi.kernels_compiled} cached {bi.kernels_cached} layouts {bi.layouts_built} "
              f"compile_ms {bi.compile_ms:.1f} layout_ms {bi.layout_ms:.1f} lock_ms {bi.lock_ms:.3f}", flush=True)
        assert bi.jobs_queued == 0 and bi.jobs_running == 0
    else:
        tw.query("query 6", st)
    res = tw.query("last query", st)
    bi = tw.dt.build_info()
    print(f"last query: flags {res.flags:#x} inline {bi.inline_builds}", flush=True)
    assert res.flags & capi.INFO_JIT, f"no compiled kernel in the steady state: {res.flags:#x}"
    for name in ("PACKED", "PACK_BITS", "SLICED"):
        assert res.flags & getattr(capi, "INFO_" + name), f"{name} clear in the steady state: {res.flags:#x}"
    if background:
        assert not res.flags & PENDING
        assert bi.compile_ms > 0 and bi.kernels_compiled >= 1
        assert bi.inline_builds == 0
    else:
        assert bi.inline_builds > 0
        assert jobs_ever(bi) == 0
    return res.flags


def case_held_then_released():
    """Cases 1 and 2: the same history on a background table (worker held, then released) and on an inline twin; the modes converge."""
    hold("start")
    a = Twin(background=True)
    arenas = a.dt.info()[2]
    fa = history(a, True)
    a.dt.unpack()          # what the worker published goes out of the table's byte ledger as it came in
    assert a.dt.info()[2] == arenas, f"device_bytes {a.dt.info()[2]} after vh_table_unpack, {arenas} before the first query"
    a.close()
    b = Twin(background=False)
    fb = history(b, False)
    b.close()
    assert fa & ~PENDING == fb & ~PENDING, f"steady states differ: background {fa:#x}, inline {fb:#x}"


def wait_running(dt, seconds=30):
    t0 = time.time()
    while time.time() - t0 < seconds:
        if dt.build_info().jobs_running:
            time.sleep(0.3)      # (the job reaches its hold within milliseconds of starting)
            return
        time.sleep(0.01)
    raise AssertionError("no build job started")


PRED_COLS, M0, COUNT = [2, 3, 4], 7, 9      # C3: the filter's columns d2, d3, d4; SUM(m0) and COUNT


def passing_row(cols):
    m = (cols[2] == 1) & (cols[3] < 447) & (cols[4] >= 553)
    return int(np.nonzero(m)[0][10])


def hold_the_projection_job(tw):
    """Three queries with the worker held before `publish`. The narrow copies and the predicate projection were built by explicit calls before,
    so the ONE job the third query queues — and the one that waits between (b) and (c) — is the payload projection of (d0, d1, m0, count)."""
    hold("publish")
    before = tw.dt.build_info()
    for i in range(3):
        tw.query(f"sighting {i}")
    t0 = time.time()
    while time.time() - t0 < 60:                 # (a kernel job of the first sighting may still be compiling: the projection job comes after it)
        bi = tw.dt.build_info()
        if bi.jobs_running == 1 and bi.jobs_queued == 0 and bi.jobs_done + bi.jobs_failed + bi.jobs_declined > before.jobs_done + before.jobs_failed + before.jobs_declined - 1:
            time.sleep(0.5)
            bi = tw.dt.build_info()
            if bi.jobs_running == 1 and bi.jobs_queued == 0 and bi.kernels_compiled + bi.kernels_cached == tw.dt.build_info().kernels_compiled + bi.kernels_cached:
                break
        time.sleep(0.01)
    time.sleep(1.0)                              # (a compile takes about half a second: what still runs a second later is the held job)
    bi = tw.dt.build_info()
    assert bi.jobs_running == 1 and bi.jobs_queued == 0, (bi.jobs_running, bi.jobs_queued)
    assert bi.layouts_built == before.layouts_built, "the held job has published"
    return before


def case_sync_during_build():
    """Case 3. A projection job waits before it publishes; a batch appends rows and rewrites metrics inside rows the job has read. Then the same
    with a synced value that outgrows its bit field: the layout is absent or rebuilt wider, never used at the stale width."""
    tw = Twin(background=True, last_rows=200_000)
    tw.dt.narrow(PRED_COLS)
    tw.dt.predpack(PRED_COLS)                    # (the library's form: bit-sliced)
    before = hold_the_projection_job(tw)
    rng = np.random.default_rng(7)
    for ci in (M0, COUNT):
        a = tw.cols[1][ci]
        a[1000:5000] = rng.integers(1, 3, 4000).astype(a.dtype)        # (values every field holds: nothing outgrown)
    tw.rows[3] = SEG
    only_metrics = [a if tw.w.columns[ci].kind >= 16 else None for ci, a in enumerate(tw.cols[1])]
    tw.dt.sync_batch([(3, 200_000, 50_000, SEG, tw.cols[3], 0), (1, 1000, 4000, SEG, only_metrics, capi.SYNC_METRICS_ONLY)])
    res = tw.query("during the hold")
    assert not res.flags & capi.INFO_PACKED and res.flags & PENDING, f"{res.flags:#x}"
    hold(None)
    bi = tw.dt.build_wait(WAIT_MS)
    print(f"first half: layouts {bi.layouts_built} done {bi.jobs_done} declined {bi.jobs_declined} restarts {bi.layout_restarts} failed {bi.jobs_failed}", flush=True)
    assert bi.layouts_built == before.layouts_built + 1 and bi.jobs_failed == 0 and bi.jobs_declined == 0
    res = tw.query("after the sync")
    print(f"flags {res.flags:#x} record bytes {capi.info_rec_bytes(res.flags)}", flush=True)
    assert res.flags & capi.INFO_PACKED and res.flags & capi.INFO_JIT and not res.flags & PENDING, f"no projection in use: {res.flags:#x}"
    assert tw.dt.build_info().inline_builds == 0
    narrow_bytes = capi.info_rec_bytes(res.flags)
    assert narrow_bytes == 4, "C3's projection is a 4-byte bit-field record"

    # ---- a value that outgrows its field, in a row that passes the filter, while the next projection waits before it publishes
    tw.dt.unpack()
    tw.dt.narrow(PRED_COLS)
    tw.dt.predpack(PRED_COLS)
    before = hold_the_projection_job(tw)
    row = passing_row(tw.cols[2])
    a = tw.cols[2][M0]
    a[row] = 1 << 40                              # m0's field was sized for values below 1001
    first = row // 256 * 256
    only = [b if k == M0 else None for k, b in enumerate(tw.cols[2])]
    tw.dt.sync_batch([(2, first, 256, SEG, only, capi.SYNC_METRICS_ONLY)])
    hold(None)
    bi = tw.dt.build_wait(WAIT_MS)
    print(f"second half: layouts {bi.layouts_built} (before {before.layouts_built}) done {bi.jobs_done} declined {bi.jobs_declined} (before {before.jobs_declined}) "
          f"restarts {bi.layout_restarts} failed {bi.jobs_failed}", flush=True)
    for label in ("after the wide value", "after the wide value, again"):
        res = tw.query(label)                     # (the oracle's rows include the wide value's group)
        print(f"{label}: flags {res.flags:#x} record bytes {capi.info_rec_bytes(res.flags)}", flush=True)
        assert not res.flags & capi.INFO_PACKED or capi.info_rec_bytes(res.flags) > narrow_bytes, f"a projection at the stale width is in use: {res.flags:#x}"
    bi = tw.dt.build_wait(WAIT_MS)
    res = tw.query("after the rebuild")
    print(f"after the rebuild: flags {res.flags:#x} record bytes {capi.info_rec_bytes(res.flags)}", flush=True)
    assert not res.flags & capi.INFO_PACKED or capi.info_rec_bytes(res.flags) > narrow_bytes
    bi = tw.dt.build_info()
    # the projection the held job built was not kept as it was: it was voided at its first refresh and replaced (one more published), or declined
    assert bi.layouts_built + bi.jobs_declined >= before.layouts_built + before.jobs_declined + 1
    assert bi.jobs_failed == 0 and bi.inline_builds == 0
    tw.close()


def case_hashed_partitioning():
    """Case 4: a count-distinct plan forced onto the hashed partitioning. Pending: the plain hash table; ready: bit 6. The oracle's rows both times."""
    from tests.test_gpu_hpart import HP, sets_table
    from tests.test_gpu_typed import F, run
    from tests.planner import mirror_table
    tab = sets_table(3, n=20_000, nseg=2, seed=23)
    dt = mirror_table(tab)
    dt.set_build_mode(True)
    q = {"dimensions": ["c", "x"], "metrics": ["users", "count"], "filter": F("lt", "x", "70")}
    hold("start")
    res, _ = run(tab, dt, q, flags=HP)
    print(f"pending: flags {res.flags:#x} path {res.path} kernel {res.kernel}", flush=True)
    assert res.path == "hash" and not res.flags & capi.INFO_HPART and not res.flags & capi.INFO_JIT and res.flags & PENDING, f"{res.flags:#x}"
    assert dt.build_info().jobs_queued >= 1
    hold(None)
    bi = dt.build_wait(WAIT_MS)
    assert bi.kernels_compiled >= 1 and bi.jobs_failed == 0
    res, _ = run(tab, dt, q, flags=HP)
    print(f"ready: flags {res.flags:#x} kernel {res.kernel}", flush=True)
    assert res.flags & capi.INFO_HPART and res.flags & capi.INFO_JIT and not res.flags & PENDING, f"{res.flags:#x}"
    assert dt.build_info().inline_builds == 0
    dt.close()


def case_readers_writer_build():
    """Case 5: four threads querying two plan shapes, one thread appending segments (the table grows: its arenas are replaced), the worker
    released half-way. Every answer equals the oracle's for the snapshot that call took."""
    from viyadb_amd.executor import GroupSpec
    first, total, iters = 4, 8, 24
    tw = Twin(nseg=first, background=True)
    for s in range(first, total):
        tw.cols.append([osynth.gen_column(ci, capi.ELEM_NP[c.elem], c.gen, 42, s * SEG, SEG) for ci, c in enumerate(tw.w.columns)])
        tw.rows.append(SEG)
    q2 = dict(tw.w.query, dimensions=["d0"], metrics=["m0"])
    shapes = [(tw.w.query, tw.w.plan.groups, [M0, COUNT]), (q2, [GroupSpec(0)], [M0])]
    want = {(k, n): tw.oracle(n, shapes[k][0]) for k in range(2) for n in range(first, total + 1)}
    synced, errors, done = [first], [], [0] * 4
    hold("start")

    def reader(i):
        try:
            k = i % 2
            for it in range(iters):
                n = synced[0]                      # the snapshot: whatever the writer finished before this call
                plan = AggPlan(filter=tw.w.plan.filter, groups=shapes[k][1], metrics=shapes[k][2], seg_rows=[SEG] * n, flags=J)
                compare(tw.dt.query_agg(plan), want[(k, n)], f"reader {i} iteration {it} segments {n}")
                done[i] = it + 1
        except Exception as e:   # noqa: BLE001
            errors.append((i, repr(e)))

    def writer():
        try:
            for s in range(first, total):
                time.sleep(0.05)
                tw.dt.sync_segment(s, tw.cols[s], SEG)
                synced[0] = s + 1
        except Exception as e:   # noqa: BLE001
            errors.append(("writer", repr(e)))

    threads = [threading.Thread(target=reader, args=(i,)) for i in range(4)] + [threading.Thread(target=writer)]
    for th in threads:
        th.start()
    while min(done) < iters // 2 and not errors and any(th.is_alive() for th in threads[:4]):
        time.sleep(0.005)
    hold(None)
    tw.dt.build_info()                            # (the hook is read on calling threads)
    for th in threads:
        th.join()
    assert not errors, errors[:3]
    bi = tw.dt.build_wait(WAIT_MS)
    print(f"done {bi.jobs_done} declined {bi.jobs_declined} failed {bi.jobs_failed} layouts {bi.layouts_built} restarts {bi.layout_restarts} compiled {bi.kernels_compiled} "
          f"warm {bi.warm_queries} inline {bi.inline_builds}", flush=True)
    assert bi.jobs_failed == 0 and bi.inline_builds == 0 and bi.kernels_compiled >= 1
    for k in range(2):
        plan = AggPlan(filter=tw.w.plan.filter, groups=shapes[k][1], metrics=shapes[k][2], seg_rows=None, flags=J)
        res = tw.dt.query_agg(plan)
        compare(res, want[(k, total)], f"shape {k} at the end")
        print(f"shape {k} at the end: flags {res.flags:#x}", flush=True)
    tw.close()


def case_host_shim():
    """Case 7: a reference case through the host shim with background builds: build_pending on the first query, clear after the worker is done,
    the reference's rows both times. (VIYA_HIP_PLAN_FLAGS = VH_PLAN_FORCE_JIT in this process: the case's table is far below VH_JIT_MIN_ROWS.)"""
    from tests import golden_cases as gc
    from viyadb_amd import hostdb
    seen = {}

    def run_bg(tconf, loads, query, now):
        db = hostdb.Database({"tables": [tconf]})
        try:
            db.set_background_builds(True)
            for batch in loads:
                db.load(tconf["name"], batch, now=now)
            hold("start")
            rows, stats = db.query(query, now=now)
            seen["first"] = (rows, stats)
            hold(None)
            t0 = time.time()
            while True:                               # (the facade has no wait of its own: the next queries tell)
                rows2, stats2 = db.query(query, now=now)
                if not stats2["build_pending"] or time.time() - t0 > WAIT_MS / 1000:
                    break
                time.sleep(0.05)
            seen["after"] = (rows2, stats2)
            ti = db.table_info(tconf["name"])
            return rows2, stats2, {"segments": ti["segments"], "segment_sizes": [ti["first_segment_size"]]}
        finally:
            db.close()

    case = gc.case_by_id("aggregation.BasicQuery")
    gc.check_case(case, run_bg)
    (rows1, st1), (rows2, st2) = seen["first"], seen["after"]
    print(f"first: pending {st1['build_pending']} compile_ms {st1['compile_ms']:.1f}; after: pending {st2['build_pending']} compile_ms {st2['compile_ms']:.1f}", flush=True)
    assert st1["build_pending"] == 1 and st2["build_pending"] == 0
    assert sorted(map(list, rows1)) == sorted(map(list, rows2))
    assert st2["compile_ms"] > 0


def case_lifetimes():
    """Case 6: tables destroyed and unpacked under the worker's feet, vh_table_prepare joining a held job; the process goes on answering."""
    other = Twin(nseg=2)
    hold("start")
    d = Twin(background=True)
    d.query("d0")                   # (first in this process: nothing has compiled the shape yet)
    assert d.dt.build_info().jobs_queued >= 1
    threading.Timer(0.5, lambda: (hold(None), d.dt.build_info())).start()      # released by a second thread after vh_table_prepare began
    d.dt.warm(d.plan)               # vh_table_prepare
    bi = d.dt.build_info()
    print(f"prepare: compiled {bi.kernels_compiled} cached {bi.kernels_cached} done {bi.jobs_done}", flush=True)
    assert bi.kernels_compiled == 1, "the held shape was compiled by the worker, once"
    res = d.query("d after prepare")
    assert res.flags & capi.INFO_JIT
    d.close()
    hold("start")
    a = Twin(background=True)
    for i in range(3):
        a.query(f"a{i}")
    assert a.dt.build_info().jobs_queued >= 2
    a.close()                       # jobs held at `start`
    hold("publish")
    b = Twin(background=True)
    for i in range(3):
        b.query(f"b{i}")
    wait_running(b.dt)
    b.close()                       # a layout job held at `publish`
    hold(None)
    c = Twin(background=True)
    for i in range(3):
        c.query(f"c{i}")
    c.dt.unpack()                   # with layout jobs queued or running
    c.query("c after unpack")
    c.dt.build_wait(WAIT_MS)
    c.query("c after the wait")
    c.close()
    other.plan.flags = 0
    other.query("another table")
    other.close()


if __name__ == "__main__":
    executor.init(0)
    {"held_then_released": case_held_then_released, "sync_during_build": case_sync_during_build, "hashed_partitioning": case_hashed_partitioning,
     "readers_writer_build": case_readers_writer_build, "lifetimes": case_lifetimes, "host_shim": case_host_shim}[sys.argv[1]]()
    print("case ok", flush=True)
