"""W ranks of a sharded query as W threads of ONE process: every rank has its own vh_table and its own vh_comm, and the communicators talk
through a table of callbacks (vh_comm_init_custom) whose collectives meet on a threading.Barrier. The library keeps its per-query state
in thread_locals, so the whole protocol of vh_query_agg_sharded / vh_query_select_sharded runs at any world size on one GPU, without a
process launcher. What this does not cover is RCCL itself (tests/test_gpu_distributed.py::test_one_rank_through_rccl).

The callbacks are those of distributed.GlooTransport: a rank-major host all-gather, an in-place reduce of a device buffer (root < 0: an
all-reduce; integer SUM wraps in the element's own type, unsigned MIN / MAX compare unsigned, floats are added in rank order) and a ragged
all-to-all over several columns (sender q's block lands at recv_off[q]; empty blocks and null pointers of empty columns are fine). Bytes
move through distributed._Mem, after a hipStreamSynchronize on the stream the library passes.

A collective is two barrier waits: everyone has posted its payload / everyone has read what it needs. A Python exception inside a callback
is recorded, breaks the barrier and makes the callback return 1; the peers then get BrokenBarrierError out of their wait and return 1 too,
so a wedged protocol ends as a failed test and not as a hang (the barrier's 60 s are that guard, not a performance figure)."""
import ctypes as C
import threading
import time

import numpy as np

from viyadb_amd import capi, distributed

RED_SUM, RED_MIN, RED_MAX = distributed.RED_SUM, distributed.RED_MIN, distributed.RED_MAX


def reduce_arrays(arrays, op):
    """What a reduce leaves: `arrays` (one per rank, same dtype and length) combined in rank order, in their own dtype."""
    acc = arrays[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for a in arrays[1:]:
            acc = acc + a if op == RED_SUM else np.minimum(acc, a) if op == RED_MIN else np.maximum(acc, a)
    return acc


class ThreadTransport:
    """The meeting point of `world` rank threads. `endpoint(rank)` is one rank's side of it: .ops (capi.CommOps), .errors, .calls."""

    def __init__(self, world):
        self.world = int(world)
        self.barrier = threading.Barrier(self.world, timeout=60)
        self.slots = [None] * self.world
        self.mem = distributed._Mem()
        self.lock = threading.Lock()
        self.errors = []                                   # (rank, repr of the exception), in the order they happened
        self.endpoints = [_Endpoint(self, r) for r in range(self.world)]

    def endpoint(self, rank):
        return self.endpoints[rank]

    def comm(self, rank):
        """A vh_comm of this rank over the callbacks (needs vh_init)."""
        ep = self.endpoints[rank]
        h = C.c_void_p()
        capi.check(capi.load().vh_comm_init_custom(C.byref(ep.ops), rank, self.world, C.byref(h)))
        return distributed.Comm(h, rank, self.world, ep)

    def abort(self):
        self.barrier.abort()


class _Endpoint:
    def __init__(self, transport, rank):
        self.t, self.rank, self.world = transport, rank, transport.world
        self.errors = []
        self.calls = {"allgather": 0, "reduce": 0, "alltoallv": 0}
        self.fail_next = None                              # a test's hook: an exception to raise inside this rank's next callback
        self.ops = capi.CommOps(None, capi.CommOps.ALLGATHER(self._allgather), capi.CommOps.REDUCE(self._reduce),
                                capi.CommOps.ALLTOALLV(self._alltoallv))

    def _guard(self, fn, *a):
        try:
            if self.fail_next is not None:
                e, self.fail_next = self.fail_next, None
                raise e
            fn(*a)
            return 0
        except Exception as e:   # noqa: BLE001 - a Python exception must not unwind through C
            self.errors.append(repr(e))
            with self.t.lock:
                self.t.errors.append((self.rank, repr(e)))
            self.t.barrier.abort()
            return 1

    def _meet(self, payload):
        """Post `payload`, wait for everyone's; -> the ranks' payloads. `_part()` when they have been read."""
        self.t.slots[self.rank] = payload
        self.t.barrier.wait()
        return list(self.t.slots)

    def _part(self):
        self.t.barrier.wait()

    # -- host all-gather, rank-major
    def _allgather(self, ctx, send, recv, nbytes):
        return self._guard(self.allgather, send, recv, nbytes)

    def allgather(self, send, recv, nbytes):
        self.calls["allgather"] += 1
        nbytes = int(nbytes)
        mine = np.frombuffer((C.c_char * nbytes).from_address(send), dtype=np.uint8).copy() if nbytes else np.empty(0, dtype=np.uint8)
        everyone = np.concatenate(self._meet(mine))
        self._part()
        if everyone.size != nbytes * self.world:
            raise ValueError("all-gather: the ranks posted %d bytes, %d x %d expected" % (everyone.size, self.world, nbytes))
        if nbytes:
            C.memmove(recv, everyone.ctypes.data, everyone.size)

    # -- in-place reduce of a device buffer
    def _reduce(self, ctx, buf, count, elem, op, root, stream):
        return self._guard(self.reduce, buf, count, elem, op, root, stream)

    def reduce(self, buf, count, elem, op, root, stream):
        self.calls["reduce"] += 1
        self.t.mem.sync(stream)
        dt = np.dtype(capi.ELEM_NP[elem])
        mine = self.t.mem.read(buf, int(count) * dt.itemsize).view(dt)
        posted = self._meet((mine, int(elem), int(op), int(root)))
        self._part()
        if any(p[1:] != posted[0][1:] or len(p[0]) != len(mine) for p in posted):
            raise ValueError("reduce: the ranks disagree on (count, elem, op, root): %r" % [(len(p[0]),) + p[1:] for p in posted])
        if root < 0 or root == self.rank:
            self.t.mem.write(buf, reduce_arrays([p[0] for p in posted], op))

    # -- ragged all-to-all over several columns
    def _alltoallv(self, ctx, ncols, send, recv, esize, send_off, recv_off, stream):
        return self._guard(self.alltoallv, ncols, send, recv, esize, send_off, recv_off, stream)

    def alltoallv(self, ncols, send, recv, esize, send_off, recv_off, stream):
        self.calls["alltoallv"] += 1
        self.t.mem.sync(stream)
        W = self.world
        so = [int(send_off[p]) for p in range(W + 1)]
        ro = [int(recv_off[p]) for p in range(W + 1)]
        es = [int(esize[c]) for c in range(ncols)]
        cols = [self.t.mem.read(send[c], so[W] * es[c]) if so[W] else np.empty(0, dtype=np.uint8) for c in range(ncols)]
        posted = self._meet((so, es, cols))
        self._part()
        for q, (qso, qes, qcols) in enumerate(posted):
            if qes != es:
                raise ValueError("all-to-all: rank %d sends columns of %r bytes, rank %d expects %r" % (q, qes, self.rank, es))
            n = qso[self.rank + 1] - qso[self.rank]
            if n != ro[q + 1] - ro[q]:
                raise ValueError("all-to-all: rank %d sends %d rows to rank %d, which expects %d" % (q, n, self.rank, ro[q + 1] - ro[q]))
            for c in range(ncols):
                if n:
                    self.t.mem.write(recv[c] + ro[q] * es[c], qcols[c][qso[self.rank] * es[c]:qso[self.rank + 1] * es[c]])


def run_threads(transport, fn, timeout=240):
    """fn(rank, transport.endpoint(rank)) on one daemon thread per rank -> the ranks' results. The first exception (in time) is re-raised;
    a thread still alive after `timeout` seconds breaks the barrier and fails the test."""
    world = transport.world
    results, failures = [None] * world, []

    def body(rank):
        try:
            results[rank] = fn(rank, transport.endpoint(rank))
        except BaseException as e:   # noqa: BLE001 - carried to the test's thread
            with transport.lock:
                failures.append((rank, e))
            transport.abort()                              # peers waiting for this rank get BrokenBarrierError, not a timeout

    threads = [threading.Thread(target=body, args=(r,), daemon=True, name="rank%d" % r) for r in range(world)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        transport.abort()
        raise AssertionError("rank threads still running after %d s: %s; transport errors: %r" % (timeout, alive, transport.errors))
    if failures:
        rank, e = failures[0]
        raise e
    return results


def run_ranks(world, fn, timeout=240):
    """fn(rank, comm) on `world` daemon threads, comm being the rank's distributed.Comm over a ThreadTransport (comm.transport: its
    endpoint, with .calls and .errors) -> the ranks' results. Every communicator is closed, whatever happens."""
    transport = ThreadTransport(world)

    def body(rank, endpoint):
        comm = transport.comm(rank)
        try:
            return fn(rank, comm)
        finally:
            comm.close()
    return run_threads(transport, body, timeout)
