"""tests/thread_ranks.py without a GPU: host pointers stand in for device pointers (as in test_distributed_gloo.py) and the rank threads
call the three callbacks exactly as vh_comm_init_custom's caller would. Every expectation is written out with Python integers or a
rank-ordered float loop — never taken from the transport's own reduction."""
import ctypes as C
import time

import numpy as np
import pytest

from tests.thread_ranks import RED_MAX, RED_MIN, RED_SUM, ThreadTransport, run_threads
from viyadb_amd import capi

WORLDS = [1, 2, 3, 4, 8]
N = 37                                    # elements per reduced buffer (odd, no multiple of anything)


def roots(world):
    return sorted({-1, 0, world - 1})


# name -> (element type, reduce op, value of element i on rank r as a Python number)
REDUCES = {
    "u8_max": (capi.U8, RED_MAX, lambda r, i: (r * 37 + i * 11) % 256),
    "u32_sum_wraps": (capi.U32, RED_SUM, lambda r, i: 2 ** 32 - 1 - (r * 7 + i) % 5),
    "u64_sum_wraps": (capi.U64, RED_SUM, lambda r, i: 2 ** 64 - 1 - (r * 3 + i * i) % 11),
    "u32_min_both_sides_of_2_31": (capi.U32, RED_MIN, lambda r, i: 2 ** 31 + (1, -1, (-1) ** r)[i % 3] * (1 + r * 1000 + i)),      # all above / all below / mixed
    "u64_max_above_2_63": (capi.U64, RED_MAX, lambda r, i: 2 ** 63 + ((r * 2654435761 + i * 40503) % 2 ** 40 if (r + i) % 3 else -1 - r)),
    "i32_min_negatives": (capi.I32, RED_MIN, lambda r, i: -2 ** 31 + (r * 7919 + i * 104729) % 2 ** 32 if i % 4 else (r - 3) * (i + 1)),
    "i64_max": (capi.I64, RED_MAX, lambda r, i: (-1) ** (r + i) * (2 ** 62 + r * 2 ** 40 + i)),
    "f64_sum_rank_order": (capi.F64, RED_SUM, lambda r, i: [1e16, 1.0, -1e16, 3.0, 0.1, -1.0, 1e-3, 7.0][(r + i) % 8] * (1 + i % 3)),
}


def _ints_in_range(name, elem, values):
    if elem == capi.F64:
        return
    info = np.iinfo(capi.ELEM_NP[elem])
    assert all(info.min <= v <= info.max for row in values for v in row), name


def expected_reduce(elem, op, values):
    """values[r][i] -> the reduced array, by plain arithmetic: Python integers wrapped to the type's width, or a float loop in rank order."""
    dt = np.dtype(capi.ELEM_NP[elem])
    out = []
    for i in range(len(values[0])):
        col = [values[r][i] for r in range(len(values))]
        if op == RED_MIN:
            out.append(min(col))
        elif op == RED_MAX:
            out.append(max(col))
        elif dt.kind == "f":
            acc = col[0]
            for v in col[1:]:
                acc = acc + v                     # IEEE double additions, rank 0 first
            out.append(acc)
        else:
            out.append(sum(col) % (1 << (8 * dt.itemsize)))
    return np.array(out, dtype=object).astype(dt)


@pytest.mark.parametrize("world", WORLDS)
def test_reduce_every_type_and_root(world):
    for name, (elem, op, f) in REDUCES.items():
        dt = np.dtype(capi.ELEM_NP[elem])
        values = [[f(r, i) for i in range(N)] for r in range(world)]
        _ints_in_range(name, elem, values)
        want = expected_reduce(elem, op, values)
        if name == "u32_min_both_sides_of_2_31" and world > 1:
            assert (want > 2 ** 31).any() and (want < 2 ** 31).any()
        if name.endswith("wraps") and world > 1:
            assert all(sum(values[r][i] for r in range(world)) >= 2 ** (8 * dt.itemsize) for i in range(N))
        for root in roots(world):
            def rank_body(rank, ep):
                a = np.array(values[rank], dtype=object).astype(dt)
                rc = ep.ops.reduce_device(None, a.ctypes.data, N, elem, op, root, None)
                return rc, a
            tr = ThreadTransport(world)
            got = run_threads(tr, rank_body, timeout=90)
            assert tr.errors == [], (name, root, tr.errors)
            for rank, (rc, a) in enumerate(got):
                assert rc == 0, (name, root, rank)
                if root < 0 or rank == root:
                    assert a.tobytes() == want.tobytes(), (name, world, root, rank, a[:4], want[:4])
                else:                              # a rank that is not the root keeps its partial
                    assert a.tobytes() == np.array(values[rank], dtype=object).astype(dt).tobytes(), (name, world, root, rank)


def test_float_sum_order_matters_here():
    """The F64 case can tell rank order from another order: at world 3 the reversed order gives a different sum somewhere."""
    elem, op, f = REDUCES["f64_sum_rank_order"]
    values = [[f(r, i) for i in range(N)] for r in range(3)]
    assert expected_reduce(elem, op, values).tobytes() != expected_reduce(elem, op, values[::-1]).tobytes()


@pytest.mark.parametrize("world", WORLDS)
def test_allgather_is_rank_major(world):
    def rank_body(rank, ep):
        mine = np.array([rank, 10 + rank, 2 ** 63 + 20 + rank], dtype=np.uint64)
        everyone = np.zeros(3 * world, dtype=np.uint64)
        rc = ep.ops.allgather_host(None, mine.ctypes.data, everyone.ctypes.data, mine.nbytes)
        return rc, everyone, dict(ep.calls)
    want = np.array([v for r in range(world) for v in (r, 10 + r, 2 ** 63 + 20 + r)], dtype=np.uint64)
    for rank, (rc, everyone, calls) in enumerate(run_threads(ThreadTransport(world), rank_body, timeout=90)):
        assert rc == 0 and np.array_equal(everyone, want), (world, rank)
        assert calls == {"allgather": 1, "reduce": 0, "alltoallv": 0}


ESIZES = (1, 2, 4, 8)


def _sends(world, r, p):
    """Rows rank r sends to rank p: none to its right-hand neighbour, none to the last rank (which so receives nothing at all)."""
    if p == (r + 1) % world or p == world - 1:
        return 0
    return 1 + (3 * r + 5 * p) % 4


def _cell(r, j, c):
    """Row j of column c of rank r's send buffer: tells sender, row and column apart, cut to the column's width."""
    return (r * 1000003 + j * (2 * c + 3) + c * 77) % (1 << (8 * ESIZES[c]))


@pytest.mark.parametrize("world", WORLDS)
def test_ragged_exchange_of_four_column_widths(world):
    GUARD = 3                                  # elements behind every receive buffer that must stay untouched

    def rank_body(rank, ep):
        so = np.concatenate([[0], np.cumsum([_sends(world, rank, p) for p in range(world)])]).astype(np.uint64)
        ro = np.concatenate([[0], np.cumsum([_sends(world, q, rank) for q in range(world)])]).astype(np.uint64)
        send = [np.array([_cell(rank, j, c) for j in range(int(so[-1]))], dtype=object).astype("u%d" % ESIZES[c]) for c in range(4)]
        recv = [np.full(int(ro[-1]) + GUARD, 0xAB, dtype="u%d" % ESIZES[c]) for c in range(4)]
        sp = (C.c_void_p * 4)(*[a.ctypes.data for a in send])
        rp = (C.c_void_p * 4)(*[a.ctypes.data for a in recv])
        es = (C.c_uint32 * 4)(*ESIZES)
        rc = ep.ops.alltoallv_device(None, 4, sp, rp, es, so.ctypes.data_as(C.POINTER(C.c_uint64)), ro.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        return rc, recv
    tr = ThreadTransport(world)
    got = run_threads(tr, rank_body, timeout=90)
    assert tr.errors == []
    received = [0] * world
    for p, (rc, recv) in enumerate(got):
        assert rc == 0
        for c in range(4):
            want = []
            for q in range(world):               # sender q's block for p: the rows behind what q sends to the ranks below p
                start = sum(_sends(world, q, x) for x in range(p))
                want += [_cell(q, j, c) for j in range(start, start + _sends(world, q, p))]
            received[p] = len(want)
            assert recv[c][:len(want)].tolist() == want, (world, p, c)
            assert (recv[c][len(want):] == (0xAB if c == 0 else recv[c].dtype.type(0xAB))).all(), (world, p, c)
    assert received[world - 1] == 0
    if world > 2:
        assert all(n > 0 for n in received[:-1]), received


def test_null_pointers_of_empty_columns_are_not_touched():
    """The gather on a root: the other ranks receive nothing and pass no receive buffer at all."""
    world, root = 3, 1

    def rank_body(rank, ep):
        n = 4 + rank
        so = np.array([0 if p <= root else n for p in range(world + 1)], dtype=np.uint64)       # everything goes to root
        ro = np.zeros(world + 1, dtype=np.uint64)
        if rank == root:
            ro[:] = np.concatenate([[0], np.cumsum([4 + q for q in range(world)])])
        send = np.arange(n, dtype=np.uint32) + 100 * rank
        recv = np.zeros(int(ro[-1]), dtype=np.uint32)
        sp = (C.c_void_p * 1)(send.ctypes.data)
        rp = (C.c_void_p * 1)(recv.ctypes.data if rank == root else None)
        es = (C.c_uint32 * 1)(4)
        rc = ep.ops.alltoallv_device(None, 1, sp, rp, es, so.ctypes.data_as(C.POINTER(C.c_uint64)), ro.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        return rc, recv
    got = run_threads(ThreadTransport(world), rank_body, timeout=90)
    assert [rc for rc, _ in got] == [0, 0, 0]
    assert got[root][1].tolist() == [100 * q + j for q in range(world) for j in range(4 + q)]


def test_an_exception_in_one_rank_fails_every_rank_quickly():
    """A Python exception inside rank 2's callback: that rank returns non-zero, and its peers — already waiting for it — return non-zero
    as well, long before the barrier's timeout."""
    world = 4
    tr = ThreadTransport(world)
    tr.endpoint(2).fail_next = RuntimeError("boom")

    def rank_body(rank, ep):
        mine = np.array([rank], dtype=np.uint64)
        everyone = np.zeros(world, dtype=np.uint64)
        first = ep.ops.allgather_host(None, mine.ctypes.data, everyone.ctypes.data, 8)
        a = np.ones(4, dtype=np.uint32)
        second = ep.ops.reduce_device(None, a.ctypes.data, 4, capi.U32, RED_SUM, -1, None)      # the barrier stays broken: no later collective hangs either
        return first, second
    t0 = time.monotonic()
    got = run_threads(tr, rank_body, timeout=90)
    assert time.monotonic() - t0 < 20
    assert all(first != 0 and second != 0 for first, second in got), got
    assert tr.errors[0] == (2, repr(RuntimeError("boom")))
    assert all(tr.endpoint(r).errors for r in range(world))


def test_run_threads_reraises_the_first_failure():
    tr = ThreadTransport(3)

    def rank_body(rank, ep):
        if rank == 1:
            raise KeyError("rank 1 went wrong")
        mine = np.array([rank], dtype=np.uint64)
        everyone = np.zeros(3, dtype=np.uint64)
        assert ep.ops.allgather_host(None, mine.ctypes.data, everyone.ctypes.data, 8) == 0, "a peer failed"
    with pytest.raises(KeyError):
        run_threads(tr, rank_body, timeout=90)
