"""The device top-N's sort key and slack (viyadb_amd/csrc/vh_topk_key.h, plain C++: compiled here by g++) against the reference's
order, as oracle.viya_oracle.fmt_num and _cmp_strings restate it (pinned by tests/test_numcmp_golden.py).

The contract is a superset: the device drops row b once key(b) < threshold - slack, the threshold being the key of the K-th best
row a. So, for all values a, b of a type and both directions:

    key(b) < key(a) - slack   =>   the reference ranks a STRICTLY better than b

(anything that ties with or beats a survives a threshold set at a). No tolerance: the property is exact. It is checked over every
pair of an adversarial list and over random pairs, a quarter of them within +-200 ulps / units of each other.

Left out, as in every sorted query of the suite: NaN (the reference's comparator is then no strict order), sub-normal doubles and
DBL_MAX (std::stod throws on their "%.15g" text, tests/test_numcmp_golden.py); the largest double whose text parses stands in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import viya_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TU = r"""
#include "vh_topk_key.h"
extern "C" void keys(int cls, int elem, const unsigned long long* bits, long n, unsigned long long* out) { for (long i = 0; i < n; ++i) out[i] = vh_topk_key(cls, elem, bits[i]); }
extern "C" unsigned long long slack(int cls, int elem) { return vh_topk_slack(cls, elem); }
"""
# enum vh_elem (include/viya_hip.h)
ELEM = {"ubyte": 0, "ushort": 1, "uint": 2, "ulong": 3, "byte": 4, "short": 5, "int": 6, "long": 7, "float": 8, "double": 9}
INT_TYPES = ["byte", "ubyte", "short", "ushort", "int", "uint", "long", "ulong"]
DBL_TEXT_MAX = float("1.79769313486231e+308")      # the largest "%.15g" text that std::stod reads


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("topk_key")
    src = d / "tk.cc"
    src.write_text(_TU)
    so = d / "libtk.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.keys.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    lib.keys.restype = None
    lib.slack.argtypes = [C.c_int, C.c_int]
    lib.slack.restype = C.c_uint64
    return lib


def _dtype(t):
    return np.dtype(vo.NUMERIC_TYPES[t][0])


def _cls(t):
    return 1 if t in ("float", "double") else 0


def device_keys(lib, t, vals):
    """vh_topk_key of each value, fed the way topk_keys_kernel feeds it: the element's bits, zero-extended."""
    vals = np.ascontiguousarray(vals, dtype=_dtype(t))
    bits = np.ascontiguousarray(vals.view("u%d" % vals.dtype.itemsize).astype(np.uint64))
    out = np.empty(len(bits), dtype=np.uint64)
    lib.keys(_cls(t), ELEM[t], bits.ctypes.data, len(bits), out.ctypes.data)
    return out


def reference_ranks(t, vals):
    """Dense rank of each value in the reference's ASCENDING order: equal rank = the comparator calls neither smaller. Uses the
    comparator's own definition once per value (stod of the text / (length, text)) instead of once per pair; _spot_check() holds
    that against _cmp_strings itself."""
    texts = [vo.fmt_num(v) for v in vals]
    ks = [vo._stod(s) for s in texts] if _cls(t) else [(len(s), s) for s in texts]
    order = {k: i for i, k in enumerate(sorted(set(ks)))}
    return np.array([order[k] for k in ks], dtype=np.int64), texts


def _spot_check(t, texts, ranks, pairs):
    kind = "float" if _cls(t) else "integer"
    lt, gt = vo._cmp_strings(kind, True), vo._cmp_strings(kind, False)
    for i, j in pairs:
        assert lt(texts[i], texts[j]) == (ranks[i] < ranks[j]) and gt(texts[i], texts[j]) == (ranks[i] > ranks[j]), (texts[i], texts[j])


def violations(keys_a, ranks_a, keys_b, ranks_b, slack, desc, pairwise):
    """(i, j) with b = j dropped by a threshold at a = i although the reference does not rank a strictly better. Mirrors
    topk_keys_kernel (ascending: ~key) and topk_compact_kernel (thr = T > slack ? T - slack : 0; keep key >= thr)."""
    ka, kb = (keys_a, keys_b) if desc else (~keys_a, ~keys_b)
    thr = np.where(ka > np.uint64(slack), ka - np.uint64(slack), np.uint64(0))
    if not pairwise:
        dropped = kb < thr
        better = ranks_a > ranks_b if desc else ranks_a < ranks_b
        return [(int(i), int(i)) for i in np.nonzero(dropped & ~better)[0]]
    bad = []
    step = max(1, (1 << 22) // max(1, len(kb)))
    for lo in range(0, len(ka), step):
        dropped = kb[None, :] < thr[lo:lo + step, None]
        ra = ranks_a[lo:lo + step, None]
        better = ra > ranks_b[None, :] if desc else ra < ranks_b[None, :]
        i, j = np.nonzero(dropped & ~better)
        bad += [(int(x) + lo, int(y)) for x, y in zip(i, j)]
    return bad


# ---------------------------------------------------------------------------------------------------------- adversarial values
def int_adversaries(t):
    info = np.iinfo(_dtype(t))
    vals = {0, info.min, info.max}
    d = 0
    while 10 ** d <= info.max:
        for m in (10 ** d, 10 ** (d + 1) - 1):
            for v in (m, -m):
                if info.min <= v <= info.max:
                    vals.add(v)
        d += 1
    if info.bits == 64:
        # the classes whose key drops the low 6 bits: runs of 130 neighbours at the class's start, inside it and at its end
        for nd in (18, 19, 20):
            lo, hi = 10 ** (nd - 1), min(10 ** nd - 1, info.max)
            if lo > info.max:
                continue
            for start in (lo, lo + (hi - lo) // 3 * 2 + 37, hi - 129):
                for v in range(start, start + 130):
                    vals.add(v)
                    if -v >= info.min:
                        vals.add(-v)
        if info.min < 0:
            vals.update(range(info.min, info.min + 130))
    return np.array(sorted(vals), dtype=object).astype(_dtype(t))


def same_text_run(x, dtype):
    """Every value of `dtype` that prints the text of x, in order, plus the first value on either side."""
    dtype = np.dtype(dtype)
    x = dtype.type(x)
    text = vo.fmt_num(x)
    lo = x
    while vo.fmt_num(np.nextafter(lo, dtype.type(-np.inf))) == text:
        lo = np.nextafter(lo, dtype.type(-np.inf))
    run = [np.nextafter(lo, dtype.type(-np.inf)), lo]
    while vo.fmt_num(run[-1]) == text:
        run.append(np.nextafter(run[-1], dtype.type(np.inf)))
    return np.array(run, dtype=dtype)          # run[1:-1] share the text


def run_width_ulps(run):
    u = run.view("u%d" % run.dtype.itemsize).astype(np.int64)
    return int(u[-2] - u[1])


def float_runs(t):
    dtype = _dtype(t)
    head = "1.00000000000001" if t == "double" else "1.00001"
    return [same_text_run(float("%se%d" % (head, e)), dtype) for e in range(-3, 16)]


def float_adversaries(t):
    dtype = _dtype(t)
    vals = [np.concatenate(float_runs(t))]
    if t == "float":
        one = np.float32(999999.5)
        near = [one]
        for _ in range(40):
            near = [np.nextafter(near[0], np.float32(-np.inf))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
        vals.append(np.array(near, dtype=dtype))          # "%g" switches from 999999 to 1e+06 here
        vals.append(np.array([2 ** 24 - 1, 2 ** 24, 2 ** 24 + 2, 2 ** 25, 2 ** 25 + 4, 2 ** 31, 2 ** 63, 3.0e38, np.finfo(np.float32).max,
                              np.finfo(np.float32).tiny, 1e-45], dtype=dtype))
    else:
        vals.append(np.array([DBL_TEXT_MAX, np.nextafter(DBL_TEXT_MAX, 0.0), 2.0 ** 53, 2.0 ** 53 + 2, 1e300, 1e-300, 2.2250738585073e-308], dtype=dtype))
    v = np.concatenate(vals)
    return np.concatenate([v, -v, np.array([0.0, -0.0, np.inf, -np.inf], dtype=dtype)])


def adversaries(t):
    return float_adversaries(t) if _cls(t) else int_adversaries(t)


def random_pairs(t, n, rng):
    """n pairs (a, b); a quarter of them within +-200 ulps (floats) / units (integers) of each other."""
    dtype = _dtype(t)
    near = rng.integers(-200, 201, n)
    near[n // 4:] = 0
    if _cls(t):
        u = "u%d" % dtype.itemsize
        bits = 8 * dtype.itemsize

        def draw(m):
            x = rng.integers(0, 1 << bits, m, dtype=np.uint64, endpoint=False).astype(u).view(dtype)
            ok = np.isfinite(x) & ((np.abs(x) >= np.finfo(dtype).tiny) | (x == 0))          # no NaN / inf here; no sub-normal (stod throws on a double's)
            if t == "double":
                ok &= np.abs(x) <= DBL_TEXT_MAX
            return np.where(ok, x, dtype.type(1.5))
        a, b = draw(n), draw(n)
        # a quarter: b = a moved by `near` ulps (staying finite and normal: `a` is re-drawn from mid-range magnitudes)
        mid = (rng.uniform(1, 10, n // 4) * 10.0 ** rng.integers(-30, 31, n // 4) * rng.choice([-1, 1], n // 4)).astype(dtype)
        a[:n // 4] = mid
        ai = a[:n // 4].view("i%d" % dtype.itemsize)
        b[:n // 4] = (ai + near[:n // 4].astype(ai.dtype)).view(dtype)          # the sign bit stays: bit patterns are monotone in |x|, one step = one ulp
        return a, b
    info = np.iinfo(dtype)
    import random
    rnd = random.Random(int(rng.integers(1 << 30)))
    # magnitudes spread over every digit class, not uniform over the range (which would almost only draw the longest class)
    digits = rng.integers(1, len(str(info.max)) + 1, 2 * n)
    mags = [rnd.randrange(10 ** int(d)) for d in digits]
    sign = rng.choice([-1, 1], 2 * n) if info.min < 0 else np.ones(2 * n, dtype=np.int64)
    v = [min(max(int(s) * m, info.min), info.max) for s, m in zip(sign, mags)]
    a, b = v[:n], v[n:]
    for i in range(n // 4):
        b[i] = min(max(a[i] + int(near[i]), info.min), info.max)
    return np.array(a, dtype=object).astype(dtype), np.array(b, dtype=object).astype(dtype)


# --------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("t", INT_TYPES + ["float", "double"])
def test_superset_property_on_adversarial_pairs(lib, t, desc):
    vals = adversaries(t)
    keys = device_keys(lib, t, vals)
    ranks, texts = reference_ranks(t, vals)
    rng = np.random.default_rng(5)
    _spot_check(t, texts, ranks, rng.integers(0, len(vals), (3000, 2)))
    bad = violations(keys, ranks, keys, ranks, lib.slack(_cls(t), ELEM[t]), desc, pairwise=True)
    assert not bad, "%d of %d pairs; first: threshold at %r drops %r (keys %#x, %#x; slack %d)" % (
        len(bad), len(vals) ** 2, texts[bad[0][0]], texts[bad[0][1]], keys[bad[0][0]], keys[bad[0][1]], lib.slack(_cls(t), ELEM[t]))


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("t", INT_TYPES + ["float", "double"])
def test_superset_property_on_random_pairs(lib, t, desc):
    n = 100_000
    a, b = random_pairs(t, n, np.random.default_rng(ELEM[t] * 2 + desc))
    ranks, texts = reference_ranks(t, np.concatenate([a, b]))
    _spot_check(t, texts, ranks, [(i, i + n) for i in range(0, n, 37)])
    bad = violations(device_keys(lib, t, a), ranks[:n], device_keys(lib, t, b), ranks[n:], lib.slack(_cls(t), ELEM[t]), desc, pairwise=False)
    assert not bad, "%d of %d pairs; first: threshold at %r drops %r" % (len(bad), n, texts[bad[0][0]], texts[bad[0][0] + n])


def test_integer_keys_order_exactly_up_to_17_digits(lib):
    """Below the lossy classes the key is not only monotone but strict: different values, different keys (so integer top-N keeps no
    row it does not have to), and no slack is applied to integers at all."""
    for t in INT_TYPES:
        assert lib.slack(0, ELEM[t]) == 0
        vals = adversaries(t)
        vals = vals[np.abs(vals.astype(object)) < 10 ** 17] if _dtype(t).itemsize == 8 else vals
        keys = device_keys(lib, t, vals)
        ranks, _ = reference_ranks(t, vals)
        o = np.argsort(ranks, kind="stable")
        assert np.all(np.diff(keys[o].astype(object)) > 0), t


@pytest.mark.parametrize("t,bound", [("double", 2 * 2.0 ** 52 / 1e14), ("float", 2 * 2.0 ** 23 / 1e5)])
def test_slack_covers_the_formatter(lib, t, bound):
    """From formatting alone: the widest run of values that print one text (so tie in the reference) is narrower than the slack, in
    ulps, and within the bound the slack is derived from (vh_topk_key.h). A change of formatter or slack trips this."""
    widths = [run_width_ulps(r) for r in float_runs(t)]
    slack = lib.slack(1, ELEM[t]) >> (32 if t == "float" else 0)
    print(t, "widest run of one text:", max(widths), "ulps; bound %.2f; slack %d" % (bound, slack))
    assert max(widths) <= bound < slack
    assert max(widths) == (87 if t == "double" else 163)          # the figures vh_topk_key.h quotes
