#!/usr/bin/env python3
"""CPU ORACLE — TEST INFRASTRUCTURE ONLY.  Generates tests/golden/numcmp_golden.json from the reference's own
util/string.h (oracle/_ref/libviya_numcmp.so; run in the authoring container, where /root/reference exists).
The JSON holds string pairs and the four comparators' answers — data, no source.  tests/test_numcmp_golden.py holds
oracle/viya_oracle.py's _cmp_strings to it, and draws fresh pairs with random_pair() below where the library is built."""
import ctypes as C
import json
import os
import random
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
FNS = ("ref_greater_int", "ref_smaller_int", "ref_greater_float", "ref_smaller_float")


def load_library(path=None):
    lib = C.CDLL(path or os.path.join(HERE, "_ref", "libviya_numcmp.so"))
    for fn in FNS:
        getattr(lib, fn).restype = C.c_int
        getattr(lib, fn).argtypes = [C.c_char_p, C.c_char_p]
    return lib


def answers(lib, a, b):
    """The four comparators' answers (1 / 0; -1: std::stod threw)."""
    return [getattr(lib, fn)(a.encode(), b.encode()) for fn in FNS]


def fmt_double(x):
    return "%.15g" % x


def fmt_float(x):
    return "%g" % struct.unpack("<f", struct.pack("<f", x))[0]


def random_int_string(rnd):
    n = rnd.randrange(1, 21)
    s = str(rnd.randrange(10 ** (n - 1) if n > 1 else 0, 10 ** n))
    return ("-" if rnd.random() < 0.4 else "") + s


def random_float_string(rnd):
    """A normal double or float as the formatters print it (no NaN, no sub-normal text: see _about)."""
    if rnd.random() < 0.5:
        x = rnd.choice((-1, 1)) * rnd.uniform(1, 10) * 10.0 ** rnd.randrange(-300, 300)
        return fmt_double(x)
    x = rnd.choice((-1, 1)) * rnd.uniform(1, 10) * 10.0 ** rnd.randrange(-30, 30)
    return fmt_float(x)


def random_pair(rnd):
    """One fuzz pair: both integers or both floats; a third of the pairs are near each other."""
    if rnd.random() < 0.5:
        a = random_int_string(rnd)
        r = rnd.random()
        if r < 0.15:
            b = a
        elif r < 0.35:                      # same length, one digit changed
            i = rnd.randrange(len(a))
            b = a if a[i] == "-" else a[:i] + rnd.choice("0123456789" if i > (a[0] == "-") else "123456789") + a[i + 1:]
        else:
            b = random_int_string(rnd)
        return a, b
    a = random_float_string(rnd)
    r = rnd.random()
    if r < 0.15:
        b = a
    elif r < 0.35:                          # the same value through the other formatter, or its neighbour in the last digit
        b = fmt_float(float(a)) if rnd.random() < 0.5 and 1e-30 < abs(float(a)) < 1e30 else fmt_double(float(a) * (1 + rnd.choice((-1, 1)) * 1e-14))
    else:
        b = random_float_string(rnd)
    return a, b


def crafted_pairs():
    edge = {}                                # per length 1..20: smallest and largest magnitude, with and without '-'
    for n in range(1, 21):
        lo, hi = (10 ** (n - 1) if n > 1 else 0), 10 ** n - 1
        edge[n] = [str(lo), str(hi), "-" + str(lo), "-" + str(hi)]
    pairs = []
    for n in range(1, 21):                   # every length against itself and the next ("-9" vs "10": equal string lengths)
        for m in (n, n + 1):
            if m in edge:
                pairs += [(a, b) for a in edge[n] for b in edge[m]]
    core = ["0", "-0", "5", "-5", "3", "-10", "99", "-9", "10", "127", "-128", "255", "32767", "-32768", "65535", "2147483647", "-2147483648",
            "4294967295", "9223372036854775807", "-9223372036854775808", "18446744073709551615", "99999999999999999", "100000000000000000",
            "-99999999999999999", "-100000000000000000"]
    pairs += [(a, b) for a in core for b in core]
    for n in range(1, 21):                   # equal lengths differing in the first / the last digit, with and without '-'
        base = "4" * n
        for sign in ("", "-"):
            for other in ("5" + base[1:], "3" + base[1:], base[:-1] + "5", base[:-1] + "3"):
                pairs += [(sign + base, sign + other), (sign + other, sign + base), (sign + base, other), (base, sign + other)]
    floats = ["0", "-0", "1", "-1", "0.125", "-0.125", "1e+06", "999999", "1e+15", "1000.00000000001", "1000.00000000002", "1000",
              "-1000.00000000001", "0.001", "0.00100000000000001", "1e-05", "1.00000000000001e-05", "inf", "-inf", "1.79769313486231e+308",
              "-1.79769313486231e+308", "3.40282e+38", "-3.40282e+38", "2.2250738585072e-308", "1.17549e-38", "16777216", "1.67772e+07", "123457",
              "1.23457e+06", "-5", "3", "-10", "99", "9.00719925474099e+15"]
    # std::stod throws on DBL_MIN's text (below DBL_MIN) and on DBL_MAX's ("1.79769313486232e+308" rounds up past DBL_MAX): left out,
    # with the largest text of 15 digits that it reads in DBL_MAX's place (the caller drops any pair on which it throws, too)
    floats = [f for f in floats if f != "2.2250738585072e-308"]
    pairs += [(a, b) for a in floats for b in floats]
    return pairs


ABOUT = ("string pairs with the answers of the reference's src/util/string.h (util::StringNumCmp::GreaterInt, SmallerInt, GreaterFloat, "
         "SmallerFloat, in that order) compiled with g++ in the authoring container by oracle/build_oracle.py; generated by "
         "oracle/make_numcmp_golden.py. Left out: strings on which std::stod throws (DBL_MIN's \"%.15g\" text 2.2250738585072e-308 lies below DBL_MIN, DBL_MAX's text "
         "1.79769313486232e+308 above DBL_MAX, sub-normal text), and NaN, "
         "which std::stod reads but which makes the order non-strict (every comparison false). `fuzz` holds the first draws of "
         "random_pair(random.Random(1)).")

if __name__ == "__main__":
    lib = load_library()
    doc = {"_about": ABOUT, "order": [f[4:] for f in FNS], "pairs": [], "fuzz": []}
    seen = set()
    for a, b in crafted_pairs():
        if (a, b) in seen:
            continue
        seen.add((a, b))
        ans = answers(lib, a, b)
        if -1 in ans:
            print("left out (stod threw):", a, b)
            continue
        doc["pairs"].append([a, b] + [bool(x) for x in ans])
    rnd = random.Random(1)
    for _ in range(200):
        a, b = random_pair(rnd)
        ans = answers(lib, a, b)
        assert -1 not in ans, (a, b)
        doc["fuzz"].append([a, b] + [bool(x) for x in ans])
    out = os.path.join(os.path.dirname(HERE), "tests", "golden", "numcmp_golden.json")
    json.dump(doc, open(out, "w"), separators=(",", ":"))
    print(out, len(doc["pairs"]), "crafted pairs,", len(doc["fuzz"]), "fuzz pairs,", os.path.getsize(out), "bytes")
