"""The oracle's time truncation and rollup chain, and viyadb_amd/csrc/vh_time.h compiled for the host, on the edge values of
tests/time_edges.py: against a datetime-based truncation, against outputs of the reference's own util/time.cc from 2^32 seconds on
(tests/golden/time_golden_wide.json), and against a restatement of the rule chain. The tables tests/test_gpu_time_edges.py mirrors into
device memory are checked for what those tests rely on."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests import time_edges as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = json.load(open(os.path.join(ROOT, "tests", "golden", "time_golden_wide.json")))
VHT = {"year": 0, "month": 1, "day": 3, "hour": 4, "minute": 5, "second": 6}          # enum vh_time_unit


def test_value_sets_hold_what_they_promise():
    e, w = te.EDGE_SECS, te.WIDE_SECS
    assert e == sorted(set(e)) and w == sorted(set(w)) and e[0] == 0 and e[-1] == te.U32_MAX and w[0] == 1 << 32 and w[-1] == te.LAST_SECOND
    for v in (1, 59, 60, 3599, 3600, 86399, 86400, (1 << 31) - 1, 1 << 31,
              951782400, 951868799,                     # 2000-02-29 00:00:00 and 23:59:59: the leap day of a century
              4107456000 + 86400 - 1, 4107542400,       # 2100-02-28 23:59:59 -> 2100-03-01 00:00:00: no leap day in between
              1451606399, 1451606400):                  # 2015-12-31 23:59:59 -> 2016-01-01
        assert v in e, v
    assert te.truth(4107542400, "month") == 4107542400 and te.truth(4107542399, "month") == 4107542400 - 28 * 86400
    assert 13574563200 in w and te.truth(13574563200, "day") == 13574563200 and te.truth(13574563200, "month") == 13574563200 - 28 * 86400      # 2400-02-29
    assert WIDE["secs"] == w and WIDE["micros"] == [0, 999999]


@pytest.mark.parametrize("unit", te.UNITS)
def test_oracle_truncation_equals_datetime(unit):
    u = te.UNIT_CODE[unit]
    for s in te.EDGE_SECS:
        assert vo.rollup_ts(s, False, [], u) == te.truth(s, unit), (unit, s)
    for s in te.EDGE_SECS + te.WIDE_SECS:
        for us in te.MICRO_OFFSETS:
            assert vo.rollup_ts(s * 1000000 + us, True, [], u) == te.truth(s, unit) * 1000000, (unit, s, us)      # (the microseconds go, under SECOND too)


def test_microseconds_survive_only_without_truncation():
    """Time64::trunc zeroes the microseconds whatever the unit — SECOND included; no rule and no granularity keeps them."""
    for s in (0, te.U32_MAX, 1 << 32, te.LAST_SECOND):
        for us in (1, 999999):
            v = s * 1000000 + us
            assert vo.rollup_ts(v, True, [], None) == v
            assert vo.rollup_ts(v, True, [], vo.SECOND) == s * 1000000
            assert vo.rollup_ts(v, True, [(vo.SECOND, v + 1)], None) == s * 1000000 and vo.rollup_ts(v, True, [(vo.SECOND, v)], None) == v


@pytest.mark.parametrize("unit", te.UNITS)
def test_oracle_equals_the_reference_from_2_32_on(unit):
    u = te.UNIT_CODE[unit]
    assert WIDE["units"][unit] == VHT[unit]
    for s, outs in zip(WIDE["secs"], WIDE["trunc64"][unit]):
        for us, want in zip(WIDE["micros"], outs):
            assert vo.rollup_ts(s * 1000000 + us, True, [], u) == want, (unit, s, us)
            assert te.truth(s, unit) * 1000000 == want, (unit, s, us)


_TU = r"""
#include "vh_time.h"
extern "C" unsigned int t32(unsigned int t, int u) { return vh_trunc_secs32(t, u); }
extern "C" unsigned long long t64(unsigned long long t, int u) { return vh_trunc_secs64(t, u); }
extern "C" unsigned long long tany(unsigned long long t, int u) { return vh_trunc_secs(t, u); }
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    d = tmp_path_factory.mktemp("vh_time")
    src, so = d / "tt.cc", d / "libtt.so"
    src.write_text(_TU)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.t32.restype = C.c_uint32; lib.t32.argtypes = [C.c_uint32, C.c_int]
    lib.t64.restype = C.c_uint64; lib.t64.argtypes = [C.c_uint64, C.c_int]
    lib.tany.restype = C.c_uint64; lib.tany.argtypes = [C.c_uint64, C.c_int]
    return lib


@pytest.mark.parametrize("unit", te.UNITS)
def test_device_header_on_the_host_equals_datetime(header, unit):
    """vh_trunc_secs, vh_trunc_secs32 and vh_trunc_secs64 (what the kernels truncate with) on every edge value; the 32-bit form where the
    value fits."""
    u = VHT[unit]
    for s in te.EDGE_SECS + te.WIDE_SECS:
        want = te.truth(s, unit)
        assert header.tany(s, u) == want, ("vh_trunc_secs", unit, s)
        assert header.t64(s, u) == want, ("vh_trunc_secs64", unit, s)
        if s <= te.U32_MAX:
            assert header.t32(s, u) == want, ("vh_trunc_secs32", unit, s)
    for s, outs in zip(WIDE["secs"], WIDE["trunc64"][unit]):
        assert header.tany(s, u) * 1000000 == outs[0] == header.t64(s, u) * 1000000, (unit, s)


def _rules_of(tab):
    d = tab.column("ts")
    return d, vo.rollup_boundaries(d, te.NOW)


@pytest.mark.parametrize("kind", ["time", "microtime"])
@pytest.mark.parametrize("name", sorted(te.RULE_SETS))
def test_rule_chain_equals_its_restatement(name, kind):
    tab = te.boundary_table(kind, te.RULE_SETS[name])
    d, bounds = _rules_of(tab)
    micro = kind == "microtime"
    by_name = te.named_rules(d)
    by_code = [(r.granularity, b) for r, b in zip(d.rollup_rules, bounds)]
    seen = set()
    for v in te.table_values(tab):
        for unit in (None, "hour", "day", "month"):
            got = vo.rollup_ts(v, micro, by_code, None if unit is None else te.UNIT_CODE[unit])
            assert got == te.rule_chain(v, micro, by_name, unit), (name, kind, v, unit)
        seen.add(next((k for k, (_, b) in enumerate(by_name) if v < b), len(by_name)))
    assert seen == set(range(len(by_name) + 1)), "every rule, and no rule at all, is some value's first match"
    if name == "first_match":      # a value older than both boundaries: the first rule in the reference's order wins, not the last that matches
        old = min(te.table_values(tab))
        assert all(old < b for _, b in by_name)
        assert vo.rollup_ts(old, micro, by_code, None) == te.rule_chain(old, micro, by_name[:1], None) != te.rule_chain(old, micro, by_name[1:], None)


@pytest.mark.parametrize("kind", ["time", "microtime"])
@pytest.mark.parametrize("name", sorted(te.RULE_SETS))
def test_boundary_tables_hold_every_neighbour(name, kind):
    tab = te.boundary_table(kind, te.RULE_SETS[name])
    _, bounds = _rules_of(tab)
    held = set(te.table_values(tab))
    assert len(set(bounds)) == len(te.RULE_SETS[name])
    for b in bounds:
        for v in te.boundary_neighbours(b, kind == "microtime"):
            assert v in held, (name, kind, b, v)
    assert min(held) < min(bounds) - 1 and max(held) > max(bounds) + 1
    inner = [v for v in held if min(bounds) < v < max(bounds)]
    assert len(inner) > 20
    narrow = tab.segments[2]["d"][0]
    assert int(narrow.min()) < bounds[0] <= int(narrow.max())       # the first rule switches inside the narrow segment


@pytest.mark.parametrize("kind", ["time", "microtime", "both"])
def test_edge_tables_are_what_the_gpu_tests_assume(kind):
    tab = te.edge_table(kind)
    assert [s["size"] for s in tab.segments] == list(te.SEG_ROWS) and te.SEG_ROWS[0] % 1024 == 0 and te.SEG_ROWS[3] % 1024 != 0 and te.SEG_ROWS[3] > 1025
    for name in (["ts"] if kind != "both" else ["ts", "uts"]):
        c = tab.column(name)
        micro = c.micro
        scale = 1000000 if micro else 1
        want = set(te.values_of("microtime" if micro else "time"))
        seg = [s["d"][c.index][:s["size"]] for s in tab.segments]
        assert {int(v) for v in seg[0]} == want and {int(v) for v in seg[3]} == want                 # both cycling segments hold the whole set
        assert len(np.unique(seg[1])) == 1 and int(seg[1][0]) == (((1 << 32) * 1000000) if micro else te.U32_MAX)
        span = (int(seg[2].max()) - int(seg[2].min())) // scale
        assert span == 120 < 256 and len(np.unique(seg[2] // np.uint64(scale) if micro else seg[2])) == 121
        assert te.truth(int(seg[2].min()) // scale, "month") != te.truth(int(seg[2].max()) // scale, "month")      # a month ends inside it
        if micro:
            assert max(want) > (1 << 32) * 1000000 and sum(v > (1 << 32) * 1000000 for v in want) >= 3 * len(te.WIDE_SECS) - 1
        # every value meets several groups of k
        k = tab.segments[0]["d"][tab.column("k").index][:te.SEG_ROWS[0]]
        pairs = {}
        for v, g in zip(seg[0].tolist(), k.tolist()):
            pairs.setdefault(v, set()).add(g)
        assert min(len(s) for s in pairs.values()) >= 2
    ids = np.concatenate([s["d"][tab.column("id").index][:s["size"]] for s in tab.segments])
    frac = float((ids < 40).mean())
    assert 0.02 < frac < 0.06                                                                        # the filter of the packed-form tests
