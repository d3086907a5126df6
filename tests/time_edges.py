"""Time values at calendar and width edges, and small tables that hold them.

The typed tables of the other tests draw their timestamps from the two or three years before one NOW. This module puts a time column
where truncation can go wrong instead:

  EDGE_SECS  seconds that fit 32 bits: 0, 1, the ends of the first minute / hour / day, 2^31 - 1, 2^31, 2^32 - 1, and for the years
             1970 .. 2106 listed in YEARS32 (leap, non-leap, the century 2000 that is leap and the century 2100 that is not, the 2^31 second's
             year 2038, the last 32-bit year 2106) the first second of every month +- 1 s and February 28th, 29th (where it exists) and
             March 1st at 00:00:00, 12:00:00 and 23:59:59;
  WIDE_SECS  seconds from 2^32 on: 2^32, 2^32 + 86399, 9999-12-31 23:59:59 and the same month / February points for 2106, 2107, 2400 (a
             leap century) and 9999.

truth() truncates with datetime alone: it shares nothing with oracle/viya_oracle.py or viyadb_amd/csrc/vh_time.h.

edge_table(kind) lays the values out like tests/extremes.py lays out its numbers:
  segment 0  cycles the whole set;
  segment 1  one value only (2^32 - 1 for `time`, 2^32 s in microseconds for `microtime`);
  segment 2  every second from 2100-02-28 23:59:00 to 2100-03-01 00:01:00: 121 values around a month end that is NOT a leap day (a
             projection stores a column at the bits of the TABLE's largest value, so narrow_table() holds this run alone);
  segment 3  cycles again with another stride and a row count that is no multiple of 1024.
boundary_table(kind, rules, now) is the same shape with the values chosen around the rollup rules' boundaries.
"""
from __future__ import annotations

import calendar
import datetime
from math import gcd

import numpy as np

from oracle import viya_oracle as vo

UNITS = ["year", "month", "day", "hour", "minute", "second"]
UNIT_CODE = {"year": vo.YEAR, "month": vo.MONTH, "day": vo.DAY, "hour": vo.HOUR, "minute": vo.MINUTE, "second": vo.SECOND}
UNIT_NAME = {code: name for name, code in UNIT_CODE.items()}
YEARS32 = (1970, 1971, 1972, 1999, 2000, 2001, 2016, 2037, 2038, 2099, 2100, 2101, 2105, 2106)
YEARS_WIDE = (2106, 2107, 2400, 9999)
U32_MAX = (1 << 32) - 1
LAST_SECOND = 253402300799                       # 9999-12-31 23:59:59
MICRO_OFFSETS = (0, 1, 999999)
NARROW_FIRST = calendar.timegm((2100, 2, 28, 23, 59, 0))
NARROW_LAST = calendar.timegm((2100, 3, 1, 0, 1, 0))
SEG_SIZE = 6144
SEG_ROWS = (5120, 4096, 4096, 4453)              # segment 3: four full 1024-row steps and a ragged tail of 357
ID_MOD = 1009


def _is_leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def year_points(y: int):
    """The first second of every month +- 1 s; February 28th, 29th where it exists and March 1st at 00:00:00, 12:00:00, 23:59:59."""
    out = []
    for m in range(1, 13):
        t = calendar.timegm((y, m, 1, 0, 0, 0))
        out += [t - 1, t, t + 1]
    days = [(2, 28), (3, 1)] + ([(2, 29)] if _is_leap(y) else [])
    for m, d in days:
        for hh, mm, ss in ((0, 0, 0), (12, 0, 0), (23, 59, 59)):
            out.append(calendar.timegm((y, m, d, hh, mm, ss)))
    return out


def _edge_secs():
    vals = {0, 1, 59, 60, 3599, 3600, 86399, 86400, (1 << 31) - 1, 1 << 31, U32_MAX}
    for y in YEARS32:
        vals |= set(year_points(y))
    return sorted(v for v in vals if 0 <= v <= U32_MAX)


def _wide_secs():
    vals = {1 << 32, (1 << 32) + 86399, LAST_SECOND}
    for y in YEARS_WIDE:
        vals |= set(year_points(y))
    return sorted(v for v in vals if U32_MAX < v <= LAST_SECOND)


EDGE_SECS = _edge_secs()
WIDE_SECS = _wide_secs()
_EPOCH = datetime.datetime(1970, 1, 1)


def truth(secs: int, unit: str) -> int:
    """`secs` truncated to `unit` by datetime's own calendar (proleptic Gregorian, no leap seconds: what gmtime / timegm do)."""
    t = _EPOCH + datetime.timedelta(seconds=int(secs))
    keep = {"year": 1, "month": 2, "day": 3, "hour": 4, "minute": 5, "second": 6}[unit]
    f = [t.year, t.month, t.day, t.hour, t.minute, t.second]
    f = f[:keep] + [1, 1, 1, 0, 0, 0][keep:]
    d = datetime.datetime(*f) - _EPOCH
    return d.days * 86400 + d.seconds


def truth_value(v: int, micro: bool, unit) -> int:
    """A stored value (seconds, or microseconds when `micro`) truncated to `unit`; None keeps it whole."""
    if unit is None:
        return int(v)
    return truth(v // 1000000, unit) * 1000000 if micro else truth(v, unit)


def values_of(kind: str):
    """The distinct stored values of edge_table(kind)'s cycling segments, as Python ints."""
    if kind == "time":
        return list(EDGE_SECS)
    return [s * 1000000 + o for s in EDGE_SECS + WIDE_SECS for o in MICRO_OFFSETS]


def _np(kind: str, vals):
    return np.array([int(v) for v in vals], dtype=object).astype(np.uint32 if kind == "time" else np.uint64)


def _coprime(n: int, start: int) -> int:
    k = start
    while gcd(k, n) != 1:
        k += 1
    return k


def _cycle(arr: np.ndarray, rows: int, stride: int, offset: int = 0) -> np.ndarray:
    return arr[(np.arange(rows, dtype=np.int64) * stride + offset) % len(arr)]


def _time_dim(name: str, kind: str, rules=None):
    d = {"name": name, "type": kind}
    if rules:
        d["rollup_rules"] = rules
    return d


def _schema(time_dims):
    return {"name": "t", "segment_size": SEG_SIZE,
            "dimensions": time_dims + [{"name": "k", "type": "uint"}, {"name": "id", "type": "uint"}],
            "metrics": [{"name": "count", "type": "count"}, {"name": "long_sum", "type": "long_sum"}]}


def _fill(tab: vo.Table, columns):
    """columns: per time dimension (whole set, the one value of segment 1, the narrow run of segment 2). Four segments; `k` cycles with a
    period coprime to the number of values, so that a value's repeats land in different groups; `id` spreads over [0, ID_MOD)."""
    nval = len(columns[0][0])
    nk = _coprime(nval, 7)
    base = 0
    for seg, rows in enumerate(SEG_ROWS):
        g = np.arange(base, base + rows, dtype=np.int64)
        d = []
        for j, (whole, one, narrow) in enumerate(columns):
            if seg == 0:
                d.append(_cycle(whole, rows, _coprime(len(whole), 1 + 2 * j)))
            elif seg == 1:
                d.append(np.full(rows, one, dtype=whole.dtype))
            elif seg == 2:
                d.append(_cycle(narrow, rows, _coprime(len(narrow), 1 + 4 * j)))
            else:
                d.append(_cycle(whole, rows, _coprime(len(whole), 37 + 6 * j), 11))
        d.append((np.arange(rows) % nk).astype(np.uint32))
        d.append(((g * 7919) % ID_MOD).astype(np.uint32))
        m = [(1 + g % 3).astype(np.uint32), ((g * 37) % 2001 - 1000).astype(np.int64)]
        tab.add_segment_arrays(d, m, None, rows)
        base += rows
    return tab


def _edge_columns(kind: str):
    whole = _np(kind, values_of(kind))
    secs = range(NARROW_FIRST, NARROW_LAST + 1)
    if kind == "time":
        return whole, U32_MAX, _np(kind, secs)
    return whole, (1 << 32) * 1000000, _np(kind, [s * 1000000 + MICRO_OFFSETS[i % 3] for i, s in enumerate(secs)])


def edge_table(kind: str) -> vo.Table:
    """kind: "time" (uint32 seconds, EDGE_SECS), "microtime" (uint64 microseconds, EDGE_SECS + WIDE_SECS at three offsets), or "both": a
    `time` dimension ts AND a `microtime` dimension uts, cycling with different strides."""
    if kind == "both":
        return _fill(vo.Table(_schema([_time_dim("ts", "time"), _time_dim("uts", "microtime")])), [_edge_columns("time"), _edge_columns("microtime")])
    return _fill(vo.Table(_schema([_time_dim("ts", kind)])), [_edge_columns(kind)])


def narrow_table(kind: str) -> vo.Table:
    """Segment 2 of edge_table alone, twice (4096 and 1500 rows): every time value of the TABLE lies within two minutes, so a projection
    stores the column at the fewest bits its values allow and one synced row can outgrow them."""
    _, _, narrow = _edge_columns(kind)
    tab = vo.Table(_schema([_time_dim("ts", kind)]))
    base = 0
    for rows in (4096, 1500):
        g = np.arange(base, base + rows, dtype=np.int64)
        tab.add_segment_arrays([_cycle(narrow, rows, 1, base), (g % 5).astype(np.uint32), ((g * 7919) % ID_MOD).astype(np.uint32)],
                               [(1 + g % 3).astype(np.uint32), ((g * 37) % 2001).astype(np.int64)], None, rows)
        base += rows
    return tab


def table_values(tab: vo.Table, col: str = "ts", seg_rows=None):
    """Distinct stored values of a dimension over the table's (snapshot) rows, as Python ints."""
    c = tab.column(col)
    parts = [seg["d"][c.index][:seg["size"] if seg_rows is None else int(seg_rows[i])] for i, seg in enumerate(tab.segments)]
    return [int(v) for v in np.unique(np.concatenate(parts))]


# ------------------------------------------------------------------------------------------------------------------------------------
# rollup rules
# ------------------------------------------------------------------------------------------------------------------------------------
NOW = 1496570140
RULES_NESTED = [{"granularity": "hour", "after": "1 days"}, {"granularity": "day", "after": "1 weeks"}, {"granularity": "month", "after": "1 years"}]
# the first matching rule is not the last matching one: a value older than a month is older than an hour too, and `year` must win
RULES_FIRST_MATCH = [{"granularity": "minute", "after": "1 hours"}, {"granularity": "year", "after": "1 months"}]
RULE_SETS = {"nested": RULES_NESTED, "first_match": RULES_FIRST_MATCH}


def boundary_neighbours(b: int, micro: bool):
    """The values a boundary must have around it in a table: b - 1, b, b + 1 (for microseconds: +- 1 us and +- 1 s)."""
    return [b - 1000000, b - 1, b, b + 1, b + 1000000] if micro else [b - 1, b, b + 1]


def boundary_values(kind: str, boundaries, now: int):
    micro = kind == "microtime"
    scale = 1000000 if micro else 1
    lo_s, hi_s = min(boundaries) // scale, now
    vals = set()
    for b in boundaries:
        vals |= set(boundary_neighbours(b, micro))
        bs = b // scale
        for u in UNITS:                                     # the unit edges next to every boundary: the last second a rule still truncates away
            e = truth(bs, u)
            vals |= {v * scale for v in (e - 1, e, e + 1)}
    vals.add((lo_s - 5 * 366 * 86400 - 12345) * scale)      # older than every boundary
    vals.add((hi_s + 3601) * scale + (7 if micro else 0))   # newer than every boundary
    y0, y1 = (_EPOCH + datetime.timedelta(seconds=lo_s)).year - 1, (_EPOCH + datetime.timedelta(seconds=hi_s)).year + 1
    for y in range(max(1970, y0), y1 + 1):                  # the calendar edges between the boundaries
        for s in year_points(y):
            if lo_s - 400 * 86400 <= s <= hi_s + 86400:
                vals |= {s * scale + o for o in (MICRO_OFFSETS if micro else (0,))}
    top = (1 << 64) - 1 if micro else U32_MAX
    return sorted(v for v in vals if 0 <= v <= top)


def named_rules(d: vo.Column, now: int = NOW):
    """[(unit name, boundary)] of a time dimension's rollup rules, in the reference's order (the longest `after` first)."""
    return [(UNIT_NAME[r.granularity], b) for r, b in zip(d.rollup_rules, vo.rollup_boundaries(d, now))]


def boundary_table(kind: str, rules, now: int = NOW) -> vo.Table:
    """edge_table's shape with the values chosen after the boundaries are known: every boundary with its neighbours, a value older and a value
    newer than all, the calendar edges between them. Segment 1 holds the first rule's boundary alone; segment 2 every second (microtime: at
    cycling offsets) of the two minutes around it, so the rule switches inside a segment that packs into a few bits."""
    tab = vo.Table(_schema([_time_dim("ts", kind, rules)]))
    d = tab.column("ts")
    bounds = vo.rollup_boundaries(d, now)
    micro = kind == "microtime"
    scale = 1000000 if micro else 1
    whole = _np(kind, boundary_values(kind, bounds, now))
    b0 = bounds[0]
    run = range(b0 // scale - 60, b0 // scale + 61)
    narrow = _np(kind, [s * scale + (MICRO_OFFSETS[i % 3] if micro else 0) for i, s in enumerate(run)])
    return _fill(tab, [(whole, b0, narrow)])


def rule_chain(v: int, micro: bool, rules, unit):
    """The rollup chain restated from scratch: the first rule whose boundary lies beyond the stored value truncates; then the query's
    granularity truncates. rules: [(unit name, boundary)]; unit: a unit name or None."""
    secs, rest = (v // 1000000, v % 1000000) if micro else (v, 0)
    for u, before in rules:
        if v < before:
            secs, rest = truth(secs, u), 0
            break
    if unit is not None:
        secs, rest = truth(secs, unit), 0
    return secs * 1000000 + rest if micro else secs
