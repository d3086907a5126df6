"""Tile groups that span segments in the compiled clustered scan (viyadb_amd/csrc/vh_jit_body.h, VJ_GPSPAN; vh_grouped.h, vh_gspan_*): a
wave fills its group of up to 64 tiles whatever segments they lie in, queues table-wide record indexes and flushes its drain pipeline once.
C3's columns on three tables just above the sizes at which the form is sub-sorted (4 Mi rows) and the scan compiled (VH_JIT_MIN_ROWS):

  * 5 segments of 1 000 000 rows — every segment's last tile is partial (576 rows) and its last unit short;
  * 420 segments of 10 000 rows — five tiles a segment: a 64-tile group crosses a dozen segments, and many waves get no tile at all;
  * 3 segments of 2 097 152 rows — whole tiles, groups inside one segment.

On each, under VH_PLAN_FORCE_PART (DENSE_PART through the ring writer and the drain pipeline's last flush), the default organisation and
VH_PLAN_FORCE_HASH: C3's filter; a literal no value of d2's field equals; `d3 < 0`; `d3 < 1` (every run trimmed to its first word at the
most); `d3 < 1023`, the field's maximum (nothing trimmed); a snapshot that hides whole segments in the middle of a group. Every answer is
compared with the oracle (tests/parity.compare) and, bit for bit — keys, states, passed_recs, ngroups — with the same query under
VH_TEST_NO_GPSPAN=1, which must have run another code object; `gp_spanned` (vh_result_info.reserved bit 29) is set in the first leg and
clear in the second.

One of those filters has no spanning leg: `d2 == 7` never reaches a scan — the segments' recorded ranges rule it out (scanned_segments
is 0, an empty pre-built launch answers), and no literal inside a column's range lies outside its field. Its two legs are compared all
the same, and bit 29 must be clear with bit 21. Every test prepares the table for the flagship's plan first (VH_PLAN_FORCE_PART: the
projection, the bit-sliced planes and the sub-sorted form), so that each organisation finds the same layouts whatever ran before it; the
hash organisation is asked for with VH_PLAN_FORCE_JIT, without which a pre-built kernel answers it from the byte planes.

A snapshot that cuts a segment inside a tile keeps a plan off the clustered planes altogether (choose_grouped's rule, older than this
file: places have lost their row numbers), so that case has no spanning leg: it checks that bit 29 is clear with bit 21, and the answer."""
import numpy as np
import pytest

from oracle import viya_oracle as vo
from tests.conftest import JIT_OFF
from tests.parity import compare
from tests.test_gpu_gplanes import C3, D4_GE, EQ, REL, same_bits
from tests.test_gpu_layout_lifecycle import C3Host, D2, D3
from viyadb_amd import capi
from viyadb_amd.executor import AggPlan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(JIT_OFF, reason="the clustered planes are read by the compiled scan only")]
TILE = 2048
GEOMETRY = {"5x1000000": (5, 1_000_000), "420x10000": (420, 10_000), "3x2097152": (3, 2_097_152)}
ORGANISATION = {"part": capi.PLAN_FORCE_PART, "default": 0, "hash": capi.PLAN_FORCE_HASH | capi.PLAN_FORCE_JIT}
FIELD_MAX = 1023          # d3 holds 0 .. 999: a field of 10 bits
FILTERS = {
    "C3": C3,
    "no value of d2's field": [EQ(D2, 7), REL(D3, capi.OP_LT, "lt", 447), D4_GE],
    "d3 < 0": [EQ(D2, 1), REL(D3, capi.OP_LT, "lt", 0), D4_GE],
    "d3 < 1": [EQ(D2, 1), REL(D3, capi.OP_LT, "lt", 1), D4_GE],
    "d3 < the field's maximum": [EQ(D2, 1), REL(D3, capi.OP_LT, "lt", FIELD_MAX), D4_GE],
}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


@pytest.fixture(scope="module")
def hosts():
    """One table per geometry, built on first use and kept for the module; the oracle's answers are kept beside it (nothing changes a row)."""
    made = {}

    def get(name):
        if name not in made:
            nseg, rows = GEOMETRY[name]
            made[name] = (C3Host(nseg, rows, rows), {})
        return made[name]
    yield get
    for h, _ in made.values():
        h.close()


def hidden(name):
    """Whole segments hidden in the middle of what a wave would group: every third segment of the many, the middle ones of the few."""
    nseg, rows = GEOMETRY[name]
    if nseg == 420:
        return [0 if s % 3 == 1 or 200 <= s < 230 else rows for s in range(nseg)]
    return [rows if s in (0, nseg - 1) else 0 for s in range(nseg)]


def ask(h, wants, leaves, flags, seg_rows, label):
    filt = [l[0] for l in leaves] + [("and", len(leaves))]
    p = h.w.plan
    res = h.dt.query_agg(AggPlan(filter=filt, groups=p.groups, metrics=p.metrics, flags=flags, groups_hint=p.groups_hint, seg_rows=seg_rows))
    key = (tuple(l[0] for l in leaves), tuple(seg_rows) if seg_rows else None)
    if key not in wants:
        q = dict(h.w.query, filter={"op": "and", "filters": [l[1] for l in leaves]})
        wants[key] = vo.scan_aggregate(vo.parse_query(h.tab, q), seg_rows=seg_rows)
    compare(res, wants[key], f"{label} flags={flags:#x}")
    return res


def legs(h, wants, leaves, flags, seg_rows, label, monkeypatch, spans=True):
    monkeypatch.delenv("VH_TEST_NO_GPSPAN", raising=False)
    c = ask(h, wants, leaves, flags, seg_rows, label + ", spanning")
    print(f"{label}: {c.kernel} flags {c.flags:#x} passed {c.passed_recs} groups {c.ngroups} segments {c.scanned_segments}")
    if c.scanned_segments == 0:          # (ruled out by the segments' recorded ranges: no scan, compiled or other, read a row)
        assert c.passed_recs == 0 and c.ngroups == 0, label
        spans = False
    assert c.jit or not spans, (label, hex(c.flags), c.kernel)
    assert c.grouped_payload == spans and c.grouped_planes == spans, (label, hex(c.flags), c.kernel)
    assert c.gp_spanned == spans and bool(c.flags & capi.INFO_GPSPAN) == spans, (label, hex(c.flags), c.kernel)
    monkeypatch.setenv("VH_TEST_NO_GPSPAN", "1")
    u = ask(h, wants, leaves, flags, seg_rows, label + ", VH_TEST_NO_GPSPAN=1")
    monkeypatch.delenv("VH_TEST_NO_GPSPAN")
    assert u.jit == c.jit and u.grouped_planes == spans and not u.gp_spanned, (label, hex(u.flags), u.kernel)
    assert (c.kernel != u.kernel) == spans, (label, c.kernel, u.kernel)
    same_bits(c, u, label)
    assert c.ngroups == u.ngroups and c.passed_recs == u.passed_recs, label
    return c


def test_the_host_refuses_indexes_beyond_the_bound(hosts, monkeypatch):
    """VH_TEST_GPSPAN_BOUND lowers the 2^32 the record indexes and planes units must stay under to 420 x 2048: the 420-segment table, whose
    segments are 10 000 records apart at the least, exceeds it — the groups end with their segment again, and the answer is the same."""
    h, wants = hosts("420x10000")
    flags = capi.PLAN_FORCE_PART
    monkeypatch.delenv("VH_TEST_NO_GPSPAN", raising=False)
    h.dt.warm(h.plan(flags))
    c = ask(h, wants, C3, flags, None, "under 2^32")
    assert c.gp_spanned and c.grouped_planes and c.sub_trimmed, hex(c.flags)
    monkeypatch.setenv("VH_TEST_GPSPAN_BOUND", str(420 * TILE))
    r = ask(h, wants, C3, flags, None, "beyond the lowered bound")
    assert not r.gp_spanned and r.grouped_planes and r.sub_trimmed and r.kernel != c.kernel, (hex(r.flags), r.kernel)
    same_bits(c, r, "refused against spanning")
    monkeypatch.setenv("VH_TEST_GPSPAN_BOUND", str(1 << 40))          # (a bound above 2^32 is 2^32)
    assert ask(h, wants, C3, flags, None, "a bound above 2^32").kernel == c.kernel


@pytest.mark.parametrize("name", sorted(GEOMETRY))
@pytest.mark.parametrize("org", list(ORGANISATION))
def test_spanning_groups(hosts, name, org, monkeypatch):
    h, wants = hosts(name)
    nseg, rows = GEOMETRY[name]
    flags = ORGANISATION[org]
    monkeypatch.delenv("VH_TEST_NO_GPSPAN", raising=False)
    warmed = h.dt.warm(h.plan(capi.PLAN_FORCE_PART))
    paths = capi.INFO_GROUPED_PAYLOAD | capi.INFO_GROUPED_PLANES | capi.INFO_SUBTRIM | capi.INFO_GPSPAN
    assert warmed & paths == paths, hex(warmed)
    passed = {k: legs(h, wants, leaves, flags, None, f"{name} {org}: {k}", monkeypatch).passed_recs for k, leaves in FILTERS.items()}
    assert passed["C3"] > 0 and passed["no value of d2's field"] == 0 and passed["d3 < 0"] == 0 and passed["d3 < the field's maximum"] > passed["C3"], passed
    assert 0 < passed["d3 < 1"] < passed["C3"], passed
    # (what a snapshot leaves of these tables is fewer rows than a compile is thought worth: VH_PLAN_FORCE_JIT keeps the compiled scan)
    part = legs(h, wants, C3, flags | capi.PLAN_FORCE_JIT, hidden(name), f"{name} {org}: whole segments hidden", monkeypatch).passed_recs
    assert 0 < part < passed["C3"], (part, passed)
    cut = [rows] * nseg
    cut[nseg // 2] = 2 * TILE + 37
    legs(h, wants, C3, flags | capi.PLAN_FORCE_JIT, cut, f"{name} {org}: a segment cut inside a tile", monkeypatch, spans=False)
