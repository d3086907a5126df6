"""The wave scans by DPP (viyadb_amd/csrc/vh_wave_scan.h) on the GPU: the functions themselves in a stand-alone program
(tests/wave_scan_gpu.hip, built here), and what the compiled scan makes of them — one scan for both half pushes, the item -> tile step
through 64 slots of the wave's queue and a running maximum — on C3's plan over tables of at most 300 K rows. Every answer is compared with
the oracle over the host's current arrays and bit for bit with its twin under VH_PLAN_NO_GPLANES (the row-order planes: no tile groups, no
item -> tile step).

How a small table reaches the wave's tile groups: VH_TEST_UNIT_ROWS = the segment's capacity makes a segment ONE unit, so block s scans
segment s and its wave w the tiles w, w + 4, ... of it — with 65 536 rows a segment, groups of eight tiles. The test sets how many rows of
every tile hold d2 == 0: literal 0's run starts at place 0, so a tile with n such rows contributes ceil(n / 32) words, and the word
counts of a group's tiles are chosen per case (GROUPS below)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import JIT_OFF
from tests.test_gpu_gplanes import C3, D3_LT, D4_GE, EQ, HOT, ask, same_bits
from tests.test_gpu_layout_lifecycle import C3Host, D2
from viyadb_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, CAP, NSEG = 2048, 65536, 4          # 4 x 65 536 = 262 144 rows; 32 tiles a segment, 8 per wave

# words of literal 0's run in the eight tiles of a group (segment s, wave w), in the order the wave meets them
GROUPS = {
    (0, 0): [0, 0, 0, 0, 0, 0, 0, 0],         # total 0: no item, no batch
    (0, 1): [0, 0, 0, 1, 0, 0, 0, 0],         # total 1; tiles without words at the group's start and end
    (0, 2): [10, 0, 20, 0, 0, 30, 3, 0],      # total 63; tiles without words in the middle
    (0, 3): [0, 32, 0, 32, 0, 0, 0, 0],       # total 64: exactly one batch
    (1, 0): [64, 0, 0, 0, 0, 0, 0, 1],        # total 65: the second batch holds the last tile's one word
    (1, 1): [64, 0, 64, 0, 0, 0, 0, 0],       # total 128: two batches, one tile each (runs of the whole tile)
    (1, 2): [64, 5, 0, 0, 0, 0, 0, 0],        # a run that begins exactly on a batch boundary
    (1, 3): [40, 40, 0, 0, 0, 0, 0, 0],       # a run that straddles one
    (2, 0): [50, 64, 64, 3, 0, 0, 7, 0],      # runs that straddle two boundaries, then short ones
    (2, 1): [1, 1, 1, 1, 1, 1, 1, 1],         # eight marks in slots 0..7
    (2, 2): [0, 0, 0, 0, 0, 0, 0, 64],        # only the group's last tile
    (2, 3): [63, 1, 1, 63, 0, 64, 0, 0],      # a mark in slot 63, and one in slot 0 of the next batch
}                                              # (segment 3 keeps the generator's rows: ~16 words a tile, 128 a group)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from viyadb_amd import executor
    executor.init(0)


def _build_program(tmp_path, *defs):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / ("wave_scan_gpu" + "".join(d.replace("=", "_").replace("-D", "_") for d in defs))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *defs, os.path.join(ROOT, "tests", "wave_scan_gpu.hip"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    return exe


@pytest.mark.parametrize("defs", [(), ("-DVH_WAVE_SCAN_SHFL=1",)], ids=["dpp", "shfl"])
def test_scans_against_a_host_loop(tmp_path, defs):
    """One block of 256 threads; sums and running maxima of zeros, ones, the lane number, random 32-bit values that wrap, packed halves
    with 32 per lane, markers in 1, 2 and 64 slots, 64-bit sums that carry — and each scan once inside a wave-uniform branch."""
    run = subprocess.run([str(_build_program(tmp_path, *defs))], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "wave scan ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def _two_forms(h, leaves, seg_rows=None, label="", planes=True):
    c = ask(h, leaves, HOT, seg_rows, label + " clustered")
    if not JIT_OFF:
        assert c.jit and c.sliced and c.grouped_payload and c.grouped_planes == planes, (label, hex(c.flags), c.kernel)
    g = ask(h, leaves, HOT | capi.PLAN_NO_GPLANES, seg_rows, label + " row-order planes")
    assert not g.grouped_planes, (label, hex(g.flags))
    same_bits(c, g, f"{label}: clustered planes against the row-order planes")
    return c


def _set_run_words(h):
    """d2 == 0 in exactly 32 nw - r rows of every tile GROUPS names (r < 32 differs from tile to tile), every other 0 of the tile turned
    into 1. The rows are taken at random: d3 and d4 stay the generator's, about a fifth of a run passes."""
    rng = np.random.default_rng(11)
    for (s, w), words in GROUPS.items():
        d2 = h.tab.segments[s]["d"][D2]
        for step, nw in enumerate(words):
            tile = w + 4 * step
            sl = d2[tile * TILE:(tile + 1) * TILE]
            sl[sl == 0] = 1
            if nw:
                sl[rng.choice(TILE, size=32 * nw - (tile * 7) % 32, replace=False)] = 0
    for s in range(3):
        h.sync(s, 0, CAP)


@pytest.fixture(scope="module")
def grouped_host():
    h = C3Host(NSEG, CAP, CAP)
    _set_run_words(h)
    flags = h.dt.warm(h.plan(HOT))
    assert JIT_OFF or (flags & capi.INFO_GROUPED_PAYLOAD and flags & capi.INFO_GROUPED_PLANES), hex(flags)
    yield h
    h.close()


def test_word_totals_of_a_group(grouped_host, monkeypatch):
    """Groups of eight tiles with 0, 1, 63, 64, 65 and 128 words, tiles without words at a group's start, middle and end, runs that begin
    on a batch boundary and runs that straddle one (GROUPS). Literal 1's runs begin where 0's end — in the middle of a word — and literal
    3's end with the tile."""
    monkeypatch.setenv("VH_TEST_UNIT_ROWS", str(CAP))
    h = grouped_host
    zeros = sum(32 * nw - ((w + 4 * step) * 7) % 32 for (s, w), words in GROUPS.items() for step, nw in enumerate(words) if nw)
    assert sum(int(np.count_nonzero(h.tab.segments[s]["d"][D2] == 0)) for s in range(3)) == zeros
    for v in (0, 1, 3):
        assert _two_forms(h, [EQ(D2, v), D3_LT, D4_GE], label=f"eight-tile groups, d2 == {v}").passed_recs > 0
    # ... and the same tiles one to a wave and group (the planner's own units at this size)
    monkeypatch.delenv("VH_TEST_UNIT_ROWS")
    _two_forms(h, [EQ(D2, 0), D3_LT, D4_GE], label="one-tile groups, d2 == 0")


@pytest.mark.parametrize("snap, planes", [([5 * TILE, CAP, 0, 3 * TILE], True), ([CAP, CAP - 1000, TILE + 37, 0], False)])
def test_snapshots(grouped_host, monkeypatch, snap, planes):
    """Snapshots of whole tiles shorten the groups (the clustered scan); one that cuts a segment's last tile is answered by the row-order
    sliced loop over the grouped records, whose two pushes share their scan as well."""
    monkeypatch.setenv("VH_TEST_UNIT_ROWS", str(CAP))
    for v in (0, 1):
        _two_forms(grouped_host, [EQ(D2, v), D3_LT, D4_GE], seg_rows=snap, label=f"snapshot {snap}, d2 == {v}", planes=planes)


def test_segments_of_one_tile_and_a_segment_change(monkeypatch):
    """300 segments of 1 500 rows (one tile each) and one block per CU: the grid is smaller than the segments' number, so a wave that has
    queued the survivors of one segment's tile goes on to another segment's — every group is one tile, and it ends with a flush."""
    monkeypatch.setenv("VH_TEST_BLOCKS_PER_CU", "1")
    h = C3Host(300, 1500, TILE)
    try:
        h.dt.warm(h.plan(HOT))
        for v in (1, 0, 3):
            assert _two_forms(h, [EQ(D2, v), D3_LT, D4_GE], label=f"300 one-tile segments, d2 == {v}").passed_recs > 0
    finally:
        h.close()


def test_select_through_the_sliced_kernels():
    """select_scan_kernel, select_emit_sliced_kernel and the layout builder take their prefix sums from the same functions."""
    from tests import test_gpu_select_sliced as ss
    h = ss._host()
    try:
        passed = int(sum(ss.c3_mask(seg, ss.ROWS).sum() for seg in h.tab.segments))
        for skip, limit in ((0, 0), (17, 0), (5, 3), (passed // 2, 40), (passed - 1, 0), (passed + 5, 0)):
            info, _ = ss.check(h, ss.C3, ss.ALL, skip, limit, label="C3")
            assert info.passed_recs == passed
    finally:
        h.close()


JIT_OFF_CHILD = """
import sys
sys.path.insert(0, {root!r})
from viyadb_amd import executor, synth
from tests.parity import check_workload
executor.init(0)
w = synth.WORKLOADS["C3"](segment_rows=100_000)
res, _ = check_workload(w, nseg=3, rows_per_seg=100_000 - 37, flags=64)
assert not res.jit and res.path == "dense_part", (res.jit, res.path)
print("jit off ok", res.passed_recs)
"""


def test_the_plan_without_compiled_kernels(tmp_path):
    """VH_JIT=off is read once per process: a child runs C3 on the pre-built kernels (vh_part_tile_write's and vh_part_shares' scans)."""
    script = tmp_path / "jit_off.py"
    script.write_text(JIT_OFF_CHILD.format(root=ROOT))
    run = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=dict(os.environ, VH_JIT="off"))
    assert run.returncode == 0 and "jit off ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
