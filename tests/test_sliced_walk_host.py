"""How the readers of the bit-sliced predicate planes share the rows out (viyadb_amd/csrc/vh_sliced_walk.h: VhChunkWalk and
vh_sliced_tail_mask; plain C++, compiled here by g++), run on the CPU as the select kernels and scan_agg_sliced_kernel run them.

tests/sliced_walk_host.cc is a stand-alone program. For every combination of 1, 3 and 7 segments, 1, 3 and 4 chunks per segment, grids of
1, 2, 5, 304 and more blocks than there are chunks, 4 and 16 waves per block, and snapshots drawn from {0, 1, 31, 32, 33, 2047, 2048, 2049,
5000, capacity} it asserts that every row below seg_rows of every segment is covered by exactly one (block, wave, lane, bit), that no word
beginning at or beyond seg_rows is asked for, and that chunk() is the index the select kernels' counts[] expect. It runs twice: plain, and
with AddressSanitizer and UndefinedBehaviorSanitizer (the coverage arrays are exact-size heap blocks)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sliced_walk_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_row_is_covered_once_and_no_word_beyond_the_snapshot_is_read(tmp_path, sanitize):
    exe = str(tmp_path / "sliced_walk_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
