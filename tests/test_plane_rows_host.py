"""The row sink of the aggregate on the bit-sliced planes, on the CPU (viyadb_amd/csrc/vh_bits_agg.h: vh_bits_row / vh_bits_row_bit /
vh_bits_row_field / vh_bits_row_gid; plain C++, compiled here by g++).

tests/plane_rows_host.cc is a stand-alone program. On random projections of 1 to 32 planes — fields at plane 0 and fields that end at plane
31, one to three group columns with lo > 0, rows with values below lo and at or beyond lo + extent, noise in the planes no field covers — it
checks that a row's record, its fields and its group id equal the row's own values and that the range verdict is false exactly for a row
outside the planned range; then that a host model of the sink (the compaction order of the kernel: slices of eight bits, lane by lane, bit
by bit; groups of 64; the record out of the source lane's words; one update per row and metric) fills the same table, bit for bit, as a host
model of the loop over group ids for G <= 64, across SUM32 (wrapping), SUM64 and MIN / MAX of I32 / U32 / I64 / U64, presence bytes and range
verdict included. It runs twice: plain, and with AddressSanitizer and UndefinedBehaviorSanitizer (plane words and queue are exact-size heap
blocks, so an access outside them is an error)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plane_rows_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_row_sink_equals_the_rows_and_the_loop_over_ids(tmp_path, sanitize):
    exe = str(tmp_path / "plane_rows_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
