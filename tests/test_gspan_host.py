"""Tile groups that span segments, on the CPU: the 32-bit record index and planes unit the spanning scan keeps per tile
(viyadb_amd/csrc/vh_grouped.h, vh_gspan_*) against the per-segment byte offsets, built plain and under AddressSanitizer and UBSan.
No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_spanning_index_equals_the_per_segment_address(tmp_path, flags):
    """tests/gspan_host.cc walks every (segment, tile, place) and (segment, tile, word) of the three geometries tests/test_gpu_gpspan.py
    scans — 5 x 1 000 000 rows, 420 x 10 000, 3 x 2 097 152 — at word groups of 4, 12 and 20 dwords and padded strides, and checks the
    host's condition: strides that do not divide, a bound met exactly and missed by one, 2^32 itself."""
    exe = tmp_path / "gspan_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "viyadb_amd", "csrc"),
                    os.path.join(ROOT, "tests", "gspan_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 4 and all(line.endswith(": ok") for line in lines), run.stdout
