"""The sub-sorted grouped form on the CPU: the composite order, the boundary keys and the run trimming the builder and the scan share
(viyadb_amd/csrc/vh_grouped.h) over synthetic tiles, built plain and under AddressSanitizer and UBSan. No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = 22


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_sub_sorted_tiles_and_trims(tmp_path, flags):
    """tests/gsub_host.cc orders synthetic tiles as group_bits_kernel does (vh_gsub_sort_word sorted as integers), derives start[], the
    places and kfirst[], and checks vh_gsub_trim against brute force for LT, LE, GT, GE, EQ and every literal from 0 to the field maximum:
    the stretch holds every qualifying place and is cut at multiples of 32 only. Tiles: runs of 0, 1, 31, 32, 33 and 2048 places; runs that
    start at places 31, 32, 33; all keys equal; a key repeated across word boundaries; keys 0 and the field maximum at 10 and 16 bits; 904
    valid rows; grouping values and a key value no row has; an empty tile. Boundary keys of places outside a run are poisoned: reading one
    cuts a qualifying place away."""
    exe = tmp_path / "gsub_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "viyadb_amd", "csrc"),
                    os.path.join(ROOT, "tests", "gsub_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == TILES and all(line.endswith(": ok") for line in lines), run.stdout
