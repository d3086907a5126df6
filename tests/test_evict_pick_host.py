"""Which derived layouts leave when the byte budget is short (vh_evict_pick, viyadb_amd/csrc/vhh_layout_math.h) on the CPU, against a
brute-force model. A stand-alone program under AddressSanitizer and UBSan; the library is not loaded. No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_victim_choice_against_brute_force(tmp_path):
    """tests/evict_pick_host.cc: 64 seeds x 200 random sets of at most 12 layouts with random bytes, pins and ticks (some ticks equal, some
    the current one), each against eight deficits from 0 to 2^64 - 1: "impossible" exactly when the evictable bytes are less than the
    deficit, and then no victim; the victims a prefix of the (last_use, serial) order, a minimal one, none pinned and none stamped with
    the current tick. Then the edge cases one by one: an empty set, deficit 0, everything pinned, equal ticks, byte counts near 2^64."""
    exe = tmp_path / "evict_pick_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), os.path.join(ROOT, "tests", "evict_pick_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 68 and all(line.endswith(": ok") for line in lines), run.stdout
