"""The derived layouts' arithmetic on the CPU (viyadb_amd/csrc/vhh_layout_math.h): the job cutter against a per-row model of what is stale,
and the width functions against a table recorded from the functions they replaced. A stand-alone program under AddressSanitizer and
UBSan; the library is not loaded. No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_math_against_brute_force(tmp_path):
    """tests/layout_math_host.cc: 24 seeded random journals over 3 segments of at most 40 000 rows, every applied_epoch from 0 to the last, with
    and without a floor, plain and widened to tiles — every stale row below the row limit in exactly one job, jobs on 256-row boundaries of
    at most VH_JOB_ROWS rows that neither overlap nor pass the limit and carry the segment's rows — then the edge cases one by one (a range
    that ends on a boundary and one past it, ranges that touch and overlap, a range longer than VH_JOB_ROWS, a segment the layout never
    held, applied_epoch 0 / below / exactly at the floor, entries beyond nseg, the partial last tile of a 5 000-row segment), then the
    width functions for every element type."""
    exe = tmp_path / "layout_math_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), os.path.join(ROOT, "tests", "layout_math_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 32 and all(line.endswith(": ok") for line in lines), run.stdout
