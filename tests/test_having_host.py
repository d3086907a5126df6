"""The HAVING comparison and its postfix evaluation on the CPU: what the emission kernels include (viyadb_amd/csrc/vh_having.h) against the
typed C++ comparisons, built plain and under AddressSanitizer and UBSan as a stand-alone program. No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKS = 10 + 1 + 3 + 3 + 1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_comparison_and_program(tmp_path, flags):
    """tests/having_host.cc: every element type x every relation x every ordered pair of the type's edge values (those of tests/extremes.py;
    floats with -0.0 against +0.0 and NaN against everything: `ne` holds, the rest fail) against the C++ typed comparison; the same pairs
    with the bytes above the type's own set (truncation is the contract: a `byte` sum that wrapped); IN and NOT IN with 0, 1 and 24
    literals; AND and OR of 1, 2 and 8 operands over every combination of operand values; a program of 16 nodes at stack depth 8 against
    an independent evaluation of the same tree."""
    exe = tmp_path / "having_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "viyadb_amd", "csrc"),
                    os.path.join(ROOT, "tests", "having_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == CHECKS and all(line.endswith(": ok") for line in lines), run.stdout
