"""The bit-serial filter evaluator of the select kernels (viyadb_amd/csrc/vh_bits_eval.h: vh_bits_eval; plain C++, compiled here by
g++) against a per-row evaluation of the same program.

tests/bits_eval_host.cc is a stand-alone program. On random plane words, with rows planted that hold the literals and their neighbours,
it runs: every relation on fields of 1, 5, 10, 11, 31 and 32 bits with the literals 0, 1, 2^NB - 1, 2^NB, 2^40 and, on signed element
types, -1 and the smallest value; IN / NOT IN of 1, 2 and 8 values with duplicates; set leaves on fields of 1 to 10 bits; flat AND / OR
programs (with and without the flat short cut), nests of VH_MAX_STACK operands and random trees over three fields. It runs twice: plain,
and with AddressSanitizer and UndefinedBehaviorSanitizer (the planes are an exact-size heap block, so a read outside them is an error)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bits_eval_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bit_serial_evaluation_equals_a_per_row_evaluation(tmp_path, sanitize):
    exe = str(tmp_path / "bits_eval_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
