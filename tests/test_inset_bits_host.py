"""The truth-table form of a VH_F_INSET leaf (viyadb_amd/csrc/vh_inset.h: vh_inset_bits, vh_inset_truth_build; plain C++, compiled
here by g++) against a per-row linear search.

tests/inset_bits_host.cc is a stand-alone program: for every field width from 1 to 10 bits it takes 32-row plane words (all zeros, all
ones, rows that hold members and their neighbours, random) and sets that are empty after clipping, hold one member, member 0, member
2^NB - 1, the word edge 31 / 32 / 33, every value, every other value and random densities, on an unsigned and on a signed element type.
It runs twice: plain, and with AddressSanitizer and UndefinedBehaviorSanitizer (the tables are exact-size heap copies, so a read past
the end is an error, not a lucky read)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "inset_bits_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_truth_table_equals_a_linear_search(tmp_path, sanitize):
    exe = str(tmp_path / "inset_bits_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
