"""The set of a VH_F_INSET leaf (viyadb_amd/csrc/vh_inset.h, plain C++: compiled here by g++) against a linear search.

tests/inset_host.cc is a stand-alone program: for every integer element type it builds lists of 1 to 3000 members (duplicates, the
type's min and max), lists whose span sits on either side of every boundary of the two lookup forms (31 .. 65, 2^20 - 1 | 2^20,
2^32 - 1 | 2^32 and beyond), builds each in the form the builder picks and in the forced sorted-array form, and asks both for every
member, member +- 1, the type's extremes and 10 000 random values. It runs twice: plain, and with AddressSanitizer and
UndefinedBehaviorSanitizer (the tables are exact-size copies, so an index past the end is an error, not a lucky read)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "inset_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_both_forms_equal_a_linear_search(tmp_path, sanitize):
    exe = str(tmp_path / "inset_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
