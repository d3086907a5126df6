"""The aggregates on the bit-sliced planes (viyadb_amd/csrc/vh_bits_agg.h: vh_bits_sum / vh_bits_min / vh_bits_max / vh_bits_group and their
`_at` forms; plain C++, compiled here by g++) against an evaluation row by row.

tests/bits_agg_host.cc is a stand-alone program. On random plane words with planted rows it checks: fields of 1, 5, 10, 11, 31 and 32 bits
at the first plane, the last planes and plane 1 of a 32-plane projection whose other planes hold noise; the masks empty, bit 0 alone, bit 31
alone, full and random; MIN and MAX with ties, with the value 0 present and with the empty mask reported as empty; the sum of 2^20 words of
all-ones 32-bit values, truncated to 32 bits, against a wrapping u32 add; the rows of every id of two group fields of 2 and 3 bits with lo > 0,
where a value outside [lo, lo + extent) is in no id's mask. It runs twice: plain, and with AddressSanitizer and UndefinedBehaviorSanitizer
(the plane words are an exact-size heap block, so a read outside them is an error)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bits_agg_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_aggregates_on_the_planes_equal_an_evaluation_row_by_row(tmp_path, sanitize):
    exe = str(tmp_path / "bits_agg_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
