"""Which members of one fused launch share a pass mask (viyadb_amd/csrc/vh_batch.h: vh_batch_share; plain C++, compiled here by g++).

tests/batch_share_host.cc is a stand-alone program. Over hand-made and 20 000 random member lists it checks: mask_of[k] <= k and
mask_of[mask_of[k]] == mask_of[k]; two members share exactly when the mask key is equal, held against a naive pairwise comparison on the
test's own representation, and a follower points at the FIRST member of its class; one literal, one op (lt / le, AND / OR), `flat`, F's
serial, planes, stride or pitch, has_filter, one row of one segment, a skipped segment or the number of segments separate two members; a set
leaf never shares, even with an identical twin; no-filter members with equal rows share; ops beyond nprog (filled with a different pattern
in every member) and literals no op refers to do not matter; all literals of an IN leaf do; eight equal members give one class, eight
different ones eight; A, B, A, none, B, none, A gives three, also for a launch that holds a sub-list in another order. It runs twice: plain,
and with AddressSanitizer and UndefinedBehaviorSanitizer (programs, literals and snapshots are exact-size heap blocks, so a read outside
the used part is an error)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "batch_share_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_mask_classes_of_a_fused_launch(tmp_path, sanitize):
    exe = str(tmp_path / "batch_share_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
