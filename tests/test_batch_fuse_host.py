"""Which members of a batch share a fused launch (viyadb_amd/csrc/vh_batch.h: vh_batch_group; plain C++, compiled here by g++).

tests/batch_fuse_host.cc is a stand-alone program. Over hand-made and 20 000 random descriptor lists it checks: every candidate is in exactly
one group or left single, and no non-candidate is ever grouped; a group has two to VH_BATCH_MAX members of ONE fuse key (projection V, memory
scope, segments, chunks per segment) whose LDS tables sum to at most 48 KB; groups are numbered by their first members and a key's groups are
filled one after the other in plan order; a lone candidate is single; 8 equal candidates make one group; 8 candidates of 7 KB split six and
two, 7 of 8 KB six and a single; exactly 48 KB fits and 16 bytes more do not. It runs twice: plain, and with AddressSanitizer and
UndefinedBehaviorSanitizer (the lists are exact-size heap blocks, so an index outside them is an error)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "batch_fuse_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_grouping_of_a_batch(tmp_path, sanitize):
    exe = str(tmp_path / "batch_fuse_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
