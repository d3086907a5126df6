"""Compiled and pre-built candidates of a batch never share a fused launch, and members of a compiled launch share a pass mask only under
equal filter texts (viyadb_amd/csrc/vh_batch.h: VhFuseDesc::compiled, VhShareDesc::filter_shape; plain C++, compiled here by g++).

tests/batch_jit_fuse_host.cc is a stand-alone program. Over hand-made and 6 000 random descriptor lists it holds vh_batch_group to a
brute-force restatement — the list split by kind, each half grouped by the rule without the field, the groups numbered by their first members
— and checks that no group mixes the kinds, that the caps apply per group and that a lone candidate of either kind stays single. Over 4 000
random launches it holds vh_batch_share to the pairwise comparison with the filter shape as one more condition, with mask_of[k] <= k and
mask_of[mask_of[k]] == mask_of[k]. It runs twice: plain, and with AddressSanitizer and UndefinedBehaviorSanitizer (exact-size heap blocks)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "batch_jit_fuse_host.cc")
INC = os.path.join(ROOT, "viyadb_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_compiled_and_prebuilt_candidates(tmp_path, sanitize):
    exe = str(tmp_path / "batch_jit_fuse_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok: ")
