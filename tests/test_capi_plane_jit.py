"""PLAN2_PLANE_JIT at the C ABI's edge, without a GPU: the header (include/viya_hip.h) and viyadb_amd/capi.py agree on the flag, it shares no
bit with its neighbours, and vh_info_compose (viyadb_amd/csrc/vhh_info.h) with VhWhatRan::plane_jit gives bit 27's word plus bit 5 while
every combination tests/info_bits_host.cc checks stays what it was with the field false."""
import os
import re
import subprocess

from viyadb_amd import capi
from viyadb_amd.executor import AggResult, info_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_capi_agree_on_the_flag():
    header = open(os.path.join(ROOT, "include", "viya_hip.h")).read()
    m = {name: int(shift) for name, shift in re.findall(r"\b(VH_PLAN2_\w+) = 1u << (\d+)", header)}
    assert m == {"VH_PLAN2_PLANE_AGG": 0, "VH_PLAN2_PLANE_ROWS": 1, "VH_PLAN2_PLANE_JIT": 2}, m
    assert capi.PLAN2_PLANE_JIT == 1 << m["VH_PLAN2_PLANE_JIT"] and capi.PLAN2_PLANE_AGG == 1 and capi.PLAN2_PLANE_ROWS == 2
    # the module's own PLAN2_* names stay enum vh_plan_flags2's two; the second enum's bit is served by name (capi.__getattr__)
    assert sorted(n for n in vars(capi) if n.startswith("PLAN2_")) == ["PLAN2_PLANE_AGG", "PLAN2_PLANE_ROWS"]
    assert getattr(capi, "PLAN2_PLANE_JIT") == 4 and not hasattr(capi, "PLAN2_NO_SUCH_FLAG")
    assert "VH_PLANE_JIT=1" in header and "the compiled\n * kernel that runs the query is the plane aggregate's" in header


def test_a_result_with_bits_27_and_5_is_both():
    """AggResult.jit and AggResult.plane_agg come from the word's bits: both are true for a compiled plane aggregate's result."""
    got = info_fields(capi.INFO_PLANE_AGG | capi.INFO_JIT | capi.INFO_ON_PLANES)
    assert got["jit"] and got["sliced"] and got["predpack"] and got["narrow"], got
    assert not got["fast"] and not got["lanes"] and not got["sliced_prebuilt"] and not got["packed"], got
    class Word:                      # the properties read `.flags` and nothing else
        def __init__(self, flags):
            self.flags = flags
    both, alone = Word(capi.INFO_PLANE_AGG | capi.INFO_JIT | capi.INFO_ON_PLANES), Word(capi.INFO_PLANE_AGG | capi.INFO_ON_PLANES)
    assert AggResult.plane_agg.fget(both) and AggResult.plane_jit.fget(both) and info_fields(both.flags)["jit"]
    assert AggResult.plane_agg.fget(alone) and not AggResult.plane_jit.fget(alone) and not info_fields(alone.flags)["jit"]
    assert not AggResult.plane_agg.fget(Word(capi.INFO_JIT)) and not AggResult.plane_jit.fget(Word(capi.INFO_JIT))


def test_the_composer_with_the_new_field(tmp_path):
    exe = tmp_path / "plane_jit_info_host"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), "-I", os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "tests", "plane_jit_info_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 5 and all(line.endswith(": ok") for line in lines), run.stdout
