"""Background build mode (viyadb_amd/csrc/vhh_build.h) on the device: queries of a VH_BUILD_BACKGROUND table never compile and never build a
layout, answer the oracle's rows from what exists, and converge on the steady state an inline table of the same history reaches.

Each case runs in a fresh child process with an empty JIT cache directory (tests/background_cases.py), under a time limit of its own; the
test stops at the first child that fails.
"""
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(name, seconds=420, extra=None):
    with tempfile.TemporaryDirectory() as cache:
        env = dict(os.environ, VH_JIT_CACHE_DIR=cache, VH_TEST_HOOKS="1", PYTHONPATH=ROOT)
        env.pop("VH_TEST_BUILD_HOLD", None)
        env.pop("VH_BUILD", None)
        env.update(extra or {})
        p = subprocess.run([sys.executable, "-m", "tests.background_cases", name], cwd=ROOT, env=env, capture_output=True, text=True, timeout=seconds)
    print(p.stdout[-6000:])
    print(p.stderr[-6000:], file=sys.stderr)
    assert p.returncode == 0 and "case ok" in p.stdout, f"case {name}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"


CASES = ("held_then_released", "sync_during_build", "hashed_partitioning", "readers_writer_build", "lifetimes", "host_shim")


def test_background_build_cases():
    """In order, one child each; the first child that fails ends the test, so that nothing more is started on a device that may have faulted."""
    for name in CASES:
        extra = {"VIYA_HIP_PLAN_FLAGS": str(1 << 18)} if name == "host_shim" else {}
        run_case(name, extra=extra)
