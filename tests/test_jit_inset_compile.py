"""The two canonical plan shapes with a set leaf (VH_F_INSET; viyadb_amd/csrc/vh_jit.hip, vj_canonical) through the generator and
hipRTC, on the CPU: the text compiles for gfx950, takes no scratch and spills nothing, and holds no trace of a list's length — the
set's form, bounds and size are run-time data, so every list on a shape runs one code object.

(tests/test_jit_compile.py's `_meta` check, re-stated: that file is a yardstick of its own. The shapes are numbered 23 and 24 — 21
and 22 were taken by the grouped records and the clustered planes.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from viyadb_amd import capi

LLVM = "/opt/rocm/lib/llvm/bin"
SHAPES = {23: "C3 with its d3 leaf as a set, the columns bit fields of a predicate projection's byte planes",
          24: "a NOT-IN set on an i64 column from the arenas, hash path with the LDS front table"}


def _compile(which, tmp_path):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    return rc, buf.value.decode(), out


def _meta(path):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_set_leaf_shapes_compile_without_scratch(which, tmp_path):
    rc, text, out = _compile(which, tmp_path)
    assert rc == 0, f"{SHAPES[which]}:\n{text[:4000]}"
    assert "vj_scan<VJ>" in text and os.path.getsize(out) > 4096
    # the leaf is a lookup in P.set[0] on the column's own element type, in the mask and in the bool expression alike
    T = "uint32_t" if which == 23 else "int64_t"
    assert f"vj_inset<{T}>(L.s0, c{1 if which == 23 else 0}<I>(v))" in text and "s0(P.set[0])" in text, text[:3000]
    assert ("vj_b(z0)" in text and "(z0)" in text) if which == 23 else ("vj_b(!z0)" in text and "(!z0)" in text)
    m = _meta(out)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (SHAPES[which], m)
