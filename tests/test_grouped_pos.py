"""Grouped payload records on the CPU: the place function the builder and the scan share (viyadb_amd/csrc/vh_grouped.h) over synthetic
tiles, and the compiled scan's shape with grouped records through the generator and hipRTC. No GPU needed."""
import os
import re
import subprocess

import ctypes as C

from viyadb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_place_function_on_synthetic_tiles(tmp_path):
    """tests/grouped_pos_host.cc builds the permutation of a tile with vh_grouped_pos() as group_bits_kernel does and finds every valid
    row's record again as the scan does — for every literal of the field and two beyond it, and snapshots that end at 0, inside a lane, at
    a lane's edge and at the tile's end. Tiles: all rows equal, none equal, one equal row in lane 0 bit 0 / lane 63 bit 31, 904 valid rows,
    2048 + 37 rows over two tiles, all 16 values of a 4-bit field. No place may reach the tile's valid rows."""
    exe = tmp_path / "grouped_pos_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "viyadb_amd", "csrc"),
                    os.path.join(ROOT, "tests", "grouped_pos_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 10 and all(line.endswith(": ok") for line in lines), run.stdout


def _selftest(which, tmp_path):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    return rc, buf.value.decode(), out


def test_grouped_shape_compiles_for_gfx950(tmp_path):
    """Selftest shape 21 = shape 14 (C3, bit-sliced predicates, 4-byte bit records) gathering from the grouped records by d2: the text the
    generator writes compiles for gfx950 without scratch or spills, carries the `==` leaf's mask and the header index, and differs from
    shape 14's (pp_group is part of the shape)."""
    rc, text, out = _selftest(21, tmp_path)
    assert rc == 0, text[:4000]
    assert "GROUPED = true" in text and "G_HDR = 14, G_BITS = 2" in text
    assert re.search(r"uint32_t gmask\(.*\n\s+return vj_bits_rel<2, 0>\(v \+ 0,", text) and "uint32_t glit(" in text
    assert os.path.getsize(out) > 4096
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", out], capture_output=True, text=True, check=True).stdout
    meta = {k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    rc14, text14, _ = _selftest(14, tmp_path)
    assert rc14 == 0 and "GROUPED = false" in text14 and "gmask(" not in text14
