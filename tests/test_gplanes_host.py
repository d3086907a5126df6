"""Clustered predicate planes on the CPU: the addressing and run arithmetic the builder and the scan share (viyadb_amd/csrc/vh_grouped.h)
over synthetic tiles, under AddressSanitizer and UBSan, and the compiled scan's shape that reads them through the generator and hipRTC.
No GPU needed."""
import os
import re
import subprocess

import ctypes as C

from viyadb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_clustered_planes_on_synthetic_tiles(tmp_path):
    """tests/gplanes_host.cc builds a tile's clustered block as group_bits_kernel does (permutation, header, squeezed words spread over the
    planes, word-major) and finds every passing row as the scan does (the run's words, the in-run mask, place = bit position), against a
    plain row-order evaluation, for every literal of the field and two beyond it. Tiles: all rows one value; values with no rows; runs of
    exactly 1, 31, 32, 33 and 2047 places starting at places 0, 1, 31, 32, 33, 1000 and ending at 2048 and one short of it; 904 valid
    rows; all 16 values of a 4-bit field; the field's last value, whose run ends with the valid rows. A stand-alone program built with
    -fsanitize=address,undefined: its block is exactly 256 G bytes, so a step outside it is an error."""
    exe = tmp_path / "gplanes_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "viyadb_amd", "csrc"), os.path.join(ROOT, "tests", "gplanes_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 43 and all(line.endswith(": ok") for line in lines), run.stdout


def _selftest(which, tmp_path):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    return rc, buf.value.decode(), out


def test_clustered_shape_compiles_for_gfx950(tmp_path):
    """Selftest shape 22 = shape 21 (C3 gathering from the records grouped by d2) reading the clustered planes: the text compiles for
    gfx950 without scratch or spills, loads a word group of 20 dwords with five 16-byte non-temporal loads, evaluates the filter without
    the `==` leaf on d2, and differs from shape 21's (the arena's slot and G are part of the shape)."""
    rc, text, out = _selftest(22, tmp_path)
    assert rc == 0, text[:4000]
    assert "GROUPED = true" in text and "GPLANES = true" in text and "GP_SLOT = 15, GP_G = 20, NVG = 20" in text
    mask = re.search(r"uint32_t gp_mask\(.*\n.*\n\s+return (.*);", text).group(1)
    assert "vj_bits_rel<10, 2>(vg + 0," in mask and "vj_bits_rel<10, 5>(vg + 10," in mask and "vj_bits_rel<2," not in mask, mask
    at = text.index("void gp_load(")
    load = text[at:text.index("\n  }\n", at)]
    assert load.count("__builtin_nontemporal_load(VJ_GLOBAL(vh_u32x4, grp)") == 5 and "VJ_GLOBAL(uint32_t, grp)" not in load, load[:2000]
    assert os.path.getsize(out) > 4096
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", out], capture_output=True, text=True, check=True).stdout
    scan = notes[notes.index(".name:           viya_jit_scan_selftest\n"):]
    meta = {k: int(re.search(rf"\.{k}:\s+(\d+)", scan).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    rc21, text21, _ = _selftest(21, tmp_path)
    assert rc21 == 0 and "GPLANES = false" in text21 and "gp_mask(" not in text21
