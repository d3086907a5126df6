"""The canonical plan shapes with a set leaf ON THE BIT-SLICED PLANES (VH_F_INSET as a truth table over its field: vj_bits_inset,
viyadb_amd/csrc/vh_jit_body.h; vh_inset_bits, vh_inset.h) through the generator and hipRTC, on the CPU: the text compiles for gfx950,
takes no scratch and spills nothing, names the field's bits and the set's index and nothing of the list — so every list on a shape
runs one code object — and holds no per-row lookup.

Shape 30 = shape 14 (C3 on the bit-sliced planes) with its d3 leaf as a set, 31 = shape 22 (the clustered planes) likewise, 32 = shape 14
with a NOT-IN set on the 2-bit d2 field. Each shape's register count is printed beside shape 14's (a number for the round's notes, not
an assertion)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from viyadb_amd import capi

LLVM = "/opt/rocm/lib/llvm/bin"
SHAPES = {30: "C3 on the bit-sliced planes with its d3 leaf (10 bits) as a set",
          31: "the same over the clustered planes beside the grouped records",
          32: "C3 on the bit-sliced planes with a NOT-IN set on the 2-bit d2 field"}


def _compile(which, tmp_path):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    return rc, buf.value.decode(), out


def _meta(path):
    """The SCAN kernel's entry of the code object's metadata (the module holds other kernels too: keys come in alphabetical order, so a
    kernel's figures lie between its .name and the next kernel's .agpr_count)."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    at = re.search(r"\.name:\s+viya_jit_scan_selftest\s*\n", notes)
    assert at, notes[:2000]
    mine = notes[at.end():]
    mine = mine[:mine.find(".agpr_count") if ".agpr_count" in mine else len(mine)]
    return {k: int(re.search(rf"\.{k}:\s+(\d+)", mine).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}


@pytest.fixture(scope="module")
def shape14(tmp_path_factory):
    rc, text, out = _compile(14, tmp_path_factory.mktemp("shape14"))
    assert rc == 0, text[:4000]
    return _meta(out)


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_set_leaf_on_bit_planes_compiles_without_scratch(which, tmp_path, shape14):
    rc, text, out = _compile(which, tmp_path)
    assert rc == 0, f"{SHAPES[which]}:\n{text[:4000]}"
    assert "vj_scan<VJ>" in text and os.path.getsize(out) > 4096
    assert "static constexpr bool SLICED = true" in text
    # the leaf: the field's bits, where its planes lie in the lane's registers, the set's index — and its truth table's address out of P.set
    assert "s0(P.set[0].truth)" in text and "const uint32_t* s0;" in text, text[:3000]
    if which == 30:
        assert "vj_bits_inset<10>(v + 2, L.s0)" in text and "~vj_bits_inset" not in text
    elif which == 31:
        assert "static constexpr bool GPLANES = true" in text
        assert "vj_bits_inset<10>(vg + 0, L.s0)" in text        # the clustered planes hold no plane of d2: d3's come first
        assert "vj_bits_inset<10>(v + 2, L.s0)" in text         # ... and the row-order form of the same filter beside it
    else:
        assert "~vj_bits_inset<2>(v + 0, L.s0)" in text
    # no lookup per row, no marker of the old pairing, nothing of a list
    assert "vj_inset<" not in text and "VhSetDev s0" not in text and "vj_a_set_leaf" not in text
    m = _meta(out)
    print(f"shape {which}: {m}   shape 14: {shape14}")
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (SHAPES[which], m)


def test_old_shapes_keep_their_text(tmp_path):
    """The rows-form set leaf (shape 23) still looks members up per row in a VhSetDev; shape 14 knows nothing of sets."""
    rc, text, _ = _compile(23, tmp_path)
    assert rc == 0 and "VhSetDev s0" in text and "vj_inset<uint32_t>(L.s0, c1<I>(v))" in text and "vj_bits_inset" not in text
    rc, text, _ = _compile(14, tmp_path)
    assert rc == 0 and "vj_bits_inset" not in text and "P.set" not in text
