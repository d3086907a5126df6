"""The wave scans by DPP (viyadb_amd/csrc/vh_wave_scan.h) in the compiled scan, CPU side: the selftest shapes of the bit-sliced scans compile
for gfx950 (hipRTC cross-compiles without a GPU) without scratch or spills; C3's form — shape 25, the clustered planes at drain depth 1 —
keeps only the ten ds_bpermute_b32 that fetch a tile's parameters (it held 40: six per prefix scan and six for the search item -> tile),
its scans are DPP chains that end in row_bcast:31, and it still fits five blocks per CU; -DVH_WAVE_SCAN_SHFL=1 brings the 40 back."""
import ctypes as C
import re
import subprocess

import pytest

from viyadb_amd import capi

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "viya_jit_scan_selftest"
SHAPES = {14: "C3 on the bit-sliced planes", 22: "the clustered planes beside the grouped records", 25: "shape 22 at drain depth 1",
          26: "shape 22 at drain depth 2", 27: "row-order planes over the grouped records at the default depth"}


def _compile(which, tmp_path, tag=""):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}{tag}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    assert rc == 0, f"shape {which}:\n{buf.value.decode()[:4000]}"
    return out


def _meta(path):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    mine = [b for b in re.split(r"\n\s+- \.", notes) if re.search(rf"\.name:\s+{KERNEL}\s*\n", b)]
    assert len(mine) == 1, len(mine)
    return {k: int(re.search(rf"\.?{k}:\s+(\d+)", mine[0]).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}


def _scan_isa(path):
    isa = subprocess.run([f"{LLVM}/llvm-objdump", "-d", path], capture_output=True, text=True, check=True).stdout
    body = isa[isa.index(f"<{KERNEL}>:"):]
    nxt = re.search(r"\n[0-9a-f]+ <", body[10:])
    return body[:nxt.start() + 10] if nxt else body


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_shapes_compile_without_scratch(which, tmp_path, monkeypatch):
    monkeypatch.delenv("VH_JIT_FLAGS", raising=False)
    m = _meta(_compile(which, tmp_path))
    print(f"shape {which}: {m}")
    # (scalar registers parked in lanes of a vector register are no scratch: the count is printed for the round's notes, not asserted)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (SHAPES[which], m)
    if which in (25, 26):       # five blocks of four waves per CU: at most 96 registers
        assert m["vgpr_count"] <= 96, (SHAPES[which], m)


def test_clustered_scan_keeps_only_the_parameter_shuffles(tmp_path, monkeypatch):
    monkeypatch.delenv("VH_JIT_FLAGS", raising=False)
    isa = _scan_isa(_compile(25, tmp_path))
    n = len(re.findall(r"\bds_bpermute_b32\b", isa))
    print(f"shape 25: {n} ds_bpermute_b32, {len(re.findall(r'row_bcast:31', isa))} row_bcast:31")
    assert n <= 10, n
    assert "row_bcast:31" in isa and "v_add_u32_dpp" in isa and "v_max_u32_dpp" in isa


def test_the_switch_brings_the_shuffles_back(tmp_path, monkeypatch):
    monkeypatch.setenv("VH_JIT_FLAGS", "-DVH_WAVE_SCAN_SHFL=1")
    out = _compile(25, tmp_path, tag="_shfl")
    isa = _scan_isa(out)
    assert len(re.findall(r"\bds_bpermute_b32\b", isa)) == 40 and "row_bcast:31" not in isa
    m = _meta(out)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
