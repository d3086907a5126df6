"""The pipelined drain (vj_drain_pipe, viyadb_amd/csrc/vh_jit_body.h), CPU side: the selftest shapes that carry a drain depth compile for
gfx950 (hipRTC cross-compiles without a GPU), stay free of scratch and within the registers five blocks of four waves per CU would need,
and the scan kernel's instruction order is the pipeline's — a survivor's record load is still in flight when the ring writer's first LDS
atomic of the group before it is issued — while depth 0 waits for every record behind its load, as it always did."""
import ctypes as C
import hashlib
import re
import subprocess

import pytest

from viyadb_amd import capi

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "viya_jit_scan_selftest"
SHAPES = {25: "shape 22 (clustered planes beside the grouped records) at depth 1",
          26: "shape 22 at depth 2",
          27: "shape 21 (row-order planes over the grouped records) at the default depth",
          28: "shape 7 (the compressed 8-byte record) at the default depth",
          29: "shape 1 (the arenas: no packed record) at the default depth"}


def _compile(which, tmp_path, tag=""):
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    buf = C.create_string_buffer(1 << 20)
    out = str(tmp_path / f"shape{which}{tag}.hsaco")
    rc = lib.vh_jit_selftest(which, out.encode(), buf, len(buf))
    assert rc == 0, f"shape {which}:\n{buf.value.decode()[:4000]}"
    return buf.value.decode(), out


def _meta(path, kernel=KERNEL):
    """The notes of ONE kernel of the code object (it holds phase 2 and the hashed partitioning's planner beside the scan)."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    mine = [b for b in re.split(r"\n\s+- \.", notes) if re.search(rf"\.name:\s+{kernel}\s*\n", b)]
    assert len(mine) == 1, (kernel, len(mine))
    return {k: int(re.search(rf"\.?{k}:\s+(\d+)", mine[0]).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}


def _scan_lines(path):
    isa = subprocess.run([f"{LLVM}/llvm-objdump", "-d", path], capture_output=True, text=True, check=True).stdout
    body = isa[isa.index(f"<{KERNEL}>:"):]
    nxt = re.search(r"\n[0-9a-f]+ <", body[10:])
    return [l.split("//")[0].strip() for l in (body[:nxt.start() + 10] if nxt else body).splitlines()]


def _text_hash(path, tmp_path):
    out = str(tmp_path / "text.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", path, out], check=True)
    with open(out, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _record_loads(L):
    """(line of a survivor's record load, line of the ring writer's next LDS atomic, the vmcnt waits between them). The record is the one
    4-byte global load through a lane's own 64-bit address whose value becomes the tuple a few dozen instructions later; the planes and
    headers are loaded elsewhere, hundreds of instructions from the nearest atomic."""
    sites = []
    for i, l in enumerate(L):
        if not re.match(r"global_load_dword v\d+, v\[\d+:\d+\], off", l):
            continue
        j = next((k for k in range(i + 1, min(len(L), i + 120)) if L[k].startswith("ds_add_rtn_u32")), None)
        if j is not None:
            sites.append((i, j, [L[k] for k in range(i + 1, j) if re.match(r"s_waitcnt.*vmcnt\(", L[k])]))
    return sites


@pytest.mark.parametrize("which", sorted(SHAPES))
def test_drain_shapes_compile_without_scratch(which, tmp_path):
    text, out = _compile(which, tmp_path)
    assert "vj_scan<VJ>" in text
    depth = int(re.search(r"DRAIN_DEPTH = (\d+)", text).group(1)), int(re.search(r"REC_BYTES = (\d+)", text).group(1))
    assert depth == {25: (1, 4), 26: (2, 4), 27: (1, 4), 28: (1, 8), 29: (0, 0)}[which], (SHAPES[which], depth)
    m = _meta(out)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (SHAPES[which], m)


def test_clustered_shape_leaves_room_for_five_blocks(tmp_path):
    """Five blocks of four waves per CU are five waves per SIMD: at most 96 registers (512 / 5, in blocks of 8)."""
    for which in (25, 26):
        _, out = _compile(which, tmp_path)
        m = _meta(out)
        assert m["vgpr_count"] <= 96, (SHAPES[which], m)


@pytest.mark.parametrize("which", [25, 26])
def test_record_load_stays_in_flight_across_the_sink(which, tmp_path):
    _, out = _compile(which, tmp_path)
    sites = _record_loads(_scan_lines(out))
    assert sites, "no record load found"
    free = [s for s in sites if not s[2]]
    assert free, (SHAPES[which], [(i, j, w) for i, j, w in sites])


def test_depth_0_waits_behind_every_record_load(tmp_path):
    _, out = _compile(22, tmp_path)
    sites = _record_loads(_scan_lines(out))
    assert sites, "no record load found"
    assert all(w for _, _, w in sites), [(i, j, w) for i, j, w in sites]


def test_arena_shape_ignores_the_depth(tmp_path, monkeypatch):
    """No packed record, no pipeline: the same bytes of code whatever VH_TEST_DRAIN_DEPTH asks for."""
    monkeypatch.delenv("VH_TEST_DRAIN_DEPTH", raising=False)
    _, plain = _compile(1, tmp_path)
    want = _text_hash(plain, tmp_path)
    for depth in ("0", "2"):
        monkeypatch.setenv("VH_TEST_DRAIN_DEPTH", depth)
        for which in (1, 29):
            _, out = _compile(which, tmp_path, tag=f"_d{depth}")
            assert _text_hash(out, tmp_path) == want, (which, depth)
    # ... and a shape with a packed record does follow it: the hook reaches the generator
    monkeypatch.setenv("VH_TEST_DRAIN_DEPTH", "2")
    text, _ = _compile(27, tmp_path, tag="_d2")
    assert "DRAIN_DEPTH = 2" in text
    monkeypatch.setenv("VH_TEST_DRAIN_DEPTH", "0")
    text, out0 = _compile(27, tmp_path, tag="_d0")
    assert "DRAIN_DEPTH = 0" in text
    _, base = _compile(21, tmp_path)
    assert _text_hash(out0, tmp_path) == _text_hash(base, tmp_path)
