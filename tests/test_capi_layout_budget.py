"""The C ABI of the layout budget (include/viya_hip.h: vh_table_set_layout_budget, vh_table_layouts, vh_table_layout_pin,
vh_table_layout_drop) as far as it can be checked without a GPU: the ctypes mirrors of its two structures against the header's own
declarations, and the calls' answers to a NULL table."""
import ctypes as C
import os
import re

from viyadb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()
SIZES = {"uint64_t": 8, "int64_t": 8, "uint32_t": 4, "int32_t": 4, "uint16_t": 2, "uint8_t": 1}


def _declared(name):
    """[(field, offset, size)] and sizeof of `typedef struct <name> { ... }` as a C compiler lays it out (natural alignment), from the header."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(VH_\w+)\s+(\d+)\s*$", HEADER, re.M)}
    fields, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, names = decl.split(None, 1)
        size = SIZES[typ]
        align = max(align, size)
        for n in (x.strip() for x in names.split(",")):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", n)
            count = 1 if m.group(2) is None else macros[m.group(2)] if m.group(2) in macros else int(m.group(2))
            off = (off + size - 1) // size * size
            fields.append((m.group(1), off, size * count))
            off += size * count
    return fields, (off + align - 1) // align * align


def _check(name, mirror):
    fields, size = _declared(name)
    assert C.sizeof(mirror) == size, (name, C.sizeof(mirror), size)
    assert [f[0] for f in mirror._fields_] == [f[0] for f in fields], name
    for fname, off, fsize in fields:
        d = getattr(mirror, fname)
        assert (d.offset, d.size) == (off, fsize), (name, fname, d.offset, d.size, off, fsize)
    return {f[0]: f[1] for f in fields}


def test_structures_match_the_header():
    offs = _check("vh_layout_info", capi.LayoutInfo)
    assert offs["bytes"] == 144 and capi.LayoutInfo.bytes.offset == 144
    assert C.sizeof(capi.LayoutInfo) == 184
    _check("vh_layout_summary", capi.LayoutSummary)
    assert C.sizeof(capi.LayoutSummary) == 64
    assert capi.LAYOUT_COLS == int(re.search(r"#define\s+VH_LAYOUT_COLS\s+(\d+)", HEADER).group(1))
    kinds = dict(re.findall(r"(VH_LAYOUT_[A-Z_]+)\s*=\s*(\d+)", re.search(r"enum\s+vh_layout_kind\s*\{(.*?)\}", HEADER, re.S).group(1)))
    assert {k: int(v) for k, v in kinds.items()} == {"VH_LAYOUT_PROJECTION": capi.LAYOUT_PROJECTION, "VH_LAYOUT_PRED_BYTES": capi.LAYOUT_PRED_BYTES,
                                                     "VH_LAYOUT_PRED_SLICED": capi.LAYOUT_PRED_SLICED, "VH_LAYOUT_NARROW": capi.LAYOUT_NARROW}
    assert capi.INFO_EVICTED == 1 << 24 and re.search(r"bit 24:", HEADER)


def _calls(lib, t):
    n, summ = C.c_uint32(77), capi.LayoutSummary()
    return [("vh_table_set_layout_budget", lambda: lib.vh_table_set_layout_budget(t, 1 << 20)),
            ("vh_table_layouts", lambda: lib.vh_table_layouts(t, None, 0, C.byref(n), C.byref(summ))),
            ("vh_table_layout_pin", lambda: lib.vh_table_layout_pin(t, 1, 1)),
            ("vh_table_layout_drop", lambda: lib.vh_table_layout_drop(t, 1))]


def test_null_table_is_invalid_with_a_message():
    """VH_E_INVALID (-1) and a message that names the call and the NULL table, with or without vh_init: that test comes first."""
    lib = capi.load()
    for name, call in _calls(lib, None):
        rc = call()
        msg = lib.vh_last_error()
        assert rc == -1, (name, rc)
        assert msg and name.encode() + b": null table" in msg, (name, msg)


def test_calls_fail_loudly_without_init():
    """Without vh_init (no GPU in this process) the four entry points say so instead of pretending, as vh_table_create does. The table
    they are given is a block of zeroes that no code may look into before vh_init has been asked about."""
    import torch
    if torch.cuda.is_available():
        return  # on the GPU box this path is covered by the -m gpu tests
    lib = capi.load()
    fake = C.create_string_buffer(1 << 16)
    for name, call in _calls(lib, C.cast(fake, C.c_void_p)):
        assert call() == -1 and b"vh_init" in lib.vh_last_error(), name
