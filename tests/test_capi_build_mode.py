"""The background build mode's boundary, without a GPU: vh_table_set_build_mode / vh_table_build_wait / vh_table_build_info are declared in
include/viya_hip.h, exported by the library and bound in capi.SYMBOLS; vh_build_info's ctypes mirror has the header's size and field order;
without vh_init the entry points fail loudly like the rest."""
import ctypes as C
import os
import re

from viyadb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vh_table_set_build_mode", "vh_table_build_wait", "vh_table_build_info")


def _header():
    return open(os.path.join(ROOT, "include", "viya_hip.h")).read()


def test_entry_points_declared_exported_and_bound():
    lib = capi.load()
    declared = set(re.findall(r"VH_API\s+[\w\s\*]+?\b(vh_\w+)\s*\(", _header()))
    for name in NAMES:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == capi.SYMBOLS[name][1]
    assert re.search(r"VH_BUILD_INLINE\s*=\s*0\s*,\s*VH_BUILD_BACKGROUND\s*=\s*1", _header())
    assert (capi.BUILD_INLINE, capi.BUILD_BACKGROUND) == (0, 1)


def test_build_info_mirror_matches_header():
    body = re.search(r"typedef struct vh_build_info \{(.*?)\} vh_build_info;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in capi.BuildInfo._fields_]
    for (ctype, name), (_, py) in zip(fields, capi.BuildInfo._fields_):
        assert py is (C.c_uint64 if ctype == "uint64_t" else C.c_double), name
    assert C.sizeof(capi.BuildInfo) == 8 * len(fields) == 128


def test_pending_bit_is_documented_and_free():
    """Bit 19 of vh_result_info.reserved: above the projection's record size (bits 16-18), named in the header's list."""
    assert capi.INFO_BUILD_PENDING == 1 << 19
    assert "bit 19:" in _header()


def test_calls_fail_loudly_without_init():
    lib = capi.load()
    bi = capi.BuildInfo()
    assert lib.vh_table_set_build_mode(None, capi.BUILD_BACKGROUND) != 0
    assert lib.vh_last_error()
    assert lib.vh_table_build_wait(None, 1, C.byref(bi)) != 0
    assert lib.vh_table_build_info(None, C.byref(bi)) != 0
