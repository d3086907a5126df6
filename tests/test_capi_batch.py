"""The public surface of the batch entry point, as far as it can be checked without a GPU: include/viya_hip.h declares vh_query_agg_batch,
VH_BATCH_MAX and vh_batch_info and documents vh_result_info.reserved bit 30; viyadb_amd/capi.py binds the symbol and mirrors the struct; the
call refuses bad arguments before it touches a device and fails loudly, with the vh_init message, where there is none; the executor's result
tells a fused member from its flags."""
import ctypes as C
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()
VH_E_INVALID = -1


def test_the_symbol_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    assert re.search(r"VH_API\s+int\s+vh_query_agg_batch\s*\(\s*vh_table\*\s*t,\s*const\s+vh_plan\*\s*const\*\s*plans,\s*uint32_t\s+n,\s*vh_result\*\*\s*out", HEADER)
    assert "vh_query_agg_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.vh_query_agg_batch.restype is C.c_int and len(lib.vh_query_agg_batch.argtypes) == 5


def test_the_struct_and_the_constants_equal_the_header():
    assert re.search(r"#define\s+VH_BATCH_MAX\s+8\b", HEADER) and capi.BATCH_MAX == 8
    m = re.search(r"typedef struct vh_batch_info \{(.*?)\}\s*vh_batch_info;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [f[0] for f in capi.BatchInfo._fields_]
    assert C.sizeof(capi.BatchInfo) == 24
    assert capi.BatchInfo.fused_kernel_ms.offset == 16
    assert capi.INFO_BATCH_FUSED == 1 << 30
    infos = {n: v for n, v in vars(capi).items() if n.startswith("INFO_") and isinstance(v, int)}
    assert [n for n, v in infos.items() if v == 1 << 30] == ["INFO_BATCH_FUSED"]
    info = re.search(r"uint32_t\s+reserved;\s*/\*(.*?)\*/", HEADER, re.S).group(1)
    assert info.index("bit 29:") < info.index("bit 30:")
    bit30 = re.search(r"bit 30:(.*?)(?:bit \d+:|$)", info, re.S).group(1)
    assert "vh_query_agg_batch" in bit30 and "scan_agg_planes_batch_kernel" in bit30
    assert "48 KB" in HEADER and "VH_E_INVALID" in HEADER


def _plan():
    p = capi.Plan()
    return p


def test_bad_arguments_are_refused_before_a_device_is_touched():
    lib = capi.load()
    out = (C.c_void_p * 9)()
    plans = (C.POINTER(capi.Plan) * 9)(*[C.pointer(_plan()) for _ in range(9)])
    info = capi.BatchInfo(7, 7, 7, 7, 7.0, 7)
    assert lib.vh_query_agg_batch(None, plans, 1, out, C.byref(info)) == VH_E_INVALID            # a null table
    assert info.nplans == 0 and info.fused_groups == 0                                           # (the info is cleared whatever happens)
    fake = C.create_string_buffer(64)                                                            # never dereferenced by what follows
    t = C.cast(fake, C.c_void_p)
    assert lib.vh_query_agg_batch(t, plans, 9, out, None) == VH_E_INVALID                        # more than VH_BATCH_MAX
    assert b"max 8" in lib.vh_last_error()
    assert lib.vh_query_agg_batch(t, None, 0, None, None) == 0                                   # n == 0: nothing to do
    assert lib.vh_query_agg_batch(t, None, 1, out, None) == VH_E_INVALID
    assert lib.vh_query_agg_batch(t, plans, 1, None, None) == VH_E_INVALID
    holes = (C.POINTER(capi.Plan) * 3)(C.pointer(_plan()), None, C.pointer(_plan()))
    out[0] = 12345
    assert lib.vh_query_agg_batch(t, holes, 3, out, None) == VH_E_INVALID                        # a null plan
    assert lib.vh_last_error().startswith(b"plan 1: ") and out[0] is None


def test_the_call_fails_loudly_without_gpu_or_init():
    """No silent CPU fallback: without vh_init the entry point returns an error code and says so."""
    import torch
    if torch.cuda.is_available():
        return  # on the GPU box this path is covered by the -m gpu tests
    lib = capi.load()
    fake = C.create_string_buffer(64)
    out = (C.c_void_p * 2)()
    plans = (C.POINTER(capi.Plan) * 2)(C.pointer(_plan()), C.pointer(_plan()))
    rc = lib.vh_query_agg_batch(C.cast(fake, C.c_void_p), plans, 2, out, None)
    assert rc != 0 and b"vh_init" in lib.vh_last_error()
    assert out[0] is None and out[1] is None


def test_the_executor_tells_a_fused_member_from_its_flags():
    assert callable(executor.DeviceTable.query_agg_batch)
    assert isinstance(executor.AggResult.batch_fused, property) and executor.AggResult.batch_fused.fset is None
    fields = dataclasses.fields(executor.AggResult)
    blank = {f.name: None for f in fields if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING}
    assert executor.AggResult(**blank, flags=capi.INFO_BATCH_FUSED | capi.INFO_PLANE_AGG).batch_fused is True
    assert executor.AggResult(**blank, flags=capi.INFO_PLANE_AGG).batch_fused is False
