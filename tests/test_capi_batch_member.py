"""The public surface of vh_result_batch_member, as far as it can be checked without a GPU: include/viya_hip.h declares the call and
vh_batch_member_info, viyadb_amd/capi.py binds the symbol and mirrors the struct field for field (24 bytes, no field named `reserved`), the
built library exports it and refuses null arguments, the executor's result carries it as an attribute with a default, and the header
comment of vh_query_agg_batch states the rule by which members of a fused launch share a pass mask."""
import ctypes as C
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()
VH_E_INVALID = -1
FIELDS = ["fused", "launch", "position", "members", "mask_of", "mask_classes"]


def test_the_struct_equals_the_header():
    m = re.search(r"typedef struct vh_batch_member_info \{(.*?)\}\s*vh_batch_member_info;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\buint32_t\s+(\w+)\s*;", body) == FIELDS == [f[0] for f in capi.BatchMemberInfo._fields_]
    assert re.findall(r"\b(\w+)\s*[,;]", body) == FIELDS                       # nothing but these, whatever the type
    assert all(f[1] is C.c_uint32 for f in capi.BatchMemberInfo._fields_)
    assert C.sizeof(capi.BatchMemberInfo) == 24
    assert "reserved" not in FIELDS
    # vh_batch_info is as it was
    assert [f[0] for f in capi.BatchInfo._fields_] == ["nplans", "fused_groups", "fused_members", "singles", "fused_kernel_ms", "reserved"]


def test_the_symbol_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    assert re.search(r"VH_API\s+int\s+vh_result_batch_member\s*\(\s*vh_result\*\s*r,\s*vh_batch_member_info\*\s*out\s*\)", HEADER)
    assert "vh_result_batch_member" in capi.SYMBOLS
    lib = capi.load()
    assert lib.vh_result_batch_member.restype is C.c_int and len(lib.vh_result_batch_member.argtypes) == 2
    raw = C.CDLL(lib._name)                                                     # the shared object itself exports it
    assert hasattr(raw, "vh_result_batch_member")


def test_null_arguments_are_refused():
    lib = capi.load()
    info = capi.BatchMemberInfo(7, 7, 7, 7, 7, 7)
    assert lib.vh_result_batch_member(None, C.byref(info)) == VH_E_INVALID
    assert b"null argument" in lib.vh_last_error()
    assert [getattr(info, f) for f in FIELDS] == [7] * 6                        # (nothing is written on a refusal)
    assert lib.vh_result_batch_member(None, None) == VH_E_INVALID


def test_the_header_states_the_sharing_rule():
    m = re.search(r"/\* A batch of aggregates over ONE table.*?\*/\s*#define VH_BATCH_MAX", HEADER, re.S)
    assert m
    text = re.sub(r"\s*\n \* ?", " ", m.group(0))
    fusion = text[text.index("Fusion."):text.index("Failure is all-or-nothing")]
    assert "each member keeps its own filter" not in fusion
    for phrase in ("sharing rule", "both have a filter or both have none", "same projection F", "same literals", "VH_F_INSET",
                   "effective rows are equal in every segment", "one row fewer", "never spans launches", "scan_kernel_ms",
                   "vh_result_batch_member"):
        assert phrase in fusion, phrase
    assert re.search(r"changes neither a member's results nor its scan_kernel_ms", fusion)


def test_the_executor_carries_it_with_a_default():
    assert isinstance(executor.AggResult.batch_member, property) and executor.AggResult.batch_member.fset is None
    fields = dataclasses.fields(executor.AggResult)
    assert "batch_member" not in [f.name for f in fields]
    blank = {f.name: None for f in fields if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING}
    assert executor.AggResult(**blank).batch_member is None                     # a record built by hand
