"""The public surface of the row sink of the aggregate on the bit-sliced planes, as far as it can be checked without a GPU: include/viya_hip.h
defines VH_PLAN2_PLANE_ROWS as bit 1 of vh_plan.flags2 beside VH_PLAN2_PLANE_AGG, declares vh_result_plane_sink and says in the rule text what
both do; viyadb_amd/capi.py mirrors the constant and binds the symbol; the built library exports it and refuses null arguments; the executor
passes the flag through AggPlan.flags2 and carries the sink as a property with a default, no field of its own."""
import ctypes as C
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()
VH_E_INVALID = -1


def flat(text):
    return re.sub(r"\s*\n\s*\*? ?", " ", text)


def test_header_defines_the_flag_as_bit_1():
    m = re.search(r"enum\s+vh_plan_flags2\s*\{(.*?)\};", HEADER, re.S)
    assert m
    body = m.group(1)
    assert re.search(r"\bVH_PLAN2_PLANE_AGG\s*=\s*1u\s*<<\s*0\b", body) and re.search(r"\bVH_PLAN2_PLANE_ROWS\s*=\s*1u\s*<<\s*1\b", body)
    names = re.findall(r"\b(VH_PLAN2_\w+)\s*=", body)
    assert names == ["VH_PLAN2_PLANE_AGG", "VH_PLAN2_PLANE_ROWS"]
    said = flat(body[body.index("VH_PLAN2_PLANE_ROWS"):])
    for phrase in ("VH_PLAN2_PLANE_AGG", "64 group ids", "ROW SINK", "No environment variable", "sharded calls ignore it", "vh_result_plane_sink"):
        assert phrase in said, phrase


def test_header_rule_text_documents_flag_and_call():
    rule = flat(HEADER[HEADER.index("Aggregates on the bit-sliced planes. The readers above"):HEADER.index("#define VH_COL_ROWID")])
    for phrase in ("at most 64 group ids", "VH_PLAN2_PLANE_ROWS lifts that bound", "VH_PLANE_AGG=1 alone keeps it", "From 65 ids on the ROW SINK",
                   "no queue of row numbers", "once per row and metric", "bit 27 tells, whichever sink ran", "vh_result_plane_sink",
                   "1 the loop over ids, 2 the row sink"):
        assert phrase in rule, phrase
    assert re.search(r"VH_API\s+int\s+vh_result_plane_sink\s*\(\s*vh_result\*\s*r,\s*uint32_t\*\s*sink\s*\)", HEADER)
    batch = flat(re.search(r"/\* A batch of aggregates over ONE table.*?\*/\s*#define VH_BATCH_MAX", HEADER, re.S).group(0))
    fusion = batch[batch.index("Fusion."):batch.index("Failure is all-or-nothing")]
    for phrase in ("row sink", "VH_PLAN2_PLANE_ROWS", "candidate like any other", "scan_agg_planes_batch_kernel<256, S, rows>"):
        assert phrase in fusion, phrase


def test_capi_mirrors_flag_and_symbol():
    assert capi.PLAN2_PLANE_AGG == 1 << 0 and capi.PLAN2_PLANE_ROWS == 1 << 1
    plan2 = {n: v for n, v in vars(capi).items() if n.startswith("PLAN2_") and isinstance(v, int)}
    assert sorted(plan2.values()) == [1, 2]
    assert "vh_result_plane_sink" in capi.SYMBOLS
    restype, argtypes = capi.SYMBOLS["vh_result_plane_sink"]
    assert restype is C.c_int and len(argtypes) == 2 and argtypes[1] is C.POINTER(C.c_uint32)


def test_the_library_exports_the_symbol_and_refuses_null_arguments():
    import __graft_entry__ as g
    g.build()
    lib = capi.load()
    assert lib.vh_result_plane_sink.restype is C.c_int and len(lib.vh_result_plane_sink.argtypes) == 2
    raw = C.CDLL(lib._name)                                                     # the shared object itself exports it
    assert hasattr(raw, "vh_result_plane_sink")
    sink = C.c_uint32(7)
    assert lib.vh_result_plane_sink(None, C.byref(sink)) == VH_E_INVALID
    assert b"null argument" in lib.vh_last_error()
    assert sink.value == 7                                                      # (nothing is written on a refusal)
    assert lib.vh_result_plane_sink(None, None) == VH_E_INVALID


def test_the_executor_passes_the_flag_and_carries_the_sink_with_a_default():
    plan = executor.AggPlan(flags2=capi.PLAN2_PLANE_ROWS)
    assert plan.flags2 == 2 and dataclasses.replace(plan, flags2=capi.PLAN2_PLANE_AGG | capi.PLAN2_PLANE_ROWS).flags2 == 3
    p = capi.Plan()
    p.flags2 = capi.PLAN2_PLANE_ROWS
    assert p.flags2 == 2
    fields = dataclasses.fields(executor.AggResult)
    assert "plane_sink" not in [f.name for f in fields] and fields[-1].name == "sliced_prebuilt"
    assert isinstance(executor.AggResult.plane_sink, property) and executor.AggResult.plane_sink.fset is None
    blank = {f.name: None for f in fields if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING}
    assert executor.AggResult(**blank).plane_sink == 0                          # a record built by hand: no plane aggregate
