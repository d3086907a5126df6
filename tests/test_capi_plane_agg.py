"""The public surface of the aggregate on the bit-sliced planes, as far as it can be checked without a GPU: include/viya_hip.h defines
VH_PLAN2_PLANE_AGG in vh_plan.flags2 (every bit of `flags` is taken) and documents vh_result_info.reserved bit 27 behind bit 26; the constants
of viyadb_amd/capi.py equal them; capi.Plan has flags2 where reserved2 was; the executor passes it through and adds no field to its result."""
import ctypes
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()


def test_header_defines_the_flag_and_documents_the_bit():
    m = re.search(r"enum\s+vh_plan_flags2\s*\{(.*?)\};", HEADER, re.S)
    assert m and re.search(r"\bVH_PLAN2_PLANE_AGG\s*=\s*1u\s*<<\s*0\b", m.group(1))
    assert re.search(r"int32_t\s+nhaving;\s*uint32_t\s+flags2;", HEADER) and "reserved2" not in HEADER
    info = re.search(r"uint32_t\s+reserved;\s*/\*(.*?)\*/", HEADER, re.S).group(1)
    assert info.index("bit 26:") < info.index("bit 27:")          # appended behind bit 26's text
    bit27 = re.search(r"bit 27:(.*?)(?:bit \d+:|$)", info, re.S).group(1)
    assert "bit-sliced" in bit27 and "VH_PLAN2_PLANE_AGG" in bit27
    assert "VH_PLANE_AGG=1" in HEADER and "Aggregates on the bit-sliced planes" in HEADER      # the switch and the rule


def test_capi_constants_equal_the_header():
    assert capi.PLAN2_PLANE_AGG == 1 << 0
    assert capi.INFO_PLANE_AGG == 1 << 27
    infos = {n: v for n, v in vars(capi).items() if n.startswith("INFO_") and isinstance(v, int)}
    assert [n for n, v in infos.items() if v == capi.INFO_PLANE_AGG] == ["INFO_PLANE_AGG"]


def test_plan_has_flags2_where_reserved2_was():
    names = [f[0] for f in capi.Plan._fields_]
    assert "reserved2" not in names and names[names.index("nhaving") + 1] == "flags2"
    assert capi.Plan.flags2.size == 4
    assert capi.Plan.flags2.offset == capi.Plan.nhaving.offset + 4       # the same four bytes
    assert capi.Plan.top_col.offset == capi.Plan.flags2.offset + 4       # ... and nothing behind them moved
    p = capi.Plan()
    p.flags2 = 0xFFFFFFFF
    assert p.flags2 == 0xFFFFFFFF                                        # unsigned, all 32 bits
    assert ctypes.sizeof(capi.Plan) % 8 == 0


def test_the_executor_passes_flags2_and_adds_no_result_field():
    assert {f.name: f.default for f in dataclasses.fields(executor.AggPlan)}["flags2"] == 0
    fields = dataclasses.fields(executor.AggResult)
    assert fields[-1].name == "sliced_prebuilt" and "plane_agg" not in [f.name for f in fields]
    assert isinstance(executor.AggResult.plane_agg, property) and executor.AggResult.plane_agg.fset is None
    blank = {f.name: None for f in fields if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING}
    assert executor.AggResult(**blank, flags=capi.INFO_PLANE_AGG).plane_agg is True
    assert executor.AggResult(**blank, flags=capi.INFO_SLICED_PREBUILT).plane_agg is False
