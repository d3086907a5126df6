"""The public surface of the pre-built aggregate scan over the bit-sliced predicate planes, as far as it can be checked without a GPU:
include/viya_hip.h defines VH_PLAN_SLICED_PREBUILT as the one free flag bit and documents vh_result_info.reserved bit 26; the constants
of viyadb_amd/capi.py equal them; the flag collides with no other plan flag; the result record of the executor carries the new field last."""
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()


def test_header_defines_the_flag_and_documents_the_bit():
    m = re.search(r"\bVH_PLAN_SLICED_PREBUILT\s*=\s*1u\s*<<\s*(\d+)\s*,", HEADER)
    assert m and int(m.group(1)) == 31
    info = re.search(r"uint32_t\s+reserved;\s*/\*(.*?)\*/", HEADER, re.S).group(1)
    bit26 = re.search(r"bit 26:(.*?)(?:bit \d+:|$)", info, re.S)
    assert bit26 and "bit-sliced" in bit26.group(1) and "VH_PLAN_SLICED_PREBUILT" in bit26.group(1)
    assert "VH_SLICED_PREBUILT=1" in HEADER                     # the environment switch is documented beside the rule


def test_capi_constants_equal_the_header():
    assert capi.PLAN_SLICED_PREBUILT == 1 << 31
    assert capi.INFO_SLICED_PREBUILT == 1 << 26
    flags = {name: int(shift) for name, shift in re.findall(r"\b(VH_PLAN_[A-Z0-9_]+)\s*=\s*1u\s*<<\s*(\d+)", HEADER)}
    assert flags["VH_PLAN_SLICED_PREBUILT"] == 31
    for name, shift in flags.items():                           # every flag the header defines by a shift that capi mirrors has the same value there
        mirror = getattr(capi, name[3:], None)
        assert mirror is None or mirror == 1 << shift, (name, mirror, shift)


def test_the_flag_collides_with_no_other_plan_flag():
    plans = {n: v for n, v in vars(capi).items() if n.startswith("PLAN_") and isinstance(v, int) and n not in ("PLAN_INLINE_LITS",)}
    assert "PLAN_SLICED_PREBUILT" in plans
    for name, value in plans.items():
        assert value > 0 and value & (value - 1) == 0, (name, value)       # one bit each
        assert name == "PLAN_SLICED_PREBUILT" or value != capi.PLAN_SLICED_PREBUILT, name
    assert len(set(plans.values())) == len(plans)
    assert capi.PLAN_SLICED_PREBUILT < 1 << 32                  # vh_plan::flags is a uint32_t


def test_the_result_record_ends_with_the_new_field():
    fields = dataclasses.fields(executor.AggResult)
    assert fields[-1].name == "sliced_prebuilt" and fields[-1].default is False
