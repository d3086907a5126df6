"""The names of vh_result_info.reserved's bits, as far as they can be checked without a GPU: enum vh_info_bits of include/viya_hip.h, the
INFO_* constants of viyadb_amd/capi.py and the executor's table of AggResult's flag fields say the same thing, and the comment behind the
field tells every bit by its name."""
import dataclasses
import os
import re

from viyadb_amd import capi, executor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "viya_hip.h")).read()


def _enum():
    """name (without VH_) -> value, evaluated in order: the composites are ORs of enumerators before them."""
    body = re.search(r"enum\s+vh_info_bits\s*\{(.*?)\};", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = {}
    for item in body.split(","):
        name, expr = [x.strip() for x in item.split("=")]
        assert re.fullmatch(r"VH_INFO_[A-Z0-9_]+", name) and name[3:] not in out, name
        expr = re.sub(r"\bVH_(INFO_[A-Z0-9_]+)\b", lambda m: str(out[m.group(1)]), expr)
        assert re.fullmatch(r"[0-9u<| ]+", expr), (name, expr)
        out[name[3:]] = eval(expr.replace("u", ""))
    return out


ENUM = _enum()
SINGLE = {n: v for n, v in ENUM.items() if n != "INFO_REC_SHIFT" and bin(v).count("1") == 1}


def test_the_enum_is_in_front_of_the_struct_and_capi_has_the_same_names():
    assert re.search(r"enum\s+vh_info_bits\s*\{[^}]*\};\s*typedef struct vh_result_info \{", HEADER)
    infos = {n: v for n, v in vars(capi).items() if n.startswith("INFO_") and isinstance(v, int)}
    assert infos == ENUM
    assert len(SINGLE) == 27 and 1 << 9 not in ENUM.values() and 1 << 31 not in ENUM.values()
    assert ENUM["INFO_REC_SHIFT"] == 16 and ENUM["INFO_REC_MASK"] == 7 << 16
    assert ENUM["INFO_ON_PLANES"] == 1 << 4 | 1 << 11 | 1 << 13 and ENUM["INFO_PROJECTION"] == 1 << 3 | 1 << 7 | 1 << 15 | 7 << 16
    assert set(ENUM) == set(SINGLE) | {"INFO_REC_SHIFT", "INFO_REC_MASK", "INFO_ON_PLANES", "INFO_PROJECTION"}


def test_the_single_bits_are_disjoint():
    names = sorted(SINGLE)
    for i, a in enumerate(names):
        assert not SINGLE[a] & ENUM["INFO_REC_MASK"], a
        for b in names[i + 1:]:
            assert not SINGLE[a] & SINGLE[b], (a, b)


def test_the_comment_tells_every_bit_by_its_name_in_bit_order():
    info = re.search(r"uint32_t\s+reserved;\s*/\*(.*?)\*/", HEADER, re.S).group(1)
    for name, v in SINGLE.items():
        assert re.search(rf"\bbit {v.bit_length() - 1}: VH_{name}\b", info), name
    assert re.search(r"\bbits 16-18: VH_INFO_REC_MASK\b", info)
    told = [int(n) for n in re.findall(r"\bbits? (\d+)(?:-\d+)?: ", info)]
    assert told == sorted(told) and told == list(range(31)[:17]) + list(range(19, 31))
    assert "never set" in re.search(r"bit 9:(.*?)bit 10:", info, re.S).group(1) and "VH_INFO" not in re.search(r"bit 9:(.*?)bit 10:", info, re.S).group(1)


def test_every_flag_field_decodes_its_own_bit_and_no_other():
    fields = dataclasses.fields(executor.AggResult)
    table = executor.INFO_FIELDS
    assert set(table) == {f.name for f in fields if f.type in (bool, "bool")}
    assert len(set(table.values())) == len(table) and set(table.values()) <= set(SINGLE.values())
    for field, bit in table.items():       # the field is named after its enumerator, as far as the names go
        name = [n for n, v in SINGLE.items() if v == bit][0]
        assert name == "INFO_" + field.upper(), (field, name)
    blank = {f.name: None for f in fields if f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING}
    props = {"plane_agg": capi.INFO_PLANE_AGG, "batch_fused": capi.INFO_BATCH_FUSED, "sub_trimmed": capi.INFO_SUBTRIM, "gp_spanned": capi.INFO_GPSPAN}
    for name, c in SINGLE.items():
        res = executor.AggResult(**blank, flags=c, **executor.info_fields(c))
        assert {f for f in table if getattr(res, f)} == {f for f, bit in table.items() if bit == c}, name
        assert {p for p in props if getattr(res, p)} == {p for p, bit in props.items() if bit == c}, name
        assert res.flags == c
    everything = sum(SINGLE.values()) | 3 << capi.INFO_REC_SHIFT
    assert all(executor.info_fields(everything).values()) and not any(executor.info_fields(0).values())
    assert capi.info_rec_bytes(everything) == 16 and capi.info_rec_bytes(everything & ~capi.INFO_PACKED) == 0
