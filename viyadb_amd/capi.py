"""ctypes mirror of include/viya_hip.h — the C-ABI boundary of the aggregate path.

Nothing in here computes: it loads ``libviya_hip.so`` (built in-tree by
``viyadb_amd.build``) and exposes the structs/functions one to one.  There is no
CPU fallback: if the library is missing or a call fails, a ``VhError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VIYA_HIP_LIB") or os.path.join(_HERE, "libviya_hip.so")   # VIYA_HIP_LIB: a measurement build (tools/build_variant.py)

# enum vh_elem
U8, U16, U32, U64, I8, I16, I32, I64, F32, F64, BITSET32, BITSET64 = range(12)
ELEM_NAMES = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64", "bitset32", "bitset64"]
ELEM_NP = ["uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float32", "float64"]
ELEM_SIZE = [1, 2, 4, 8, 1, 2, 4, 8, 4, 8]
# enum vh_kind
DIM_STRING, DIM_NUMERIC, DIM_TIME, DIM_BOOLEAN = 0, 1, 2, 3
METRIC_MAX, METRIC_MIN, METRIC_SUM, METRIC_AVG, METRIC_COUNT, METRIC_BITSET, METRIC_HIDDEN_COUNT = 16, 17, 18, 19, 20, 21, 22
# enum vh_fkind / vh_relop
F_TRUE, F_REL, F_IN, F_AND, F_OR, F_INSET = range(6)
MAX_SETS = 4                      # VH_MAX_SETS: set leaves (F_INSET) per plan
PLAN_INLINE_LITS = 32             # VH_PLAN_INLINE_LITS
OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE = range(6)
# enum vh_time_unit
T_YEAR, T_MONTH, T_WEEK, T_DAY, T_HOUR, T_MINUTE, T_SECOND, T_NONE = range(8)
MAX_ROLLUP = 8
# plan flags
PLAN_FORCE_HASH, PLAN_FORCE_GLOBAL, PLAN_NO_XCD_PRIVATE, PLAN_NO_FAST, PLAN_NO_PART, PLAN_NO_CARRIER, PLAN_FORCE_PART = 1, 2, 4, 8, 16, 32, 64
PLAN_NO_LANES, PLAN_FORCE_LANES, PLAN_NO_LDS_HASH, PLAN_NO_HASH_RECORDS, PLAN_FORCE_HASH_RECORDS = 128, 256, 512, 1024, 2048
PLAN_NO_PACK, PLAN_FORCE_PACK, PLAN_NO_PART2, PLAN_NO_SHAPE, PLAN_NO_NARROW = 4096, 8192, 16384, 32768, 65536
PLAN_NO_JIT, PLAN_FORCE_JIT, PLAN_NO_HPART, PLAN_FORCE_HPART, PLAN_NO_HP_PACK, PLAN_CARD32, PLAN_NO_NARROW_TUPLES = 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22, 1 << 23
PLAN_NO_PREDPACK, PLAN_NO_QPAY, PLAN_FORCE_QPAY, PLAN_NO_SLICED = 1 << 24, 1 << 25, 1 << 26, 1 << 27
PLAN_NO_GROUPED = 1 << 28
PLAN_NO_GPLANES = 1 << 29
PLAN_SET_SEARCH = 1 << 30         # testing: every set of an F_INSET leaf takes the sorted-array form
PLAN_SLICED_PREBUILT = 1 << 31    # opt-in: an aggregate no compiled kernel answers reads its filter off the bit-sliced planes (scan_agg_sliced_kernel)
PLAN2_PLANE_AGG = 1 << 0          # vh_plan.flags2 (enum vh_plan_flags2). Opt-in: an aggregate of few groups is computed on the bit-sliced planes (scan_agg_planes_kernel)
PLAN2_PLANE_ROWS = 1 << 1         # ... the same, without the bound of 64 group ids: beyond it the row sink fills the table (scan_agg_planes_rows_kernel; vh_result_plane_sink)
# enum vh_plan_flags2_compiled, the header's second enum of vh_plan.flags2 bits. The module's own PLAN2_* names are enum vh_plan_flags2's and
# nothing else (tests/test_capi_plane_rows.py holds vars(capi) to those two), so the bits of the second enum are served by name through the
# module's __getattr__ below: capi.PLAN2_PLANE_JIT and `from viyadb_amd.capi import PLAN2_PLANE_JIT` both work.
_PLAN2_COMPILED = {"PLAN2_PLANE_JIT": 1 << 2}      # ... PLAN2_PLANE_AGG, by a kernel compiled for the plan's shape wherever a compiled kernel may run the query (bits 27 and 5; VH_PLANE_JIT=1)


def __getattr__(name):
    if name in _PLAN2_COMPILED:
        return _PLAN2_COMPILED[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# paths
PATH_SCALAR, PATH_DENSE_LDS, PATH_DENSE_GLOBAL, PATH_HASH, PATH_DENSE_PART = range(5)
PATH_NAMES = ["scalar", "dense_lds", "dense_global", "hash", "dense_part"]
# generator
GEN_UNIFORM, GEN_ROWID, GEN_CONST, GEN_ZIPF, GEN_SORTED, GEN_HOT = range(6)


class ColDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("elem", C.c_int32)]


class AnyNum(C.Union):
    _fields_ = [("u8", C.c_uint8), ("u16", C.c_uint16), ("u32", C.c_uint32), ("u64", C.c_uint64),
                ("i8", C.c_int8), ("i16", C.c_int16), ("i32", C.c_int32), ("i64", C.c_int64),
                ("f32", C.c_float), ("f64", C.c_double)]


class FilterNode(C.Structure):
    _fields_ = [("kind", C.c_int32), ("col", C.c_int32), ("op", C.c_int32), ("count", C.c_int32),
                ("lit", C.c_int32), ("reserved", C.c_int32)]


class GroupCol(C.Structure):
    _fields_ = [("col", C.c_int32), ("granularity", C.c_int32), ("nrollup", C.c_int32),
                ("rollup_unit", C.c_int32 * MAX_ROLLUP), ("rollup_before", C.c_uint64 * MAX_ROLLUP),
                ("micro", C.c_int32), ("reserved", C.c_int32), ("cardinality", C.c_uint64)]


class Plan(C.Structure):
    _fields_ = [("filter", C.POINTER(FilterNode)), ("nfilter", C.c_int32),
                ("lits", C.POINTER(AnyNum)), ("nlits", C.c_int32),
                ("groups", C.POINTER(GroupCol)), ("ngroups", C.c_int32),
                ("metrics", C.POINTER(C.c_int32)), ("nmetrics", C.c_int32),
                ("seg_rows", C.POINTER(C.c_uint64)), ("nseg", C.c_uint32),
                ("flags", C.c_uint32), ("groups_hint", C.c_uint64),
                ("having", C.POINTER(FilterNode)), ("nhaving", C.c_int32), ("flags2", C.c_uint32),
                ("top_col", C.c_int32), ("top_desc", C.c_int32), ("top_k", C.c_uint64)]


class ResultInfo(C.Structure):
    _fields_ = [("ngroups", C.c_uint64), ("scanned_recs", C.c_uint64), ("scanned_segments", C.c_uint64),
                ("passed_recs", C.c_uint64), ("path", C.c_int32), ("ngroup_cols", C.c_int32),
                ("nmetrics", C.c_int32), ("has_hidden_count", C.c_int32), ("scan_kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("algorithmic_bytes", C.c_uint64), ("retries", C.c_uint32),
                ("reserved", C.c_uint32), ("returned_groups", C.c_uint64)]


TAIL_NONE, TAIL_FUSED, TAIL_EMIT2, TAIL_EMIT16 = range(4)      # enum vh_tail_kind
TAIL_KIND_NAMES = ["none", "fused", "emit2", "emit16"]
MERGE_NONE, MERGE_KERNEL, MERGE_FUSED = range(3)                # enum vh_tail_merge


class TailInfo(C.Structure):
    """vh_tail_info: which kernels ended the query (vh_result_tail)."""
    _fields_ = [("kind", C.c_int32), ("direct", C.c_int32), ("merged", C.c_int32), ("copies", C.c_int32),
                ("entries", C.c_uint64), ("states_per_entry", C.c_uint32), ("reserved", C.c_uint32), ("region_bytes", C.c_uint64)]


class SelectPlan(C.Structure):
    _fields_ = [("filter", C.POINTER(FilterNode)), ("nfilter", C.c_int32),
                ("lits", C.POINTER(AnyNum)), ("nlits", C.c_int32),
                ("cols", C.POINTER(C.c_int32)), ("ncols", C.c_int32),
                ("seg_rows", C.POINTER(C.c_uint64)), ("nseg", C.c_uint32),
                ("flags", C.c_uint32), ("skip", C.c_uint64), ("limit", C.c_uint64)]


class RowsInfo(C.Structure):
    _fields_ = [("nrows", C.c_uint64), ("scanned_recs", C.c_uint64), ("scanned_segments", C.c_uint64),
                ("passed_recs", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float)]


COL_ROWID = -2


class DeviceBuffer(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("count", C.c_uint64), ("elem", C.c_int32), ("reduce", C.c_int32)]


class CommInfo(C.Structure):
    """vh_comm_info_t: the communicator as the transport itself reports it."""
    _fields_ = [("transport", C.c_int32), ("nranks", C.c_int32), ("rank", C.c_int32), ("device", C.c_int32), ("pci_bus_id", C.c_char * 32)]


COMM_RCCL, COMM_CALLBACKS = 1, 2


class SyncItem(C.Structure):
    """vh_sync_item: one contiguous row range of one segment (vh_table_sync_batch)."""
    _fields_ = [("seg", C.c_uint32), ("flags", C.c_uint32), ("row_first", C.c_uint64), ("nrows", C.c_uint64),
                ("new_size", C.c_uint64), ("col_ptrs", C.POINTER(C.c_void_p))]


SYNC_METRICS_ONLY, SYNC_DEVICE_SRC = 1, 2


class GenSpec(C.Structure):
    _fields_ = [("mode", C.c_int32), ("param", C.c_int32), ("mod", C.c_uint64), ("add", C.c_int64),
                ("scale", C.c_double)]


class CommOps(C.Structure):
    """vh_comm_ops: a transport as a table of callbacks (tests: gloo; see viyadb_amd/distributed.py)."""
    ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)
    REDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p)
    ALLTOALLV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p)
    _fields_ = [("ctx", C.c_void_p), ("allgather_host", ALLGATHER), ("reduce_device", REDUCE), ("alltoallv_device", ALLTOALLV)]


COMM_ID_BYTES = 128

BUILD_INLINE, BUILD_BACKGROUND = 0, 1
# enum vh_info_bits: what ran, one name per bit of vh_result_info.reserved (include/viya_hip.h tells each bit's meaning at the field)
INFO_FAST = 1 << 0                # the register-resident fast scan kernel ran
INFO_LANES = 1 << 1               # ... its no-compaction "lanes" variant
INFO_LDS_HASH = 1 << 2            # LDS front table of the hash path
INFO_PACKED = 1 << 3              # group / metric values came from a payload projection
INFO_NARROW = 1 << 4              # predicate columns streamed from narrow copies
INFO_JIT = 1 << 5                 # a scan kernel compiled for this plan shape ran
INFO_HPART = 1 << 6               # hashed partitioning of the hash path
INFO_PACKED_COMPRESSED = 1 << 7   # the projection's records are compressed
INFO_HP_PACKED = 1 << 8           # the hashed partitioning's tuples were packed (bit 9 is never set)
INFO_TUPLE1 = 1 << 10             # DENSE_PART wrote one-word tuples
INFO_PREDPACK = 1 << 11           # predicate columns streamed as byte planes of a bit-packed predicate projection (bit 4 is set too)
INFO_STREAMED_PAYLOAD = 1 << 12   # the payload was streamed beside the predicate columns, not gathered (bits 3 and 7 are set too)
INFO_SLICED = 1 << 13             # ... of the predicate projection's bit-sliced form
INFO_TUPLE4 = 1 << 14             # DENSE_PART's one-word tuples were four bytes (bit 10 is set too)
INFO_PACK_BITS = 1 << 15          # the projection's records are bit fields (bits 3 and 7 are set too)
INFO_REC_SHIFT = 16               # bits 16-18: log2 of the projection's record bytes, less one (info_rec_bytes)
INFO_REC_MASK = 7 << 16
INFO_BUILD_PENDING = 1 << 19      # a kernel compile or a layout build for this query's shape is queued or running (BUILD_BACKGROUND tables)
INFO_GROUPED_PAYLOAD = 1 << 20    # the payload records were gathered from the projection's grouped form
INFO_GROUPED_PLANES = 1 << 21     # ... and the predicate bits read from the planes clustered in the same order (bit 20 is set too)
INFO_INSET = 1 << 22              # the filter's set leaves were evaluated by lookup
INFO_INSET_SEARCH = 1 << 23       # ... at least one of them by binary search in a sorted array
INFO_EVICTED = 1 << 24            # planning this query evicted at least one derived layout (tables with a layout budget)
INFO_INSET_SLICED = 1 << 25       # ... all of the set leaves from truth tables on the bit-sliced predicate planes instead (no lookup per row)
INFO_SLICED_PREBUILT = 1 << 26    # a pre-built scan read the filter off the bit-sliced predicate planes (bits 4, 11 and 13 are set too)
INFO_PLANE_AGG = 1 << 27          # the aggregate was computed on the bit-sliced planes (bits 4, 11 and 13 are set too; bits 0, 1 and 26 are clear, and so is bit 5 unless the kernel was compiled for the plan: PLAN2_PLANE_JIT)
INFO_SUBTRIM = 1 << 28            # the clustered planes are a sub-sorted form's and every run was trimmed by the sub column's leaf (bits 20 and 21 are set too)
INFO_GPSPAN = 1 << 29             # the clustered scan's tile groups spanned segments, its queue held table-wide record indexes (bits 20 and 21 are set too)
INFO_BATCH_FUSED = 1 << 30        # the result was filled by a fused launch of a batch (vh_query_agg_batch; bit 27 and its company are set too)
INFO_ON_PLANES = INFO_NARROW | INFO_PREDPACK | INFO_SLICED      # the filter was read off the bit-sliced predicate planes
INFO_PROJECTION = INFO_PACKED | INFO_PACKED_COMPRESSED | INFO_PACK_BITS | INFO_REC_MASK      # everything that describes a payload projection


def info_rec_bytes(flags: int) -> int:
    """Bytes of one projection record (0: no projection was read)."""
    return 2 << ((flags & INFO_REC_MASK) >> INFO_REC_SHIFT) if flags & INFO_PACKED else 0


BATCH_MAX = 8                     # VH_BATCH_MAX: members of one vh_query_agg_batch call


class BatchInfo(C.Structure):
    """vh_batch_info: how a batch was answered. fused_kernel_ms is the sum over the fused launches."""
    _fields_ = [("nplans", C.c_uint32), ("fused_groups", C.c_uint32), ("fused_members", C.c_uint32), ("singles", C.c_uint32),
                ("fused_kernel_ms", C.c_float), ("reserved", C.c_uint32)]

    @property
    def compiled_groups(self) -> int:
        """How many of fused_groups were compiled fused launches: PLAN2_PLANE_JIT members answered by one kernel compiled for their batch
        shape (the C field keeps its name, `reserved`)."""
        return int(self.reserved)


class BatchMemberInfo(C.Structure):
    """vh_batch_member_info: a result's place in a fused launch of a batch and whose pass mask it used (vh_result_batch_member). All zeros
    outside a fused launch."""
    _fields_ = [("fused", C.c_uint32), ("launch", C.c_uint32), ("position", C.c_uint32), ("members", C.c_uint32),
                ("mask_of", C.c_uint32), ("mask_classes", C.c_uint32)]


class BuildInfo(C.Structure):
    """vh_build_info: what the background build worker did for one table."""
    _fields_ = [("jobs_queued", C.c_uint64), ("jobs_running", C.c_uint64), ("jobs_done", C.c_uint64),
                ("jobs_failed", C.c_uint64), ("jobs_cancelled", C.c_uint64), ("kernels_compiled", C.c_uint64),
                ("kernels_cached", C.c_uint64), ("layouts_built", C.c_uint64), ("inline_builds", C.c_uint64),
                ("compile_ms", C.c_double), ("layout_ms", C.c_double), ("lock_ms", C.c_double),
                ("jobs_declined", C.c_uint64), ("layout_restarts", C.c_uint64), ("warm_queries", C.c_uint64), ("warm_ms", C.c_double)]


LAYOUT_PROJECTION, LAYOUT_PRED_BYTES, LAYOUT_PRED_SLICED, LAYOUT_NARROW = 1, 2, 3, 4      # enum vh_layout_kind
LAYOUT_COLS = 32                  # VH_LAYOUT_COLS
# vh_layout_info.flags
LAYOUT_AUTOMATIC, LAYOUT_PINNED, LAYOUT_CURRENT, LAYOUT_COMPRESSED, LAYOUT_BITS, LAYOUT_GROUPED, LAYOUT_GPLANES = 1, 2, 4, 8, 16, 32, 64


class LayoutInfo(C.Structure):
    """vh_layout_info: one derived layout of a table (vh_table_layouts)."""
    _fields_ = [("serial", C.c_uint64), ("kind", C.c_int32), ("ncols", C.c_int32), ("cols", C.c_int32 * LAYOUT_COLS),
                ("bytes", C.c_uint64), ("grouped_bytes", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("uses", C.c_uint64), ("last_use", C.c_uint64)]


class LayoutSummary(C.Structure):
    """vh_layout_summary: bytes + reserved_bytes is the figure the budget bounds."""
    _fields_ = [("budget", C.c_uint64), ("bytes", C.c_uint64), ("pinned_bytes", C.c_uint64), ("reserved_bytes", C.c_uint64),
                ("tick", C.c_uint64), ("evictions", C.c_uint64), ("evicted_bytes", C.c_uint64), ("declined", C.c_uint64)]



class VhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"viya_hip error {code}: {msg}")
        self.code = code


# every symbol include/viya_hip.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "vh_init": (C.c_int, [C.c_int]),
    "vh_set_stream": (C.c_int, [_VP]),
    "vh_last_error": (C.c_char_p, []),
    "vh_version": (C.c_char_p, []),
    "vh_table_create": (C.c_int, [C.POINTER(ColDesc), C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(_VP)]),
    "vh_table_destroy": (None, [_VP]),
    "vh_segment_sync": (C.c_int, [_VP, C.c_uint32, C.c_uint64, C.POINTER(_VP)]),
    "vh_segment_sync_range": (C.c_int, [_VP, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_VP)]),
    "vh_table_sync_batch": (C.c_int, [_VP, C.POINTER(SyncItem), C.c_uint32]),
    "vh_host_register": (C.c_int, [_VP, C.c_uint64]),
    "vh_host_unregister": (C.c_int, [_VP]),
    "vh_table_sync_stats": (C.c_int, [_VP] + [C.POINTER(C.c_uint64)] * 5),
    "vh_segment_sync_bitset": (C.c_int, [_VP, C.c_uint32, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64), _VP]),
    "vh_segment_generate": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(GenSpec), C.c_uint64]),
    "vh_table_pack": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int32]),
    "vh_table_pack_ex": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int32, C.c_uint32]),
    "vh_table_unpack": (C.c_int, [_VP]),
    "vh_table_relocate": (C.c_int, [_VP, C.c_uint32]),
    "vh_table_narrow": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int32]),
    "vh_table_predpack": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int32]),
    "vh_table_predpack_ex": (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int32, C.c_uint32]),
    "vh_segment_read": (C.c_int, [_VP, C.c_uint32, C.c_int32, C.c_uint64, _VP]),
    "vh_device_read": (C.c_int, [_VP, _VP, C.c_uint64]),
    "vh_table_info": (C.c_int, [_VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vh_table_set_layout_budget": (C.c_int, [_VP, C.c_uint64]),
    "vh_table_layouts": (C.c_int, [_VP, C.POINTER(LayoutInfo), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(LayoutSummary)]),
    "vh_table_layout_pin": (C.c_int, [_VP, C.c_uint64, C.c_int32]),
    "vh_table_layout_drop": (C.c_int, [_VP, C.c_uint64]),
    "vh_segment_stats": (C.c_int, [_VP, C.c_uint32, C.c_int32, C.POINTER(AnyNum), C.POINTER(AnyNum)]),
    "vh_query_agg": (C.c_int, [_VP, C.POINTER(Plan), C.POINTER(_VP)]),
    "vh_query_agg_batch": (C.c_int, [_VP, C.POINTER(C.POINTER(Plan)), C.c_uint32, C.POINTER(_VP), C.POINTER(BatchInfo)]),
    "vh_query_launch": (C.c_int, [_VP, C.POINTER(Plan), C.POINTER(_VP)]),
    "vh_result_device_buffers": (C.c_int, [_VP, C.POINTER(DeviceBuffer), C.c_int32, C.POINTER(C.c_int32)]),
    "vh_result_finalize": (C.c_int, [_VP]),
    "vh_result_partition": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(DeviceBuffer), C.c_int32, C.POINTER(C.c_int32)]),
    "vh_result_partition_pairs": (C.c_int, [_VP, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(DeviceBuffer), C.c_int32, C.POINTER(C.c_int32)]),
    "vh_segment_sync_ids_device": (C.c_int, [_VP, C.c_uint32, C.c_int32, C.c_uint64, _VP]),
    "vh_comm_unique_id": (C.c_int, [_VP]),
    "vh_comm_init": (C.c_int, [_VP, C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "vh_comm_init_custom": (C.c_int, [C.POINTER(CommOps), C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "vh_comm_destroy": (None, [_VP]),
    "vh_comm_info": (C.c_int, [_VP, C.POINTER(CommInfo)]),
    "vh_comm_allgather_host": (C.c_int, [_VP, _VP, _VP, C.c_uint64]),
    "vh_query_agg_sharded": (C.c_int, [_VP, C.POINTER(Plan), _VP, C.c_int32, C.POINTER(_VP)]),
    "vh_query_select": (C.c_int, [_VP, C.POINTER(SelectPlan), C.POINTER(_VP)]),
    "vh_query_select_sharded": (C.c_int, [_VP, C.POINTER(SelectPlan), _VP, C.c_int32, C.POINTER(_VP)]),
    "vh_rows_get_info": (C.c_int, [_VP, C.POINTER(RowsInfo)]),
    "vh_rows_flags": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "vh_rows_view": (C.c_int, [_VP, C.POINTER(_VP)]),
    "vh_rows_free": (None, [_VP]),
    "vh_result_get_info": (C.c_int, [_VP, C.POINTER(ResultInfo)]),
    "vh_table_prepare": (C.c_int, [_VP, C.POINTER(Plan), C.POINTER(ResultInfo)]),
    "vh_table_set_build_mode": (C.c_int, [_VP, C.c_int32]),
    "vh_table_build_wait": (C.c_int, [_VP, C.c_uint32, C.POINTER(BuildInfo)]),
    "vh_table_build_info": (C.c_int, [_VP, C.POINTER(BuildInfo)]),
    "vh_result_kernel": (C.c_char_p, [_VP]),
    "vh_result_tail": (C.c_int, [_VP, C.POINTER(TailInfo)]),
    "vh_result_batch_member": (C.c_int, [_VP, C.POINTER(BatchMemberInfo)]),
    "vh_result_plane_sink": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "vh_result_state_elem": (C.c_int, [_VP, C.c_int32]),
    "vh_result_copy": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    "vh_result_view": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(C.POINTER(C.c_uint64))]),
    "vh_result_free": (None, [_VP]),
    "vh_measure_read_bandwidth": (C.c_int, [C.c_uint64, C.c_int32, C.POINTER(C.c_double)]),
    "vh_jit_selftest": (C.c_int, [C.c_int32, C.c_char_p, C.c_char_p, C.c_uint64]),
    "vh_jit_selftest_name": (C.c_int, [C.c_int32, C.c_char_p, C.c_uint64]),
    "vh_jit_selftest_key": (C.c_int, [C.c_int32, C.c_char_p, C.c_uint64]),
}

_lib = None


def load():
    """dlopen the in-tree HIP library and type its entry points. Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VhError(-100, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback for the aggregate path)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VhError(rc, load().vh_last_error().decode("utf-8", "replace"))
