// vhh_info.h — vh_result_info.reserved, the record of which path answered a query, put together in one place from the facts the planner
// settled on. Plain C++ with no HIP in it, like vhh_layout_math.h: the library includes it (vhh_plan.h, vhh_launch.h) and
// tests/info_bits_host.cc compiles it with g++ under UBSan and checks every combination against the numerals the bits had before
// they had names (enum vh_info_bits, include/viya_hip.h).
#pragma once
#include <cstdint>
#include <algorithm>
#include "../../include/viya_hip.h"

// What QueryBuild::launch() knows when everything is enqueued up to the scan.
struct VhWhatRan {
  bool hpart = false;                                   // hashed partitioning of the hash path
  bool fast = false, fastj = false, jk = false;         // a register-resident scan (fastj || jk); pre-built or compiled; a compiled kernel
  bool lanes = false, lds_hash = false;
  bool packed = false, packed_compressed = false, packed_bits = false;      // the payload projection and its records' form ...
  uint32_t packed_rec = 0;                                                  // ... and bytes
  bool narrowed = false;                                // a predicate column is read at another width than its type's
  bool hp_pack = false;
  bool dense_part = false, gid_bits = false, tuple4 = false;                // DENSE_PART; its tuples are one word; of four bytes
  bool pp_planes = false, pp_sliced = false, qpay = false;                  // the compiled kernel's shape: byte planes, bit-sliced planes, streamed payload
  bool has_set = false, set_search = false, set_truth = false;
  bool build_pending = false;
  bool grouped = false, gplanes = false, subtrim = false, gpspan = false;
  bool sliced_prebuilt = false, plane_agg = false;      // the two pre-built readers of the bit-sliced planes
  bool plane_jit = false;                               // ... the second of them in its compiled form (VH_PLAN2_PLANE_JIT): plane_agg is set too
};

// The word of a query that planned a scan.
static inline uint32_t vh_info_compose(const VhWhatRan& w) {
  const bool one_word = w.dense_part && w.gid_bits, clustered = w.jk && w.grouped && w.gplanes;
  uint32_t bits = (w.hpart ? VH_INFO_HPART : 0u)
                | (w.fast ? VH_INFO_FAST : 0u)
                | (w.lanes ? VH_INFO_LANES : 0u)
                | (w.lds_hash ? VH_INFO_LDS_HASH : 0u)
                | (w.packed ? VH_INFO_PACKED : 0u)
                | (w.fastj && w.narrowed ? VH_INFO_NARROW : 0u)
                | (w.jk ? VH_INFO_JIT : 0u)
                | (w.packed && w.packed_compressed ? VH_INFO_PACKED_COMPRESSED : 0u)
                | (w.hpart && w.hp_pack ? VH_INFO_HP_PACKED : 0u)
                | (one_word ? VH_INFO_TUPLE1 : 0u)
                | (w.jk && (w.pp_planes || w.pp_sliced) ? VH_INFO_PREDPACK : 0u)
                | (w.jk && w.qpay ? VH_INFO_STREAMED_PAYLOAD : 0u)
                | (w.jk && w.pp_sliced ? VH_INFO_SLICED : 0u)
                | (one_word && w.tuple4 ? VH_INFO_TUPLE4 : 0u)
                | (w.has_set ? VH_INFO_INSET : 0u)
                | (w.has_set && w.set_search ? VH_INFO_INSET_SEARCH : 0u)
                | (w.jk && w.has_set && w.set_truth && w.pp_sliced ? VH_INFO_INSET_SLICED : 0u)
                | (w.build_pending ? VH_INFO_BUILD_PENDING : 0u)
                | (w.jk && w.grouped ? VH_INFO_GROUPED_PAYLOAD : 0u)
                | (clustered ? VH_INFO_GROUPED_PLANES : 0u)
                | (clustered && w.subtrim ? VH_INFO_SUBTRIM : 0u)
                | (clustered && w.gpspan ? VH_INFO_GPSPAN : 0u)
                | (w.packed && w.packed_bits ? VH_INFO_PACK_BITS : 0u)
                | (w.packed ? (uint32_t)(31 - __builtin_clz(std::max<uint32_t>(w.packed_rec, 2)) - 1) << VH_INFO_REC_SHIFT : 0u);
  // a pre-built reader of the bit-sliced planes reports a predicate projection's bit-sliced form (and the sets' truth tables), and no
  // register-resident, lanes or compiled kernel
  const uint32_t on_planes = VH_INFO_ON_PLANES | (w.has_set ? VH_INFO_INSET | VH_INFO_INSET_SLICED : 0u);
  const uint32_t no_reader = VH_INFO_FAST | VH_INFO_LANES | VH_INFO_JIT;
  if (w.sliced_prebuilt) bits = (bits & ~no_reader) | VH_INFO_SLICED_PREBUILT | on_planes;
  // the plane aggregate reports no projection — it gathers no payload, whatever choose_projection had found — and is not the pre-built scan
  if (w.plane_agg) bits = (bits & ~(no_reader | VH_INFO_SLICED_PREBUILT | VH_INFO_PROJECTION)) | VH_INFO_PLANE_AGG | on_planes;
  // ... whose compiled form is a compiled kernel all the same: bit 27's word plus bit 5
  if (w.plane_agg && w.plane_jit) bits |= VH_INFO_JIT;
  return bits;
}

// The word of a select (vh_rows_flags): the filter read off the bit-sliced planes, or evaluated by the interpreting kernels.
static inline uint32_t vh_info_select(bool sliced, bool has_set, bool set_search) {
  if (sliced) return VH_INFO_ON_PLANES | (has_set ? VH_INFO_INSET | VH_INFO_INSET_SLICED : 0u);
  return has_set ? VH_INFO_INSET | (set_search ? VH_INFO_INSET_SEARCH : 0u) : 0u;
}

// Bytes of one projection record (0: no projection was read).
inline uint32_t vh_info_rec_bytes(uint32_t bits) {
  return bits & VH_INFO_PACKED ? 2u << ((bits & VH_INFO_REC_MASK) >> VH_INFO_REC_SHIFT) : 0u;
}
