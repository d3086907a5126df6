// vh_sliced.h — what the PRE-BUILT readers of the bit-sliced predicate planes share on the device: the kernel arguments that name the planes
// and carry the filter program (vh_bits_eval.h), and a lane's pass mask for its word of a chunk (vh_sliced_walk.h). Included by the select
// kernels (vh_small_kernels.h), by the aggregate scan over the planes (vh_scan_sliced.hip) and by the one that also aggregates on them
// (vh_scan_planes.hip) and its form for a fused batch (vh_scan_planes_batch.hip).
#pragma once
#include "vh_internal.h"
#include "vh_bits_eval.h"
#include "vh_sliced_walk.h"

static_assert(VH_BITS_MAX_PROG == VH_INLINE_PROG && VH_BITS_MAX_LITS == VH_INLINE_LITS, "vh_bits_eval.h restates the inline program's budget");
// Where a projection's planes lie. Kernel argument: 32- and 64-bit members only (VH_PACKED_FIELD, vh_internal.h).
struct VhSlicedPlanes {
  const char* planes;             // the projection's arena: segment 0, plane 0
  uint64_t stride, pitch;         // bytes between segments / between planes
};
// The select kernels' argument: the program travels by value.
struct VhSlicedArgs {
  VhBitsProg B;
  VhSlicedPlanes L;
  const uint32_t* seg_rows;       // per segment: rows to scan (0 = skipped)
  unsigned long long* counters;   // [0] passed rows
  uint32_t nseg, pad;
};
// The aggregate scan's second argument, beside VhPlanDev (which names snapshot and counters): plan and program together would pass the 4 KB
// of kernel arguments (VhPlanDev alone is 3.9 KB), so the program lies in the query's uploaded plan block, behind the sets, and is read
// through this pointer. The launcher hands the kernel the pointer as a `__restrict__` parameter of its own and the planes by value: only
// then does the compiler know the program for unclobbered and read it with scalar loads (inside a by-value struct it took vector loads, a
// round trip per program word and chunk).
struct VhSlicedRef {
  const VhBitsProg* B;
  VhSlicedPlanes L;
};
// The aggregate scan ON the planes (vh_scan_planes.hip: scan_agg_planes_kernel) reads two projections: F, whose fields the filter program
// compares, and V, which holds every group column and every metric's source column (V may be F). Where their fields lie in V is this
// descriptor's; it follows the program in the plan block and is passed as a restrict pointer of its own, for the reason given above.
#define VH_PLANE_AGG_MAX_GROUPS 64      // group ids of a plan that takes the loop over ids, which is paid per plane word; beyond: the row sink, where asked for
struct VhPlaneAggDesc {
  uint32_t has_filter;            // 0: no program, every row of the snapshot passes
  uint32_t need;                  // bit p: plane p of V belongs to a group column's or a metric's field (the others are not read)
  uint32_t care;                  // bit p: ... to a group column's
  uint32_t rows;                  // 1: the row sink (vh_plane_agg.h: vh_plane_agg_rows) — more than VH_PLANE_AGG_MAX_GROUPS ids; valid and pat are unused then
  uint64_t valid;                // bit g: every group column's value of id g lies within its field (else no row can belong to g)
  uint32_t pat[VH_PLANE_AGG_MAX_GROUPS];      // id g: the group columns' values (VhGroupDev::lo + digit) at their fields' places (vh_bits_match)
  uint32_t goff[VH_MAX_GROUP], gbits[VH_MAX_GROUP];       // group column i: first plane and planes of its field in V (what pat and care were made of)
  uint32_t moff[VH_MAX_METRIC], mbits[VH_MAX_METRIC];     // metric j (VhPlanDev::m[j], the hidden count included): ... of its source column's field
};
struct VhPlaneAggRef {
  const VhBitsProg* B;            // nullptr: no filter
  const VhPlaneAggDesc* D;
  VhSlicedPlanes F, V;
  uint32_t rows;                  // D->rows, for the host: which instantiation the launcher takes (not a kernel argument)
};
// One member of a fused batch (vh_scan_planes_batch.hip: scan_agg_planes_batch_kernel): what scan_agg_planes_kernel takes as arguments for one
// query, without V — the members of a group share it — and with the place of the member's LDS table in the launch's dynamic LDS. An array of
// them lies in device memory (the plans do not fit the kernel arguments) and is read through a restrict pointer, for the reason given above.
// Program and descriptor lie IN the member, by value: read through a pointer that was itself loaded from the array, the compiler no longer
// knows them for unclobbered — it took vector loads and turned every branch of the interpreter, which is on plan data, into a divergent one
// (952 exec-mask branches against the single kernel's 412; measured 25 % slower than the single queries: profiles/r18/NOTES.md).
// mask_of: the position in the array of the member whose pass mask this one uses (vh_batch.h, vh_batch_share: the same filter program over the
// same F against the same effective rows per segment); its own position: it evaluates B over F itself. Never a later position.
struct VhBatchMember {
  VhPlanDev P;
  VhBitsProg B;                   // (all zeros: no filter — D.has_filter says)
  VhPlaneAggDesc D;
  VhSlicedPlanes F;
  uint32_t lds_base;              // bytes, a multiple of 16
  uint32_t mask_of;
};

#if defined(__HIPCC__)
// pass mask of the lane's word (rows base + 32 * lane ..) of a chunk that begins at row `base` < seg_rows
__device__ __forceinline__ uint32_t vh_sliced_mask(const VhBitsProg& B, const VhSlicedPlanes& L, uint32_t seg, uint64_t base, uint32_t seg_rows, int lane) {
  const uint64_t row_l = base + (uint64_t)lane * 32u;
  const uint32_t keep = vh_sliced_tail_mask(row_l, seg_rows);
  uint32_t m = 0u;
  if (keep) m = vh_bits_eval(B, L.planes + (uint64_t)seg * L.stride, L.pitch, (uint32_t)(row_l >> 5) * 4u) & keep;
  return m;
}
#endif
