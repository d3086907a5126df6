// vh_launch.h — launch entry points of the scan kernels; each lives in its own translation unit so
// the 30-odd template instantiations compile in parallel (viyadb_amd/build.py).
#pragma once
#include "vh_internal.h"
#include <cstdio>
#include <string>
#include <type_traits>

// What a pre-built scan launcher is asked for. With `occ` or `name` set nothing is launched: the launcher answers for the instantiation it
// WOULD launch — *occ = blocks of it that fit one CU with `lds` bytes of dynamic LDS, name = its symbol as rocprofv3 prints it.
struct VhScanLaunch {
  int grid = 0; size_t lds = 0; hipStream_t stream = nullptr;
  int* occ = nullptr; char* name = nullptr; size_t name_cap = 0;
  template <typename... A> void named(const char* fmt, A... a) const { if (name) snprintf(name, name_cap, fmt, a...); }
};
// Launch k, or ask its occupancy, or neither (the name alone was asked). ask_occ = false: a launcher that reports none — *L.occ stays.
template <typename... KA, typename... A>
static inline void vh_launch_or_ask(const VhScanLaunch& L, void (*k)(KA...), int block, bool ask_occ, const A&... args) {
  if (L.occ && ask_occ && hipOccupancyMaxActiveBlocksPerMultiprocessor(L.occ, k, block, L.lds) != hipSuccess) *L.occ = 0;
  if (!L.occ && !L.name) hipLaunchKernelGGL(k, dim3(L.grid), dim3(block), L.lds, L.stream, args...);
}
// f(std::integral_constant<int, SCOPE>): a table with a private copy per XCD is updated at workgroup scope, a shared one at agent scope
template <typename F> static inline void vh_with_scope(bool xcd_private, F&& f) {
  if (xcd_private) f(std::integral_constant<int, __HIP_MEMORY_SCOPE_WORKGROUP>{});
  else f(std::integral_constant<int, __HIP_MEMORY_SCOPE_AGENT>{});
}
// f(std::integral_constant<int, NP>): the register-resident kernels are instantiated for 1 .. 4 predicate columns (no filter counts as one)
template <typename F> static inline void vh_with_np(int npred, F&& f) {
  if (npred <= 1) f(std::integral_constant<int, 1>{});
  else if (npred == 2) f(std::integral_constant<int, 2>{});
  else if (npred == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}
void vh_launch_scan_generic(int mode, const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private);      // reports no occupancy
void vh_launch_scan_fast_lds(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private);               // reports no occupancy
void vh_launch_scan_lanes_lds(const VhPlanDev& P, int block, const VhScanLaunch& L, bool xcd_private);
void vh_launch_scan_lanes_hash(const VhPlanDev& P, const VhScanLaunch& L);
void vh_launch_scan_lanes_part(const VhPlanDev& P, const VhScanLaunch& L);
void vh_launch_scan_fast_global(const VhPlanDev& P, const VhScanLaunch& L, bool xcd_private);
void vh_launch_scan_fast_hash(const VhPlanDev& P, const VhScanLaunch& L);
void vh_launch_scan_fast_part(const VhPlanDev& P, const VhScanLaunch& L);
struct VhSlicedRef;
// the pre-built scan over the bit-sliced predicate planes (vh_sliced.h), whatever the organisation: `mode` picks the sink
void vh_launch_scan_sliced(int mode, const VhPlanDev& P, const VhSlicedRef& A, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private);
struct VhPlaneAggRef;
// the aggregate scan ON the bit-sliced planes (vh_sliced.h): DENSE_LDS plans of at most VH_PLANE_AGG_MAX_GROUPS ids, sums and min / max by popcount;
// A.rows: the row sink's instantiation, for plans of more ids (one LDS update per surviving row and metric, from the plane words in registers)
void vh_launch_scan_planes(const VhPlanDev& P, const VhPlaneAggRef& A, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private);
struct VhBatchMember;
struct VhSlicedPlanes;
// ... for the `n` members of a fused batch at once (vh_sliced.h, vh_batch.h): one walk, one load of V; L.lds = the members' LDS tables together;
// rows: some member is a row member (VhPlaneAggDesc::rows) — the instantiation that carries the row sink beside the loop
void vh_launch_scan_planes_batch(const VhBatchMember* d_members, uint32_t n, const VhSlicedPlanes& V, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private, bool rows);

// The tails of DENSE_PART behind the scan, and beside each launcher the symbol of the kernel it runs (for vh_result_kernel).
void vh_launch_part_agg(const VhPlanDev& P, int blocks_per_part, size_t lds, hipStream_t s);
const char* vh_part_agg_name();
// One- and two-word tuples of a two-level plan are split through the ring writer (part_split_ring_kernel: a block is one writer, extents by
// position); wider tuples by part_split_kernel. The name, the pools' layout (QueryBuild::layout_scratch) and the launcher go by this.
static inline bool vh_part_split_rings(const VhPlanDev& P) { return P.tw == 2 || P.gid_bits; }
void vh_launch_part_split(const VhPlanDev& P, int blocks_per_part, bool ring, hipStream_t s);
std::string vh_part_split_name(const VhPlanDev& P);
struct VhHpArgs;
struct VhHeavyTuples;
void vh_launch_heavy_tuples(const VhPlanDev& P, const VhHeavyTuples& A, int num_cu, hipStream_t s);      // a second pass over heavy partitions, from the first pass's tuples (vh_hpart.h)
void vh_launch_hpart(const VhPlanDev& P, const VhHpArgs* d_args, int units, int num_cu, int scan_blocks, int ring_blocks, hipStream_t s);      // hashed partitioning: everything behind the scan (vh_hpart.h)
