// vh_plane_agg.h — what the two aggregate scans ON the bit-sliced planes share on the device: scan_agg_planes_kernel (vh_scan_planes.hip, one
// query) and scan_agg_planes_batch_kernel (vh_scan_planes_batch.hip, the members of a fused batch). One plane word of V, already in registers,
// and one query's pass mask in; that query's updates of its block's LDS table out.
#pragma once
#include "vh_kernels.h"
#include "vh_sliced.h"
#include "vh_bits_agg.h"
#include "vh_wave_scan.h"

#if defined(__HIPCC__)
// The loop over the group ids of ONE plan for a lane's plane word. v: every plane of V the plan needs, for the lane's 32 rows (planes the plan
// does not need may hold anything: care, pat and the fields name the ones that are looked at); mask: the lane's passing rows; lds: the plan's
// LDS table. Every branch is on the plan, so all 64 lanes are active in it, which the wave combination needs — the caller must be in uniform
// control flow too. Per id g: the lane's rows of g, nothing more to do when no lane has any, and per metric the lane's partial result, combined
// across the wave (the DPP scans of vh_wave_scan.h) and added to the LDS table by ONE lane: one LDS update per (chunk, group, metric) in
// place of one per row and metric. Returns whether a passing row of the lane belongs to no id (a value outside the planned range).
__device__ __forceinline__ bool vh_plane_agg_groups(const VhPlanDev& P, const VhPlaneAggDesc* __restrict__ D, uint32_t care, uint64_t valid, uint32_t G,
                                                    char* lds, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t mask, int lane) {
  uint32_t seen = 0u;
#pragma unroll 1
  for (uint32_t g = 0; g < G; ++g) {
    if (__ballot((mask & ~seen) != 0u) == 0ull) break;      // every passing row of the wave's chunk has found its group
    const uint32_t mg = ((valid >> g) & 1ull) ? (mask & vh_bits_match(v, care, D->pat[g])) : 0u;
    seen |= mg;
    if (__ballot(mg != 0u) == 0ull) continue;
    const bool in = mg != 0u;
#pragma unroll 1
    for (int j = 0; j < P.nmetric; ++j) {
      const VhMetricDev& m = P.m[j];
      const int sop = (int)m.sop();
      const uint32_t off = D->moff[j], nb = D->mbits[j];
      // the lanes' partial results combined by DPP scans (vh_wave_scan.h; all lanes are active here): lane 63 ends up with the wave's. A
      // field's value is an unsigned number of at most 32 bits, so MAX takes 0 from a lane without a row of g and MIN is the complement
      // of the MAX of the complements.
      uint64_t total;
      bool empty;
      if (sop == SOP_ADD32 || sop == SOP_ADD64) total = vh_wave_incl_add((unsigned long long)vh_bits_sum_at(v, off, nb, mg));
      else if (sop == SOP_MIN_I32 || sop == SOP_MIN_U32 || sop == SOP_MIN_I64 || sop == SOP_MIN_U64) total = (uint32_t)~vh_wave_incl_max(in ? ~vh_bits_min_at(v, off, nb, mg, &empty) : 0u);
      else total = vh_wave_incl_max(in ? vh_bits_max_at(v, off, nb, mg, &empty) : 0u);
      if (lane == 63) vh_state_update<__HIP_MEMORY_SCOPE_WORKGROUP>(lds + m.lds_off, g, sop, total);
    }
    if (lane == 63) reinterpret_cast<uint8_t*>(lds + P.lds_present_off)[g] = 1;
  }
  return (mask & ~seen) != 0u;
}
#endif
