// vh_plane_agg.h — what the two aggregate scans ON the bit-sliced planes share on the device: scan_agg_planes_kernel (vh_scan_planes.hip, one
// query) and scan_agg_planes_batch_kernel (vh_scan_planes_batch.hip, the members of a fused batch). One plane word of V, already in registers,
// and one query's pass mask in; that query's updates of its block's LDS table out. Two sinks with that contract: the loop over group ids
// (vh_plane_agg_groups: one LDS update per chunk, id and metric; at most VH_PLANE_AGG_MAX_GROUPS ids) and the row sink (vh_plane_agg_rows: one
// per surviving row and metric; any number of ids the table holds).
#pragma once
#include "vh_kernels.h"
#include "vh_sliced.h"
#include "vh_bits_agg.h"
#include "vh_wave_scan.h"

#if defined(__HIPCC__)
// WHERE THE FIELDS LIE is a traits object of the two sinks, so that one text serves the pre-built kernels, which read it from the plan
// (VhPlaneAggPlan below: D->moff / mbits / need, P.m[j].sop() — run-time data, a loop over the metrics that is not unrolled), and a kernel compiled for
// one plan's shape, which knows it (vh_jit_planes.h: VjPlaneShape — the same members as constants, the loop unrolled). A traits type has
//   need()                      bit p: plane p of V belongs to a field of the plan
//   each_metric(f)              f(j) for every metric j of the plan, j an int or a VhIdx<J>
//   sop(j), sum(j, v, m), min(j, v, m), max(j, v, m)      metric j's state operation and its field's aggregates over the rows of m (vh_bits_agg.h)
//   field(j, rec), gid(rec, &id)                          metric j's field and the dense group id out of one row's record
// Everything that depends on lo / extent / stride or on the ids stays data in either form: P.g[], D->pat, D->valid.
template <int J> struct VhIdx { static constexpr int value = J; __device__ constexpr operator int() const { return J; } };
struct VhPlaneAggPlan {
  const VhPlanDev& P;
  const VhPlaneAggDesc* __restrict__ D;
  __device__ __forceinline__ uint32_t need() const { return D->need; }
  template <class F> __device__ __forceinline__ void each_metric(F f) const {
#pragma unroll 1
    for (int j = 0; j < P.nmetric; ++j) f(j);
  }
  __device__ __forceinline__ int sop(int j) const { return (int)P.m[j].sop(); }
  __device__ __forceinline__ uint64_t sum(int j, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { return vh_bits_sum_at(v, D->moff[j], D->mbits[j], m); }
  __device__ __forceinline__ uint32_t min(int j, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { bool e; return vh_bits_min_at(v, D->moff[j], D->mbits[j], m, &e); }
  __device__ __forceinline__ uint32_t max(int j, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { bool e; return vh_bits_max_at(v, D->moff[j], D->mbits[j], m, &e); }
  __device__ __forceinline__ uint32_t field(int j, uint32_t rec) const { return vh_bits_row_field(rec, D->moff[j], D->mbits[j]); }
  __device__ __forceinline__ bool gid(uint32_t rec, uint64_t* id) const { return vh_bits_row_gid(rec, P.ngroup, P.g, D->goff, D->gbits, id); }
};

// The loop over the group ids of ONE plan for a lane's plane word. v: every plane of V the plan needs, for the lane's 32 rows (planes the plan
// does not need may hold anything: care, pat and the fields name the ones that are looked at); mask: the lane's passing rows; lds: the plan's
// LDS table. Every branch is on the plan, so all 64 lanes are active in it, which the wave combination needs — the caller must be in uniform
// control flow too. Per id g: the lane's rows of g, nothing more to do when no lane has any, and per metric the lane's partial result, combined
// across the wave (the DPP scans of vh_wave_scan.h) and added to the LDS table by ONE lane: one LDS update per (chunk, group, metric) in
// place of one per row and metric. Returns whether a passing row of the lane belongs to no id (a value outside the planned range).
template <class T>
__device__ __forceinline__ bool vh_plane_agg_groups_t(const T& t, const VhPlanDev& P, const VhPlaneAggDesc* __restrict__ D, uint32_t care, uint64_t valid, uint32_t G,
                                                      char* lds, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t mask, int lane) {
  uint32_t seen = 0u;
#pragma unroll 1
  for (uint32_t g = 0; g < G; ++g) {
    if (__ballot((mask & ~seen) != 0u) == 0ull) break;      // every passing row of the wave's chunk has found its group
    const uint32_t mg = ((valid >> g) & 1ull) ? (mask & vh_bits_match(v, care, D->pat[g])) : 0u;
    seen |= mg;
    if (__ballot(mg != 0u) == 0ull) continue;
    const bool in = mg != 0u;
    t.each_metric([&](auto j) __attribute__((always_inline)) {
      const int sop = t.sop(j);
      // the lanes' partial results combined by DPP scans (vh_wave_scan.h; all lanes are active here): lane 63 ends up with the wave's. A
      // field's value is an unsigned number of at most 32 bits, so MAX takes 0 from a lane without a row of g and MIN is the complement
      // of the MAX of the complements.
      uint64_t total;
      if (sop == SOP_ADD32 || sop == SOP_ADD64) total = vh_wave_incl_add((unsigned long long)t.sum(j, v, mg));
      else if (sop == SOP_MIN_I32 || sop == SOP_MIN_U32 || sop == SOP_MIN_I64 || sop == SOP_MIN_U64) total = (uint32_t)~vh_wave_incl_max(in ? ~t.min(j, v, mg) : 0u);
      else total = vh_wave_incl_max(in ? t.max(j, v, mg) : 0u);
      if (lane == 63) vh_state_update<__HIP_MEMORY_SCOPE_WORKGROUP>(lds + P.m[j].lds_off, g, sop, total);
    });
    if (lane == 63) reinterpret_cast<uint8_t*>(lds + P.lds_present_off)[g] = 1;
  }
  return (mask & ~seen) != 0u;
}
__device__ __forceinline__ bool vh_plane_agg_groups(const VhPlanDev& P, const VhPlaneAggDesc* __restrict__ D, uint32_t care, uint64_t valid, uint32_t G,
                                                    char* lds, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t mask, int lane) {
  return vh_plane_agg_groups_t(VhPlaneAggPlan{P, D}, P, D, care, valid, G, lds, v, mask, lane);
}

// The ROW SINK: the same contract as vh_plane_agg_groups — a lane's plane words of V and its pass mask in, the plan's updates of its LDS table
// out, whether a passing row of the lane belonged to no id returned — for plans of more ids than a loop over them can pay for. It turns
// every surviving row back into its record, from the plane words in registers: no queue of row numbers, no gather from memory.
//   COMPACT. The mask is taken in VH_PLANE_ROWS_SLICES slices of VH_PLANE_ROWS_SLICE_BITS bits per lane. Per slice a lane has popc survivors;
//   an exclusive wave prefix of those (the DPP scans of vh_wave_scan.h) is where it writes one entry `lane << 5 | bit` per set bit into the
//   wave's queue q (VH_PLANE_ROWS_QUEUE entries of 16 bits in static LDS): the queue holds the slice's survivors by lane, then by bit.
//   DRAIN, in groups of 64: lane l takes survivor i = 64 b + l, entry (s, r), and fetches lane s's word of every plane of `need` with
//   ds_bpermute; bit r of that word is bit p of the record (vh_bits_agg.h: vh_bits_row_bit). The loop over p is unrolled, under the uniform
//   `need` bit, so v[] is indexed by constants only. ALL 64 lanes execute every bpermute — the trip count is the wave's, a lane with
//   i >= total fetches from itself and updates nothing —: a source lane that exec switches off supplies no defined data.
//   Per record: the group id (vh_bits_row_gid; a field outside [lo, lo + extent) skips the row and sets the return value), per metric one
//   vh_state_update with its field's value — wrapping is vh_state_update's, as in the loop — and the presence byte, as vh_consume does.
// Like the loop, the caller must be in uniform control flow: the scans and the bpermutes need all 64 lanes.
#define VH_PLANE_ROWS_SLICE_BITS 8
#define VH_PLANE_ROWS_SLICES (32 / VH_PLANE_ROWS_SLICE_BITS)
#define VH_PLANE_ROWS_QUEUE (64 * VH_PLANE_ROWS_SLICE_BITS)      // 512 entries of 2 bytes: 1 KB per wave
template <class T>
__device__ __forceinline__ bool vh_plane_agg_rows_t(const T& t, const VhPlanDev& P, char* lds, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t mask, int lane, uint16_t* q) {
  const uint32_t need = t.need();
  bool range_err = false;
#pragma unroll 1
  for (int k = 0; k < VH_PLANE_ROWS_SLICES; ++k) {
    uint32_t mk = (mask >> (VH_PLANE_ROWS_SLICE_BITS * k)) & ((1u << VH_PLANE_ROWS_SLICE_BITS) - 1u);
    const uint32_t mine = (uint32_t)__popc(mk);
    const uint32_t incl = vh_wave_incl_add(mine);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);      // (<= VH_PLANE_ROWS_QUEUE: SLICE_BITS survivors a lane)
    if (total == 0u) continue;
    uint32_t at = incl - mine;
    while (mk) {
      const uint32_t bit = (uint32_t)__builtin_ctz(mk);
      mk &= mk - 1u;
      q[at++] = (uint16_t)((uint32_t)lane << 5 | (uint32_t)(VH_PLANE_ROWS_SLICE_BITS * k) + bit);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < total; i0 += 64u) {
      const bool act = i0 + (uint32_t)lane < total;
      const uint32_t e = act ? (uint32_t)q[i0 + (uint32_t)lane] : (uint32_t)lane << 5;
      const uint32_t s = e >> 5, r = e & 31u;
      uint32_t rec = 0u;
#pragma unroll
      for (int p = 0; p < VH_BITS_MAX_FIELD; ++p)
        if ((need >> p) & 1u) rec |= vh_bits_row_bit((uint32_t)__builtin_amdgcn_ds_bpermute((int)(s << 2), (int)v[p]), r, (uint32_t)p);
      uint64_t gid = 0;
      const bool in = t.gid(rec, &gid);
      range_err |= act && !in;
      if (act && in) {
        t.each_metric([&](auto j) __attribute__((always_inline)) {
          vh_state_update<__HIP_MEMORY_SCOPE_WORKGROUP>(lds + P.m[j].lds_off, gid, t.sop(j), (uint64_t)t.field(j, rec));
        });
        reinterpret_cast<uint8_t*>(lds + P.lds_present_off)[gid] = 1;
      }
    }
    __builtin_amdgcn_wave_barrier();      // (the next slice writes the queue this one read)
  }
  // the lane that drained a row is not the lane that owns it: every lane of the wave answers for the wave's rows
  return __ballot(range_err) != 0ull;
}
__device__ __forceinline__ bool vh_plane_agg_rows(const VhPlanDev& P, const VhPlaneAggDesc* __restrict__ D, char* lds, const uint32_t (&v)[VH_BITS_MAX_FIELD],
                                                  uint32_t mask, int lane, uint16_t* q) {
  return vh_plane_agg_rows_t(VhPlaneAggPlan{P, D}, P, lds, v, mask, lane, q);
}
#endif
