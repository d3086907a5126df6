// vh_jit_planes.h — the hand-written frame of the aggregate ON the bit-sliced planes, compiled per plan shape: scan_agg_planes_kernel
// (vh_scan_planes.hip) with everything that is SHAPE turned into constants of the generated traits struct `VJ` (vh_jit.hip writes it):
//   * the filter is one expression over the planes of F its leaves read (VJ::mask over VJ::preload: the text the bit-sliced compacting
//     scan gets, vj_bits_rel / vj_bits_inset of vh_jit_body.h) — no interpreter, no program in memory;
//   * V's planes are loaded by constant plane number, exactly those of VJ::PA_NEED (VJ::pa_load);
//   * a metric's field, its state operation and the sink are constants: a 10-bit SUM is ten popcounts (vh_bits_sum_c), MIN / MAX walk the
//     field's planes and no others, the loop over the metrics is unrolled.
// What stays DATA, so that one code object serves every query of the shape: the literals and the sets' truth tables (P.ilits, P.set), the
// snapshot, and whatever depends on the group columns' lo / extent / stride — the ids' patterns and validity (VhPlaneAggDesc::pat / valid,
// read through a restrict pointer of its own, which keeps the loads scalar: vh_sliced.h) and P.g[] in the row sink.
// The two sinks are vh_plane_agg.h's, instantiated with VjPlaneShape in the place of VhPlaneAggPlan; their contract — uniform control
// flow, all 64 lanes in every DPP scan and every ds_bpermute, one lane doing the LDS update in the loop form — is stated there.
// Only the text of a plane-aggregate shape includes this file: every other shape's text and frame are what they were.
#pragma once
#include "vh_jit_body.h"
#include "vh_plane_agg.h"

// vh_plane_agg.h's traits with the generated constants: VJ::PA_NEED, VJ::NM, VJ::m_sop[], VJ::pa_moff[] / pa_mbits[] (metric j's field in V),
// VJ::NG, VJ::pa_goff[] / pa_gbits[] (group column i's).
template <class J>
struct VjPlaneShape {
  const VhPlanDev& P;
  __device__ __forceinline__ constexpr uint32_t need() const { return J::PA_NEED; }
  template <int I, class F> __device__ __forceinline__ void from(F& f) const {
    if constexpr (I < J::NM) { f(VhIdx<I>{}); from<I + 1>(f); }
  }
  template <class F> __device__ __forceinline__ void each_metric(F f) const { from<0>(f); }
  template <int I> __device__ __forceinline__ constexpr int sop(VhIdx<I>) const { return J::m_sop[I]; }
  template <int I> __device__ __forceinline__ uint64_t sum(VhIdx<I>, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { return vh_bits_sum_c<J::pa_moff[I], J::pa_mbits[I]>(v, m); }
  template <int I> __device__ __forceinline__ uint32_t min(VhIdx<I>, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { bool e; return vh_bits_min_c<J::pa_moff[I], J::pa_mbits[I]>(v, m, &e); }
  template <int I> __device__ __forceinline__ uint32_t max(VhIdx<I>, const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) const { bool e; return vh_bits_max_c<J::pa_moff[I], J::pa_mbits[I]>(v, m, &e); }
  template <int I> __device__ __forceinline__ uint32_t field(VhIdx<I>, uint32_t rec) const { return vh_bits_row_field(rec, (uint32_t)J::pa_moff[I], (uint32_t)J::pa_mbits[I]); }
  // (vh_bits_row_gid with the fields' places constant; lo, extent and stride are the plan's)
  template <int I> __device__ __forceinline__ void digit(uint32_t rec, uint64_t& id, bool& ok) const {
    if constexpr (I < J::NG) {
      const uint64_t f = vh_bits_row_field(rec, (uint32_t)J::pa_goff[I], (uint32_t)J::pa_gbits[I]), d = f - P.g[I].lo;
      ok = ok && f >= P.g[I].lo && d < P.g[I].extent;
      id += d * P.g[I].stride;
      digit<I + 1>(rec, id, ok);
    }
  }
  __device__ __forceinline__ bool gid(uint32_t rec, uint64_t* out) const {
    uint64_t id = 0;
    bool ok = true;
    digit<0>(rec, id, ok);
    *out = id;
    return ok;
  }
};

// scan_agg_planes_kernel's walk, word for word: a wave takes 2048-row chunks (VhChunkWalk), lane l owns plane word l of the chunk. A skipped
// segment, a chunk at or beyond the snapshot and a word at or beyond it are never read; a lane none of whose rows pass reads none of V.
// Counters, VH_ERR_RANGE and the block's table (vh_scan_table_init / vh_scan_block_end / vh_scan_table_flush) as there.
template <class J>
__device__ __forceinline__ void vj_plane_agg(const VhPlanDev& P, const VhPlaneAggDesc* __restrict__ D, uint32_t chunks_per_seg) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int BLOCK = J::BLOCK;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  vh_scan_table_init<VH_MODE_DENSE_LDS, BLOCK>(P, lds);

  const typename J::Lits L(P);
  const VjPlaneShape<J> shape{P};
  uint16_t* q = nullptr;
  if constexpr (J::PA_SINK == 2) {
    __shared__ uint16_t s_rowq[BLOCK / 64][VH_PLANE_ROWS_QUEUE];
    q = s_rowq[wave];
  }
  uint32_t npassed32 = 0;                              // per lane: 32 rows of every chunk this wave takes
  bool range_err = false;

  for (VhChunkWalk K(blockIdx.x, gridDim.x, (uint32_t)(BLOCK / 64), wave, chunks_per_seg); K.seg < P.nseg; K.next()) {
    const uint32_t seg = K.seg;
    const uint64_t base = K.base();
    const uint32_t seg_rows = P.seg_rows[seg];
    if (base >= seg_rows) continue;
    const uint64_t row_l = base + (uint64_t)lane * 32u;
    uint32_t mask = vh_sliced_tail_mask(row_l, seg_rows);      // (0: the word begins at or beyond the snapshot — nothing of it is read)
    if constexpr (J::PA_FILTER) {
      if (mask) {
        uint32_t f[J::NV ? J::NV : 1];
        J::template preload<true>(P, seg, (uint32_t)row_l, seg_rows, f);
        mask &= J::mask(L, f);
      }
    }
    npassed32 += __popc(mask);
    if (__ballot(mask != 0u) == 0ull) continue;

    uint32_t v[VH_BITS_MAX_FIELD];
#pragma unroll
    for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) v[p] = 0u;
    if (mask) J::pa_load(P, seg, (uint32_t)row_l, v);      // (mask != 0: the word begins below the snapshot)

    if constexpr (J::PA_SINK == 2) range_err |= vh_plane_agg_rows_t(shape, P, lds, v, mask, lane, q);
    else range_err |= vh_plane_agg_groups_t(shape, P, D, (uint32_t)J::PA_CARE, D->valid, (uint32_t)P.G, lds, v, mask, lane);
  }

  if (__ballot(range_err) != 0ull && lane == 0) atomicOr(P.counters + 2, VH_ERR_RANGE);
  unsigned long long npassed = npassed32;
  for (int off = 32; off > 0; off >>= 1) npassed += __shfl_down(npassed, off);
  vh_scan_block_end(P, npassed, 0ull, 0ull, 0u);
  vh_scan_table_flush<VH_MODE_DENSE_LDS, BLOCK, J::SCOPE>(P, lds);
}
