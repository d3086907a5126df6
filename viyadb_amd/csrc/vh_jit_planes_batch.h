// vh_jit_planes_batch.h — the hand-written frame of the aggregate ON the bit-sliced planes for the members of a fused BATCH, compiled per batch
// shape: scan_agg_planes_batch_kernel (vh_scan_planes_batch.hip) with the ordered list of member shapes a compile-time constant. vh_jit.hip
// writes one traits struct per member — VJ0, VJ1, ...: the struct a single plane-aggregate shape gets (vh_jit_planes.h) — and the list VJB:
//   VJB::N, BLOCK, SCOPE, ROWS            members, threads, the scope of the tables' flushes, whether any member takes the row sink
//   VJB::masks(Q, seg, base, row_l, m)    step 1, one line per member: a member that opens a mask class evaluates (vj_member_mask below),
//                                          a member of an earlier member's class copies that member's word
//   VJB::v_load(P, seg, row_l, need, v)   step 3, V's planes by constant number
//   VJB::each(f)                          f(VhIdx<k>, VJk) for every member in order: the frame's loops over the members, unrolled
// With positions constant the masks and the row counters are arrays that only constants index — registers —: neither the pre-built kernel's
// 8 KB of static LDS nor its select chains (vh_member_put / _get) exist here, and a member's sink is the instantiation for its own fields.
// What stays DATA, read from the members' array Q (device memory, scalar loads through the restrict pointer: vh_sliced.h): literals and truth
// tables (Q[k].P.ilits / .set), the snapshots (Q[k].P.seg_rows), lo / extent / stride (Q[k].P.g), the ids' patterns and validity (Q[k].D) and
// lds_base. Member k's F and V lie in the last two slots of Q[k].P, as in the single compiled kernel; V is the same projection for all.
// The sinks' contract (vh_plane_agg.h) holds as in the pre-built kernel: every branch around a sink is on a ballot or on plan data read by
// scalar loads, so all 64 lanes are active in every DPP scan and every ds_bpermute.
#pragma once
#include "vh_jit_planes.h"

// Member J's pass mask of the lane's word: 0 where the chunk lies at or beyond its snapshot or its segment is skipped; the word's rows below
// the snapshot, and of those the ones its filter passes — one evaluation of the generated expression over F's planes.
template <class J>
__device__ __forceinline__ uint32_t vj_member_mask(const VhPlanDev& P, uint32_t seg, uint64_t base, uint64_t row_l) {
  // (the snapshot lies behind a pointer of the plan: a vector load of a uniform address, made a scalar again so that the branch on it is one)
  const uint32_t seg_rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.seg_rows[seg]);
  uint32_t m = 0u;
  if (base < seg_rows) {
    m = vh_sliced_tail_mask(row_l, seg_rows);
    if constexpr (J::PA_FILTER) {
      if (m) {
        const typename J::Lits L(P);
        uint32_t f[J::NV ? J::NV : 1];
        J::template preload<true>(P, seg, (uint32_t)row_l, seg_rows, f);
        m &= J::mask(L, f);
      }
    }
  }
  return m;
}

// scan_agg_planes_batch_kernel's walk and its four steps per chunk, the member loops unrolled over B's list.
template <class B>
__device__ __forceinline__ void vj_plane_agg_batch(const VhBatchMember* __restrict__ Q, uint32_t chunks_per_seg) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int BLOCK = B::BLOCK, N = B::N;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint16_t* q = nullptr;
  if constexpr (B::ROWS) {      // (one queue per wave, of this text alone: some member has PA_SINK == 2)
    __shared__ uint16_t s_rowq[BLOCK / 64][VH_PLANE_ROWS_QUEUE];
    q = s_rowq[wave];
  }
  B::each([&](auto k, auto) __attribute__((always_inline)) { vh_scan_table_init<VH_MODE_DENSE_LDS, BLOCK>(Q[k].P, lds + Q[k].lds_base); });

  const uint32_t nseg = (uint32_t)Q[0].P.nseg;      // (part of the fuse key: the same for every member)
  uint32_t npassed32[N];                            // per lane and member: 32 rows of every chunk this wave takes
#pragma unroll
  for (int k = 0; k < N; ++k) npassed32[k] = 0u;
  uint32_t range_err = 0u;                          // bit k: a passing row of member k belonged to none of its ids

  for (VhChunkWalk K(blockIdx.x, gridDim.x, (uint32_t)(BLOCK / 64), wave, chunks_per_seg); K.seg < nseg; K.next()) {
    // Plan data is loop-invariant, and hoisted out of this loop it lives in scalar registers for the whole walk. The single kernel does
    // that with one plan; here the members' literals, plane addresses, snapshots, tables and patterns together pass the 100-odd scalar
    // registers there are and the rest is spilled — 80 of them with eight members, 14 already with four members of four mask classes
    // (selftest shapes 42 and 45). So the array is addressed through an offset the compiler cannot see through (a scalar 0 out of an empty
    // asm statement), whatever the number of members: the loads stay scalar loads from the restrict pointer, but they are issued in the
    // chunk that uses them — they hit the scalar cache — and their registers are free again after the member's step.
    uint32_t zero = 0u;
    asm volatile("" : "+s"(zero));
    const VhBatchMember* __restrict__ Qc = reinterpret_cast<const VhBatchMember*>(reinterpret_cast<const char*>(Q) + zero);
    const uint32_t seg = K.seg;
    const uint64_t base = K.base();
    const uint64_t row_l = base + (uint64_t)lane * 32u;
    // 1. the masks, one evaluation per class
    uint32_t m[N];
    B::masks(Qc, seg, base, row_l, m);
    uint32_t any = 0u, need = 0u;
    B::each([&](auto k, auto j) __attribute__((always_inline)) {
      npassed32[k] += __popc(m[k]);
      any |= m[k];
      if (__ballot(m[k] != 0u) != 0ull) need |= decltype(j)::PA_NEED;
    });
    // 2. no passing row of any member in the wave
    if (__ballot(any != 0u) == 0ull) continue;

    // 3. V's plane words, once (any != 0: the word begins below some member's snapshot, and V is as current as the table: the word exists)
    uint32_t v[VH_BITS_MAX_FIELD];
#pragma unroll
    for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) v[p] = 0u;
    if (any) B::v_load(Qc[0].P, seg, (uint32_t)row_l, need, v);

    // 4. per member with a passing row in the wave, its sink into its table
    B::each([&](auto k, auto j) __attribute__((always_inline)) {
      typedef decltype(j) J;
      if (__ballot(m[k] != 0u) == 0ull) return;
      const VhBatchMember& M = Qc[k];
      const VjPlaneShape<J> shape{M.P};
      bool err;
      if constexpr (J::PA_SINK == 2) err = vh_plane_agg_rows_t(shape, M.P, lds + M.lds_base, v, m[k], lane, q);
      else err = vh_plane_agg_groups_t(shape, M.P, &M.D, (uint32_t)J::PA_CARE, M.D.valid, (uint32_t)M.P.G, lds + M.lds_base, v, m[k], lane);
      if (err) range_err |= 1u << k;
    });
  }

  // the end of the block, member by member, as the pre-built kernel has it: the error flag, the waves' row counters as one set of atomics
  // (vh_scan_block_end keeps them in static LDS and ends without a barrier: one between two calls), behind all of them every table's flush
  B::each([&](auto k, auto) __attribute__((always_inline)) {
    const VhPlanDev& P = Q[k].P;
    if (__ballot(((range_err >> k) & 1u) != 0u) != 0ull && lane == 0) atomicOr(P.counters + 2, VH_ERR_RANGE);
    unsigned long long npassed = npassed32[k];
    for (int off = 32; off > 0; off >>= 1) npassed += __shfl_down(npassed, off);
    if (k) __syncthreads();
    vh_scan_block_end(P, npassed, 0ull, 0ull, 0u);
  });
  B::each([&](auto k, auto) __attribute__((always_inline)) { vh_scan_table_flush<VH_MODE_DENSE_LDS, BLOCK, B::SCOPE>(Q[k].P, lds + Q[k].lds_base); });
}
