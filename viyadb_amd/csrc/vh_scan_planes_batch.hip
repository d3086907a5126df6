// The aggregate scan on the bit-sliced planes for a BATCH of queries (vh_query_agg_batch, include/viya_hip.h): up to VH_BATCH_MAX plans that
// scan_agg_planes_kernel (vh_scan_planes.hip) would each answer alone share ONE walk over the chunks, ONE load of the value planes V per plane
// word, one launch and one wait. What a member keeps to itself is what the single kernel's whole per-query state is: a pass mask — its own
// filter program over its own projection F against its own snapshot, unless an earlier member's is the same one (step 1 below) — and an LDS
// table of at most a few KB. vh_batch.h holds the rule that forms a group (same V, same scope, same segments, same chunks per segment) and
// the one that lets members of a group share a mask; QueryBuild::choose_plane_agg (vhh_launch.h) the rule that makes a plan a candidate.
#include "vh_kernels.h"
#include "vh_launch.h"
#include "vh_sliced.h"
#include "vh_bits_agg.h"
#include "vh_wave_scan.h"
#include "vh_plane_agg.h"
#include "vh_batch.h"

static_assert(sizeof(VhBatchMember) % 8 == 0, "VhBatchMember: an array of them is read with scalar loads");
static_assert(VH_BATCH_MAX <= 32, "scan_agg_planes_batch_kernel keeps a bit per member");

// Q: the members, in device memory (VH_BATCH_MAX plans of 3.9 KB do not fit the 4 KB of kernel arguments), read through the restrict pointer so
// that they come by scalar loads like the program and the descriptor of the single kernel (vh_sliced.h) — which is why a member holds its
// program and its descriptor by value. The walk is the single kernel's over
// the segments all members share. Per chunk:
//   1. every member's pass mask of the lane's word: 0 where the chunk lies at or beyond that member's snapshot or its segment is skipped.
//      ONE evaluation per mask class: a member whose filter program, projection F and effective rows per segment equal an earlier member's
//      (VhBatchMember::mask_of, set by the host with vh_batch_share) takes that member's word from its LDS slot instead of running the
//      interpreter again — K breakdowns under one filter evaluate it once. Its row counter, its share of `any` and `need`, its group loop,
//      its error flag and its flush stay its own;
//   2. nothing more when no lane of the wave has a passing row of any member;
//   3. the planes of V that a member with a passing row in the wave needs, loaded ONCE, into the array that is indexed by constants only — and
//      not at all by a lane without a passing row of any member;
//   4. per member with a passing row in the wave, the loop over its group ids (vh_plane_agg_groups) — or, for a row member of a launch
//      with ROWS = 1, the row sink (vh_plane_agg_rows) — into ITS table at lds + lds_base. Every
//      branch around it is uniform over the wave: all 64 lanes are active in it.
// A lane's masks wait for step 4 in lane-private slots of static LDS (8 KB; a write and a read per member and chunk, no conflicts), its row
// counters in registers that only constant indices reach (vh_member_put / _get: a chain of selects on the uniform member index, eight moves
// beside a filter evaluation): a runtime-indexed array would go to scratch memory, and with the masks in registers too the kernel took 177
// registers — two waves per SIMD instead of the single kernel's three. The launch bound asks for three: 168 registers, nothing spilled
// (profiles/r18/NOTES.md).
__device__ __forceinline__ void vh_member_put(uint32_t (&a)[VH_BATCH_MAX], uint32_t k, uint32_t x) {
#pragma unroll
  for (uint32_t q = 0; q < VH_BATCH_MAX; ++q) a[q] = q == k ? x : a[q];
}
__device__ __forceinline__ uint32_t vh_member_get(const uint32_t (&a)[VH_BATCH_MAX], uint32_t k) {
  uint32_t x = 0u;
#pragma unroll
  for (uint32_t q = 0; q < VH_BATCH_MAX; ++q) x = q == k ? a[q] : x;
  return x;
}

// ROWS = 1, launched when any member of the group is a row member (VhPlaneAggDesc::rows: more ids than the loop can pay for): step 4 takes
// such a member's surviving rows through the row sink (vh_plane_agg.h: vh_plane_agg_rows) — the branch is on plan data read by a scalar
// load, uniform like every other one around it — and every other member through the loop, as ROWS = 0 does for all. Steps 1 to 3 are the
// same text: a row member shares or lends a mask through mask_of like any other. The sink's per-wave queue is 4 KB of static LDS of that
// instantiation alone: with s_mask and 48 KB of tables two blocks fit a CU's 160 KB.
template <int BLOCK, int SCOPE, int ROWS>
__global__ __launch_bounds__(BLOCK, 3) void scan_agg_planes_batch_kernel(const VhBatchMember* __restrict__ Q, uint32_t n, const VhSlicedPlanes V, uint32_t chunks_per_seg) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint16_t* q = nullptr;
  if constexpr (ROWS) {
    __shared__ uint16_t s_rowq[BLOCK / 64][VH_PLANE_ROWS_QUEUE];
    q = s_rowq[wave];
  }
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) vh_scan_table_init<VH_MODE_DENSE_LDS, BLOCK>(Q[k].P, lds + Q[k].lds_base);

  const uint32_t nseg = Q[0].P.nseg;      // (part of the fuse key: the same for every member)
  __shared__ uint32_t s_mask[VH_BATCH_MAX][BLOCK];      // per member and lane: the chunk's pass mask (the lane's own slot: no barrier)
  uint32_t npassed32[VH_BATCH_MAX];                     // per lane and member: 32 rows of every chunk this wave takes
#pragma unroll
  for (int q = 0; q < VH_BATCH_MAX; ++q) npassed32[q] = 0u;
  uint32_t range_err = 0u;                // bit k: a passing row of member k belonged to none of its ids

  for (VhChunkWalk K(blockIdx.x, gridDim.x, (uint32_t)(BLOCK / 64), wave, chunks_per_seg); K.seg < nseg; K.next()) {
    const uint32_t seg = K.seg;
    const uint64_t base = K.base();
    const uint64_t row_l = base + (uint64_t)lane * 32u;
    uint32_t any = 0u, need = 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) {
      const VhBatchMember& M = Q[k];
      const uint32_t of = M.mask_of;      // (plan data by a scalar load: the branch is uniform)
      uint32_t m = 0u;
      if (of < k) {
        // An earlier member of the same mask class (vh_batch.h): its word IS this member's, the cut at the snapshot and the 0 of a chunk at
        // or beyond it included — equal effective rows in every segment are part of the class key, so nothing is checked a second time. The
        // slot is this thread's own, written earlier in this loop: no barrier. (A position that is not an earlier one evaluates: no slot
        // is ever read before it is written.)
        m = s_mask[of][threadIdx.x];
      } else {
        // (the snapshot lies behind a pointer of the plan: a vector load of a uniform address, made a scalar again so that the branch on it is one)
        const uint32_t seg_rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)M.P.seg_rows[seg]);
        if (base < seg_rows) m = M.D.has_filter ? vh_sliced_mask(M.B, M.F, seg, base, seg_rows, lane) : vh_sliced_tail_mask(row_l, seg_rows);
      }
      s_mask[k][threadIdx.x] = m;
      vh_member_put(npassed32, k, vh_member_get(npassed32, k) + __popc(m));
      any |= m;
      if (__ballot(m != 0u) != 0ull) need |= M.D.need;
    }
    if (__ballot(any != 0u) == 0ull) continue;

    uint32_t v[VH_BITS_MAX_FIELD];
#pragma unroll
    for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) v[p] = 0u;
    if (any) {      // (any != 0: the word begins below some member's snapshot, and V is as current as the table: the word exists)
      const char* planes = V.planes + (uint64_t)seg * V.stride;
      const uint32_t woff = (uint32_t)(row_l >> 5) * 4u;
#pragma unroll
      for (int p = 0; p < VH_BITS_MAX_FIELD; ++p)
        if ((need >> p) & 1u) v[p] = VH_BITS_LOAD(planes + (uint64_t)p * V.pitch + woff);
    }

#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t m = s_mask[k][threadIdx.x];
      if (__ballot(m != 0u) == 0ull) continue;
      const VhBatchMember& M = Q[k];
      bool err;
      if (ROWS && M.D.rows) err = vh_plane_agg_rows(M.P, &M.D, lds + M.lds_base, v, m, lane, q);
      else err = vh_plane_agg_groups(M.P, &M.D, M.D.care, M.D.valid, (uint32_t)M.P.G, lds + M.lds_base, v, m, lane);
      if (err) range_err |= 1u << k;
    }
  }

  // the end of the block, member by member: its error flag, its waves' row counters as one set of atomics (vh_scan_block_end keeps them in
  // static LDS and ends without a barrier: one between two calls), and behind all of them its table's flush, which begins with a barrier
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) {
    const VhPlanDev& P = Q[k].P;
    if (__ballot(((range_err >> k) & 1u) != 0u) != 0ull && lane == 0) atomicOr(P.counters + 2, VH_ERR_RANGE);
    unsigned long long npassed = vh_member_get(npassed32, k);
    for (int off = 32; off > 0; off >>= 1) npassed += __shfl_down(npassed, off);
    if (k) __syncthreads();
    vh_scan_block_end(P, npassed, 0ull, 0ull, 0u);
  }
#pragma unroll 1
  for (uint32_t k = 0; k < n; ++k) vh_scan_table_flush<VH_MODE_DENSE_LDS, BLOCK, SCOPE>(Q[k].P, lds + Q[k].lds_base);
}

void vh_launch_scan_planes_batch(const VhBatchMember* d_members, uint32_t n, const VhSlicedPlanes& V, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private, bool rows) {
  constexpr int BLOCK = 256;       // (as scan_agg_planes_kernel: vh_scan_planes.hip)
  vh_with_scope(xcd_private, [&](auto scope) {
    constexpr int SCOPE = decltype(scope)::value;
    if (rows) {      // (any member of the group is a row member)
      L.named("scan_agg_planes_batch_kernel<%d, %d, rows>", BLOCK, SCOPE);
      vh_launch_or_ask(L, scan_agg_planes_batch_kernel<BLOCK, SCOPE, 1>, BLOCK, true, d_members, n, V, chunks_per_seg);
    } else {
      L.named("scan_agg_planes_batch_kernel<%d, %d>", BLOCK, SCOPE);
      vh_launch_or_ask(L, scan_agg_planes_batch_kernel<BLOCK, SCOPE, 0>, BLOCK, true, d_members, n, V, chunks_per_seg);
    }
  });
}
