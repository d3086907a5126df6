// The aggregate scan ON the bit-sliced predicate planes: the fourth reader of the planes, and the first that turns no survivor back into a
// row. The filter program gives the pass mask of a lane's 32 rows (vh_bits_eval.h, over projection F); the group columns' fields give the rows
// of every group id; a SUM is Σ_b popcount(rows & plane b) << b over the metric's field, MIN / MAX a narrowing of the rows from the top
// plane down (vh_bits_agg.h, over projection V). No queue, no gather, no state update per row: the bytes read are the bits of the fields
// involved, whatever passes. Serves the DENSE_LDS organisation (scalar aggregates included) with at most VH_PLANE_AGG_MAX_GROUPS group ids,
// integer SUM / COUNT / AVG / MIN / MAX states; QueryBuild::choose_plane_agg (vhh_launch.h) holds the rule.
#include "vh_kernels.h"
#include "vh_launch.h"
#include "vh_sliced.h"
#include "vh_bits_agg.h"
#include "vh_wave_scan.h"
#include "vh_plane_agg.h"

// VhPlanDev by value as for every scan kernel, the two projections' places by value behind it; program and descriptor lie in the plan block
// and are read through restrict pointers of their own (vh_sliced.h).
static_assert(sizeof(VhPlanDev) + 2 * sizeof(void*) + 2 * sizeof(VhSlicedPlanes) + 8 <= 4096, "scan_agg_planes_kernel: plan and planes together exceed the 4 KB of kernel arguments");
static_assert(VH_PLANE_AGG_MAX_GROUPS <= 64, "VhPlaneAggDesc::valid has a bit per group id");

// scan_agg_sliced_kernel's walk: a wave takes 2048-row chunks (VhChunkWalk), lane l owns plane word l of the chunk. A skipped segment, a chunk
// at or beyond the snapshot and a word at or beyond it are never read (vh_sliced_mask / vh_sliced_tail_mask); a lane none of whose rows pass
// reads none of V either. Per word the lane loads every plane of V that a field of the plan covers ONCE, into an array that is indexed by
// constants only (V has at most 32 planes: vh_bits_agg.h on the `_at` form). Then, per group id g — a loop whose every branch is on the plan,
// so all 64 lanes are active in it, which the wave combination needs —: the lane's rows of g, nothing more to do when no lane has any, and
// per metric the lane's partial result, combined across the wave (the DPP scans of vh_wave_scan.h) and added to
// the block's LDS table by ONE lane: one LDS update per (chunk, group, metric) in place of one per row and metric.
// A passing row that belongs to no id (a value outside the planned range, synced in since) raises VH_ERR_RANGE as vh_consume does: the
// host plans again.
// ROWS = 1: the ROW SINK stands in for the loop over ids (vh_plane_agg.h: vh_plane_agg_rows) — plans of more than VH_PLANE_AGG_MAX_GROUPS ids,
// which the loop cannot pay for. Walk, mask, loads and the end of the block are the same text; the sink's per-wave queue is static LDS of
// that instantiation alone.
template <int BLOCK, int SCOPE, int ROWS>
__global__ __launch_bounds__(BLOCK) void scan_agg_planes_kernel(const VhPlanDev P, const VhBitsProg* __restrict__ B, const VhPlaneAggDesc* __restrict__ D,
                                                                const VhSlicedPlanes F, const VhSlicedPlanes V, uint32_t chunks_per_seg) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  vh_scan_table_init<VH_MODE_DENSE_LDS, BLOCK>(P, lds);

  const uint32_t need = D->need, care = D->care, has_filter = D->has_filter;
  const uint64_t valid = D->valid;
  const uint32_t G = (uint32_t)P.G;                    // <= VH_PLANE_AGG_MAX_GROUPS (ROWS = 0)
  uint16_t* q = nullptr;
  if constexpr (ROWS) {
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
    const uint32_t mask = has_filter ? vh_sliced_mask(*B, F, seg, base, seg_rows, lane) : vh_sliced_tail_mask(row_l, seg_rows);
    npassed32 += __popc(mask);
    if (__ballot(mask != 0u) == 0ull) continue;

    uint32_t v[VH_BITS_MAX_FIELD];
#pragma unroll
    for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) v[p] = 0u;
    if (mask) {      // (mask != 0: the word begins below the snapshot)
      const char* planes = V.planes + (uint64_t)seg * V.stride;      // (uniform: a plane's address is a scalar, the lane adds its word's 32-bit offset)
      const uint32_t woff = (uint32_t)(row_l >> 5) * 4u;
#pragma unroll
      for (int p = 0; p < VH_BITS_MAX_FIELD; ++p)
        if ((need >> p) & 1u) v[p] = VH_BITS_LOAD(planes + (uint64_t)p * V.pitch + woff);
    }

    if constexpr (ROWS) range_err |= vh_plane_agg_rows(P, D, lds, v, mask, lane, q);      // (vh_plane_agg.h: one LDS update per surviving row and metric)
    else range_err |= vh_plane_agg_groups(P, D, care, valid, G, lds, v, mask, lane);      // (vh_plane_agg.h: the loop over the group ids, shared with the batch kernel)
  }

  if (__ballot(range_err) != 0ull && lane == 0) atomicOr(P.counters + 2, VH_ERR_RANGE);
  unsigned long long npassed = npassed32;
  for (int off = 32; off > 0; off >>= 1) npassed += __shfl_down(npassed, off);
  vh_scan_block_end(P, npassed, 0ull, 0ull, 0u);
  vh_scan_table_flush<VH_MODE_DENSE_LDS, BLOCK, SCOPE>(P, lds);
}

void vh_launch_scan_planes(const VhPlanDev& P, const VhPlaneAggRef& A, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private) {
  constexpr int BLOCK = 256;       // (at 1024 threads a lane may hold 128 registers, a few fewer than the filter interpreter and the 32 plane words take: QueryBuild::decompose_work)
  vh_with_scope(xcd_private, [&](auto scope) {
    constexpr int SCOPE = decltype(scope)::value;
    if (A.rows) {
      L.named("scan_agg_planes_rows_kernel<%d, %d>", BLOCK, SCOPE);
      vh_launch_or_ask(L, scan_agg_planes_kernel<BLOCK, SCOPE, 1>, BLOCK, true, P, A.B, A.D, A.F, A.V, chunks_per_seg);
    } else {
      L.named("scan_agg_planes_kernel<%d, %d>", BLOCK, SCOPE);
      vh_launch_or_ask(L, scan_agg_planes_kernel<BLOCK, SCOPE, 0>, BLOCK, true, P, A.B, A.D, A.F, A.V, chunks_per_seg);
    }
  });
}
