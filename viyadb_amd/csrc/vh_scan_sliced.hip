// The pre-built aggregate scan over the BIT-SLICED predicate planes: the filter program interpreted bit-serially (vh_bits_eval.h), 32 rows per
// lane and evaluation, in front of the pre-built sinks (vh_consume / vh_consume_fast). The third reader of the planes, beside the per-query
// compiled scan (vh_jit_body.h) and the select kernels (vh_small_kernels.h): for aggregates that no compiled kernel answers.
#include "vh_kernels.h"
#include "vh_launch.h"
#include "vh_sliced.h"

// VhPlanDev travels by value as for every scan kernel, the planes' place (VhSlicedPlanes) by value behind it. The program does not fit beside
// them: it lies in the plan block and is read through B (vh_sliced.h, VhSlicedRef).
static_assert(sizeof(VhPlanDev) + sizeof(VhBitsProg) + sizeof(VhSlicedPlanes) > 4096, "the program would fit the kernel arguments: pass it by value");
static_assert(sizeof(VhPlanDev) + sizeof(VhSlicedRef) + 16 <= 4096, "scan_agg_sliced_kernel: plan and planes together exceed the 4 KB of kernel arguments");

// A wave walks 2048-row chunks (VhChunkWalk: whatever BLOCK, P.unit_rows plays no part); lane l owns plane word l of the chunk and gets the pass
// mask of its 32 rows in one evaluation — up to 2048 survivors a step. The wave's queue is the compacting kernels' (VhScanCfg::kQueueCap),
// so the mask is consumed in eight slices of four bits per lane, at most 256 survivors each, with a drain whenever 64 are queued; entries are
// row numbers of the current segment, flushed when the wave leaves it. Everything behind the queue is the sink of the kernel this one stands
// in for: scan_agg_kernel's for the LDS, global and hash organisations, vh_scan_fast_body's for DENSE_PART.
template <int MODE, int BLOCK, int SCOPE>
__global__ __launch_bounds__(BLOCK) void scan_agg_sliced_kernel(const VhPlanDev P, const VhBitsProg* __restrict__ B, const VhSlicedPlanes L, uint32_t chunks_per_seg) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  typedef VhScanCfg<BLOCK> C;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform, and known to be: chunk, segment and plane addresses are scalars)
  uint32_t* q = reinterpret_cast<uint32_t*>(lds + ((MODE == VH_MODE_DENSE_LDS || MODE == VH_MODE_HASH) ? P.lds_bytes : 0)) + wave * C::kQueueCap;
  VhLdsHashWave H{0u, 0u, false, 0ull};
  VhPartWave W;
  VhPartTile T;
  if (MODE == VH_MODE_DENSE_PART) vh_part_tile_init(P, lds, T, W);
  vh_scan_table_init<MODE, BLOCK>(P, lds);

  const uint64_t xoff = (MODE == VH_MODE_DENSE_GLOBAL && P.nxcd > 1) ? (uint64_t)(vh_xcc_id() % P.nxcd) * P.xcd_stride : 0;
  uint32_t npassed32 = 0;                    // per lane: 32 rows of every chunk this wave takes (< 2^32 for any table a launch covers)
  unsigned long long nfresh = 0;
  uint32_t cnt = 0;                          // queued survivors of this wave (wave-uniform)

  for (VhChunkWalk K(blockIdx.x, gridDim.x, (uint32_t)C::kWaves, wave, chunks_per_seg); K.seg < P.nseg;) {
    const uint32_t seg = K.seg;
    const uint64_t base = K.base();
    const uint32_t seg_rows = P.seg_rows[seg];
    uint32_t mask = 0u;
    if (base < seg_rows) mask = vh_sliced_mask(*B, L, seg, base, seg_rows, lane);      // (a skipped segment, and the chunks beyond a snapshot: not touched)
    npassed32 += __popc(mask);
    const uint32_t row_l = (uint32_t)base + (uint32_t)lane * 32u;
    K.next();
    const bool last = K.seg != seg || K.seg >= P.nseg;      // the wave leaves the segment: queue entries are rows of the current one
    // One textual drain for the eight slices and for the flush at a segment's end (k == 8), as in vh_scan_fast_body.
#pragma unroll 1
    for (int k = 0; k <= 8; ++k) {
      bool flush = false;
      if (k < 8) {
        const uint32_t mk = (mask >> (4 * k)) & 0xFu;
        if (__ballot(mk != 0) == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool b = (mk >> j) & 1u;
          const uint64_t bal = __ballot(b);
          if (b) q[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = row_l + 4u * k + j;
          cnt += __popcll(bal);
        }
        __builtin_amdgcn_wave_barrier();
      } else {
        flush = last;
      }
      while (cnt >= 64 || (flush && cnt)) {
        const uint32_t take = cnt >= 64 ? 64u : cnt;
        cnt -= take;
        const bool act = (uint32_t)lane < take;
        const uint32_t r = act ? q[cnt + lane] : 0u;
        if constexpr (MODE == VH_MODE_DENSE_PART) vh_consume_fast<VH_MODE_DENSE_PART, __HIP_MEMORY_SCOPE_AGENT, 0>(P, seg, r, act, lds, xoff, nfresh, W, T, H);
        else vh_consume<MODE, SCOPE>(P, seg, r, act, lds, xoff, nfresh, H);
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (MODE == VH_MODE_HASH && H.dead) break;     // this wave saw the table overflow: the attempt is void (see scan_agg_kernel)
  }

  if (MODE == VH_MODE_DENSE_PART) vh_part_tile_finish(P, T, lane);
  if (MODE == VH_MODE_HASH) vh_hot_flush(P, H.hot);      // what the wave still keeps of its hot group
  unsigned long long npassed = npassed32;
  for (int off = 32; off > 0; off >>= 1) { npassed += __shfl_down(npassed, off); H.npairs += __shfl_down(H.npairs, off); }
  vh_scan_block_end(P, npassed, nfresh, H.npairs, MODE == VH_MODE_DENSE_PART ? vh_part_wave_end(P, W) : 0u);
  vh_scan_table_flush<MODE, BLOCK, SCOPE>(P, lds);
}

template <int MODE, int BLOCK>
static void launch(const VhPlanDev& P, const VhSlicedRef& A, uint32_t cps, const VhScanLaunch& L, bool xcd_private) {
  vh_with_scope(xcd_private, [&](auto scope) {
    constexpr int SCOPE = decltype(scope)::value;
    L.named("scan_agg_sliced_kernel<%d, %d, %d>", MODE, BLOCK, SCOPE);
    vh_launch_or_ask(L, scan_agg_sliced_kernel<MODE, BLOCK, SCOPE>, BLOCK, true, P, A.B, A.L, cps);
  });
}

void vh_launch_scan_sliced(int mode, const VhPlanDev& P, const VhSlicedRef& A, uint32_t chunks_per_seg, const VhScanLaunch& L, bool xcd_private) {
  if (mode == VH_MODE_DENSE_LDS) launch<VH_MODE_DENSE_LDS, 1024>(P, A, chunks_per_seg, L, xcd_private);
  else if (mode == VH_MODE_DENSE_GLOBAL) launch<VH_MODE_DENSE_GLOBAL, 256>(P, A, chunks_per_seg, L, xcd_private);
  else if (mode == VH_MODE_DENSE_PART) launch<VH_MODE_DENSE_PART, 256>(P, A, chunks_per_seg, L, false);      // (tuples and the hash table have no private copies)
  else launch<VH_MODE_HASH, 256>(P, A, chunks_per_seg, L, false);
}
