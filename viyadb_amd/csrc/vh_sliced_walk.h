// vh_sliced_walk.h — how the readers of the BIT-SLICED predicate planes (VhPredPack::sliced) share the rows out: which wave takes which
// 2048-row chunk, and which bits of a lane's plane word count under a snapshot. Plain C++ for host and device, like vh_bits_eval.h: the
// select kernels (vh_small_kernels.h) and the pre-built aggregate scan over the planes (vh_scan_sliced.hip) include it, and a host-compiled
// check runs both rules over every row of small tables (tests/sliced_walk_host.cc).
//
// A chunk is 2048 consecutive rows of one segment: 64 plane words, lane l of the wave owns word l (rows 32 l .. 32 l + 31 of the chunk, row
// 32 l + i being bit i). Chunks are numbered segment by segment, chunks_per_seg to a segment whatever its rows (the select kernels'
// counts[] are indexed by that number).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VH_WALK_FN __host__ __device__ __forceinline__
#else
#define VH_WALK_FN inline
#endif

#define VH_SLICED_CHUNK_ROWS 2048u

// A wave's walk over the chunks, as (segment, chunk of the segment): chunk waves * block + wave first, then every (waves * blocks)-th. Stepped
// as the pair: a 64-bit division per chunk would cost as much as the evaluation of a narrow field.
struct VhChunkWalk {
  uint32_t seg, k, step_seg, step_k, cps;
  // block / blocks: the block's index and the grid's size; waves: waves per block; wave: this wave's index in its block
  VH_WALK_FN VhChunkWalk(uint32_t block, uint32_t blocks, uint32_t waves, uint32_t wave, uint32_t chunks_per_seg) : cps(chunks_per_seg) {
    const uint32_t c0 = block * waves + wave, stride = blocks * waves;
    seg = c0 / cps; k = c0 - seg * cps;
    step_seg = stride / cps; step_k = stride - step_seg * cps;
  }
  VH_WALK_FN void next() { seg += step_seg; k += step_k; if (k >= cps) { k -= cps; ++seg; } }
  VH_WALK_FN uint64_t chunk() const { return (uint64_t)seg * cps + k; }
  VH_WALK_FN uint64_t base() const { return (uint64_t)k * VH_SLICED_CHUNK_ROWS; }      // first row of the chunk in its segment
};

// The tail rule. The plane word that begins at row `row_l` of a segment whose snapshot holds `seg_rows` rows: the bits of its rows below
// seg_rows. 0: the word begins at or beyond the snapshot and IS NOT READ (a skipped segment, seg_rows == 0, is never touched); the word
// that straddles seg_rows keeps its low seg_rows - row_l bits — the planes' bits beyond a snapshot are those of real rows.
VH_WALK_FN uint32_t vh_sliced_tail_mask(uint64_t row_l, uint32_t seg_rows) {
  if (row_l >= seg_rows) return 0u;
  const uint64_t left = seg_rows - row_l;
  return left < 32u ? (1u << (uint32_t)left) - 1u : ~0u;
}
