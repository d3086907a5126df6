// The chunk walk and the tail-mask rule of the readers of the bit-sliced predicate planes (viyadb_amd/csrc/vh_sliced_walk.h), run on the CPU
// exactly as the kernels run them: every (block, wave) of a grid walks its chunks, every lane of the wave asks for the bits of its plane word.
// Asserted for every combination of segments, chunks per segment, grid size, waves per block and snapshot: every row below seg_rows of every
// segment is covered by exactly one (block, wave, lane, bit); no word that begins at or beyond seg_rows is asked for; chunk() is
// segment * chunks_per_seg + chunk of the segment, every such index taken exactly once (what the select kernels' counts[] are indexed by).
// Stand-alone: g++ -std=c++17 -I viyadb_amd/csrc tests/sliced_walk_host.cc (tests/test_sliced_walk_host.py, plain and under ASan + UBSan).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vh_sliced_walk.h"

#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fprintf(stderr, "\n");                                         \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static unsigned long long g_rows = 0, g_words = 0, g_configs = 0;

static void run(uint32_t nseg, uint32_t cps, uint32_t blocks, uint32_t waves, const std::vector<uint32_t>& seg_rows) {
  const uint32_t capacity = cps * VH_SLICED_CHUNK_ROWS;
  // exact-size heap blocks: a row or a chunk outside them is an error under the sanitizer as well
  std::vector<std::vector<uint8_t>> cover(nseg);
  for (uint32_t s = 0; s < nseg; ++s) cover[s].assign(seg_rows[s], 0);
  std::vector<uint8_t> taken((size_t)nseg * cps, 0);
  for (uint32_t block = 0; block < blocks; ++block) {
    for (uint32_t wave = 0; wave < waves; ++wave) {
      uint64_t before = 0;
      bool first = true;
      for (VhChunkWalk W(block, blocks, waves, wave, cps); W.seg < nseg; W.next()) {
        CHECK(W.k < cps, "chunk %u of a segment of %u", W.k, cps);
        const uint64_t c = W.chunk();
        CHECK(c == (uint64_t)W.seg * cps + W.k, "chunk() %llu for segment %u, chunk %u", (unsigned long long)c, W.seg, W.k);
        CHECK(c < taken.size(), "chunk %llu of %zu", (unsigned long long)c, taken.size());
        CHECK(first ? c == (uint64_t)block * waves + wave : c == before + (uint64_t)blocks * waves, "the walk's stride: %llu after %llu", (unsigned long long)c, (unsigned long long)before);
        first = false; before = c;
        CHECK(++taken[c] == 1, "chunk %llu taken twice", (unsigned long long)c);
        const uint64_t base = W.base();
        CHECK(base == (uint64_t)W.k * VH_SLICED_CHUNK_ROWS && base < capacity, "base %llu", (unsigned long long)base);
        const uint32_t rows = seg_rows[W.seg];
        if (base >= rows) continue;                      // (the kernels skip such a chunk: a skipped segment is not touched)
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t row_l = base + (uint64_t)lane * 32u;
          const uint32_t keep = vh_sliced_tail_mask(row_l, rows);
          CHECK((keep != 0u) == (row_l < rows), "word at row %llu of %u rows: mask %08x", (unsigned long long)row_l, rows, keep);      // asked for <=> it begins below seg_rows
          if (!keep) continue;
          ++g_words;
          for (uint32_t i = 0; i < 32; ++i) {
            if (!((keep >> i) & 1u)) { CHECK(row_l + i >= rows, "row %llu of %u masked away", (unsigned long long)(row_l + i), rows); continue; }
            CHECK(row_l + i < rows, "row %llu beyond %u", (unsigned long long)(row_l + i), rows);
            CHECK(++cover[W.seg][row_l + i] == 1, "segment %u row %llu covered twice", W.seg, (unsigned long long)(row_l + i));
          }
        }
      }
    }
  }
  for (size_t c = 0; c < taken.size(); ++c) CHECK(taken[c] == 1, "chunk %zu taken %u times", c, taken[c]);
  for (uint32_t s = 0; s < nseg; ++s)
    for (uint32_t r = 0; r < seg_rows[s]; ++r) { CHECK(cover[s][r] == 1, "segment %u row %u covered %u times (nseg %u cps %u blocks %u waves %u)", s, r, cover[s][r], nseg, cps, blocks, waves); ++g_rows; }
  ++g_configs;
}

int main() {
  // the mask itself at the edges
  CHECK(vh_sliced_tail_mask(0, 0) == 0u && vh_sliced_tail_mask(32, 32) == 0u && vh_sliced_tail_mask(64, 33) == 0u, "words at or beyond the snapshot");
  CHECK(vh_sliced_tail_mask(0, 1) == 1u && vh_sliced_tail_mask(0, 31) == 0x7FFFFFFFu && vh_sliced_tail_mask(0, 32) == ~0u && vh_sliced_tail_mask(32, 33) == 1u, "straddling words");
  CHECK(vh_sliced_tail_mask(0, 0xFFFFFFFFu) == ~0u && vh_sliced_tail_mask(0xFFFFFFE0ull, 0xFFFFFFFFu) == 0x7FFFFFFFu && vh_sliced_tail_mask(0x100000000ull, 0xFFFFFFFFu) == 0u, "the largest snapshot");
  const uint32_t segs[] = {1, 3, 7}, chunks[] = {1, 3, 4}, wavesv[] = {4, 16};
  for (uint32_t nseg : segs)
    for (uint32_t cps : chunks) {
      const uint32_t capacity = cps * VH_SLICED_CHUNK_ROWS;
      const uint32_t draw[] = {0, 1, 31, 32, 33, 2047, 2048, 2049, 5000, capacity};
      const uint32_t ndraw = sizeof(draw) / sizeof(draw[0]);
      const uint32_t grids[] = {1, 2, 5, 304, nseg * cps + 3};      // (the last: more blocks than chunks, whatever the waves per block)
      for (uint32_t blocks : grids)
        for (uint32_t waves : wavesv)
          for (uint32_t shift = 0; shift < ndraw; ++shift) {      // every segment takes every value once
            std::vector<uint32_t> rows(nseg);
            for (uint32_t s = 0; s < nseg; ++s) { const uint32_t v = draw[(s * 3 + shift) % ndraw]; rows[s] = v < capacity ? v : capacity; }
            run(nseg, cps, blocks, waves, rows);
          }
    }
  std::printf("ok: %llu configurations, %llu rows covered once each, %llu plane words asked for\n", g_configs, g_rows, g_words);
  return 0;
}
