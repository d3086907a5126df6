// gspan_host.cc — the arithmetic of tile groups that span segments (viyadb_amd/csrc/vh_grouped.h, vh_gspan_*) as plain C++
// (tests/test_gspan_host.py compiles this plain and with -fsanitize=address,undefined and runs it).
//
// The spanning scan replaces "segment, place" by one 32-bit record index and "segment, tile, word" by one 32-bit count of 16-byte units.
// For three table geometries and several strides the program walks every (segment, tile, place) and every (segment, tile, word) and checks
// that 4 x index and 16 x units are the byte offsets the per-segment formulas give (base + seg * stride + ...), in 64-bit arithmetic. Then
// the host's condition: strides that do not divide are refused, the bound is met exactly and missed by one, and 2^32 itself is the limit.
#include <cstdint>
#include <cstdio>

#include "vh_grouped.h"

struct Geometry { const char* name; uint32_t nseg; uint64_t seg_rows; };

static bool walk(const Geometry& g, uint32_t G, uint64_t rec_pad, uint64_t pl_pad) {
  const uint64_t tiles = (g.seg_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE;
  const uint64_t rec_stride = tiles * VH_GROUP_TILE * 4u + rec_pad, pl_stride = vh_gplanes_seg_bytes(g.seg_rows, G) + pl_pad;
  if (!vh_gspan_ok(g.nseg, rec_stride, pl_stride, VH_GSPAN_BOUND)) { printf("%s: G %u refused\n", g.name, G); return false; }
  const uint32_t rec_units = (uint32_t)(rec_stride / 4u), pl_units = (uint32_t)(pl_stride / 16u);
  for (uint32_t seg = 0; seg < g.nseg; ++seg)
    for (uint32_t tile = 0; tile < tiles; ++tile) {
      const uint32_t base = tile * VH_GROUP_TILE;
      const uint64_t left = g.seg_rows - base, valid = left < VH_GROUP_TILE ? left : VH_GROUP_TILE;
      const uint32_t first = vh_gspan_rec(seg, rec_units, base);
      for (uint32_t place = 0; place < valid; ++place) {
        const uint64_t want = (uint64_t)seg * rec_stride + ((uint64_t)base + place) * 4u;
        if ((uint64_t)(first + place) * 4u != want) { printf("%s: record of segment %u tile %u place %u at %llu, not %llu\n", g.name, seg, tile, place, (unsigned long long)(first + place) * 4ull, (unsigned long long)want); return false; }
      }
      const uint32_t unit = vh_gspan_tile(seg, pl_units, tile, G);
      for (uint32_t word = 0; word < VH_GROUP_WORDS; ++word) {
        const uint64_t want = (uint64_t)seg * pl_stride + vh_gplanes_off(tile, word, G);
        if (vh_gspan_word_off(unit, word, G) != want) { printf("%s: word %u of segment %u tile %u at %llu, not %llu\n", g.name, word, seg, tile, (unsigned long long)vh_gspan_word_off(unit, word, G), (unsigned long long)want); return false; }
      }
    }
  return true;
}

static bool bounds() {
  bool ok = true;
  auto expect = [&](bool got, bool want, const char* what) { if (got != want) { printf("bound: %s\n", what); ok = false; } };
  expect(vh_gspan_ok(420, 40960, 25600, VH_GSPAN_BOUND), true, "the 420-segment table is refused under 2^32");
  expect(vh_gspan_ok(420, 40960, 25600, 420ull * 10240), true, "a bound met exactly is refused");
  expect(vh_gspan_ok(420, 40960, 25600, 420ull * 10240 - 1), false, "a bound missed by one record is accepted");
  expect(vh_gspan_ok(420, 4096, 25600, 420ull * 1600 - 1), false, "a bound missed by one unit of planes is accepted");
  expect(vh_gspan_ok(420, 40962, 25600, VH_GSPAN_BOUND), false, "a record stride that is no multiple of 4 is accepted");
  expect(vh_gspan_ok(420, 40960, 25608, VH_GSPAN_BOUND), false, "a planes stride that is no multiple of 16 is accepted");
  expect(vh_gspan_ok(1024, 4ull << 22, 16, VH_GSPAN_BOUND), true, "2^32 records are refused");                   // the largest index is 2^32 - 1
  expect(vh_gspan_ok(1025, 4ull << 22, 16, VH_GSPAN_BOUND), false, "more than 2^32 records are accepted");
  expect(vh_gspan_ok(1024, 4, 16ull << 22, VH_GSPAN_BOUND), true, "2^32 units of planes are refused");
  expect(vh_gspan_ok(1025, 4, 16ull << 22, VH_GSPAN_BOUND), false, "more than 2^32 units of planes are accepted");
  expect(vh_gspan_ok(1, 4, 16, VH_GSPAN_BOUND + 1), false, "a bound above 2^32 is accepted");
  expect(vh_gspan_ok(0, 4, 16, 0), true, "no segment at all is refused");
  return ok;
}

int main() {
  const Geometry geo[] = {{"5 x 1 000 000", 5, 1000000}, {"420 x 10 000", 420, 10000}, {"3 x 2 097 152", 3, 2097152}};
  int bad = 0;
  for (const Geometry& g : geo) {
    // C3's word group (20 dwords), the smallest (4), and strides padded by a line of records and an odd number of units
    const bool ok = walk(g, 20, 0, 0) && walk(g, 4, 128, 16) && walk(g, 12, 4, 16 * 7);
    printf("%s: %s\n", g.name, ok ? "ok" : "FAILED");
    bad += !ok;
  }
  const bool ok = bounds();
  printf("bounds: %s\n", ok ? "ok" : "FAILED");
  return bad || !ok ? 1 : 0;
}
