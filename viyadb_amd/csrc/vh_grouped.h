// vh_grouped.h — where a row's record lies in the GROUPED form of a 4-byte bit-record projection (VhGrouped, vhh_table.h).
//
// The grouped form keeps every tile of VH_GROUP_TILE = 2048 rows (one wave step of the bit-sliced scan: 64 lanes x 32 rows) stable-sorted
// by the value of one narrow predicate column c: the record of row r lies at
//     tile_base + start[value(r)] + (rows r' < r of the tile with value(r') == value(r)),
// start[v] = rows of the tile whose value is below v (a uint16 per value, the tile's header). A query with `c == literal` in its
// conjunction then finds its survivors' records in ONE run of consecutive lines per tile instead of all over it.
//
// A "lane" owns 32 consecutive rows of the tile (lane l: rows 32 l .. 32 l + 31); with
//     eq      the lane's 32-bit mask of rows whose value is v,
//     before  the sum of popcount(eq) over the lanes below it (an exclusive prefix),
// the place of the lane's row `bit` (which must be set in eq) is vh_grouped_pos(). The builder (group_bits_kernel, vh_small_kernels.h)
// and the scan (vj_scan's grouped push, vh_jit_body.h) BOTH call this function and nothing else, so the two cannot drift apart;
// tests/grouped_pos_host.cc runs it as plain C++ over synthetic tiles.
//
// The SUB-SORTED form (VhGrouped::sub_col >= 0; the second half of this file) orders every tile by (grouping value, sub key, row) instead,
// the sub key being the field the bit-sliced projection keeps of one range-compared column. start[] means the same; a row's place no longer
// follows from the row-order masks (vh_grouped_pos does not apply), so the form is read through its clustered planes only. Inside a run the
// keys ascend, so the places that can pass a range leaf on the sub column are one stretch of the run: 64 boundary keys per tile, kfirst[w] =
// the key at place 32 w, let the scan cut the run down to the words of that stretch (vh_gsub_trim). tests/gsub_host.cc runs all of it as plain C++.
#pragma once
#include <stdint.h>

#define VH_GROUP_TILE 2048u
#define VH_GROUP_MAX_BITS 4          // the grouping column's field: at most 16 values, 32 bytes of header per tile

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__HIP__)
#define VH_GROUP_HD __host__ __device__ __forceinline__
#else
#define VH_GROUP_HD inline
#endif

// rows of the lane below `bit` that share the value (bit < 32)
VH_GROUP_HD uint32_t vh_grouped_rank(uint32_t eq, uint32_t bit) { return (uint32_t)__builtin_popcount(eq & ((1u << bit) - 1u)); }
// the record's place inside its tile
VH_GROUP_HD uint32_t vh_grouped_pos(uint32_t eq, uint32_t before, uint32_t start, uint32_t bit) { return start + before + vh_grouped_rank(eq, bit); }
// bytes of a tile's header, and where the header of tile `tile` begins inside a segment's share of the header arena
VH_GROUP_HD uint32_t vh_grouped_hdr_bytes(uint32_t bits) { return 2u << bits; }
VH_GROUP_HD uint64_t vh_grouped_hdr_off(uint32_t tile, uint32_t bits) { return (uint64_t)tile * vh_grouped_hdr_bytes(bits); }

// ---- CLUSTERED predicate planes (VhGrouped::planes): the bits of every OTHER column of the bit-sliced predicate projection, kept per tile in
// the tile's grouped order — bit `place & 31` of word `place >> 5` belongs to the row whose record lies at `place`. Field order and bit order
// are the row-order planes' with the grouping column's field taken out (vh_gplanes_squeeze). Inside a tile the storage is WORD-major: the
// dwords of all planes for word w lie side by side (G dwords, G = the planes rounded up to a multiple of 4: a word group is 16-byte aligned),
// so the run [start[literal], end) of a tile is one contiguous stretch of (words of the run) x 4 G bytes. A tile's block is 256 G bytes;
// places at or beyond the tile's valid rows hold zeros. The builder (group_bits_kernel) and the scan (vj_scan_gplanes, vh_jit_body.h) both
// go through these functions; tests/gplanes_host.cc runs them as plain C++.
#define VH_GROUP_WORDS (VH_GROUP_TILE / 32u)
// dwords of a word group for `nplanes` planes
VH_GROUP_HD uint32_t vh_gplanes_group(uint32_t nplanes) { return (nplanes + 3u) & ~3u; }
// bytes of a tile's block, and of a segment's share of the arena (whole tiles)
VH_GROUP_HD uint64_t vh_gplanes_tile_bytes(uint32_t G) { return (uint64_t)VH_GROUP_WORDS * 4u * G; }
VH_GROUP_HD uint64_t vh_gplanes_seg_bytes(uint64_t segment_rows, uint32_t G) { return (segment_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE * vh_gplanes_tile_bytes(G); }
// byte offset of word `word` of tile `tile` inside a segment's share
VH_GROUP_HD uint64_t vh_gplanes_off(uint32_t tile, uint32_t word, uint32_t G) { return ((uint64_t)tile * VH_GROUP_WORDS + word) * 4u * G; }
// the words that cover places [start, end): first .. last (exclusive); an empty run has none
VH_GROUP_HD uint32_t vh_gplanes_first_word(uint32_t start) { return start >> 5; }
VH_GROUP_HD uint32_t vh_gplanes_last_word(uint32_t start, uint32_t end) { return start < end ? (end + 31u) >> 5 : start >> 5; }
// the places of word `word` that lie inside [start, end)
VH_GROUP_HD uint32_t vh_gplanes_word_mask(uint32_t word, uint32_t start, uint32_t end) {
  const uint32_t lo = word * 32u, hi = lo + 32u;
  if (start >= end || end <= lo || start >= hi) return 0u;
  const uint32_t from = start > lo ? start - lo : 0u, to = end < hi ? end - lo : 32u;       // 0 <= from < to <= 32
  return (to == 32u ? ~0u : (1u << to) - 1u) & ~((1u << from) - 1u);
}
// a row's field word with the grouping column's field (goff, gbits) taken out: the fields above it move down
VH_GROUP_HD uint32_t vh_gplanes_squeeze(uint32_t word, uint32_t goff, uint32_t gbits) {
  const uint32_t low = word & ((1u << goff) - 1u);
  return goff + gbits >= 32u ? low : low | ((word >> (goff + gbits)) << goff);
}
// ... and where plane `plane` of the row-order projection lies in a word group (planes of the grouping field have no place)
VH_GROUP_HD uint32_t vh_gplanes_plane(uint32_t plane, uint32_t goff, uint32_t gbits) { return plane < goff ? plane : plane - gbits; }

// ---- the SUB-SORTED form: tiles ordered by (grouping value, sub key, row). The builder sorts vh_gsub_sort_word() of the tile's rows as plain
// integers (the row bits make the order stable and total); rows at or beyond the tile's valid rows sort behind every valid one.
#define VH_GSUB_MAX_BITS 16u         // the sub column's field: its boundary keys are uint16
#define VH_GSUB_KEYS_BYTES (2u * VH_GROUP_WORDS)       // a tile's boundary keys: 128 bytes
// relations a run can be trimmed by: the values of vh_relop (include/viya_hip.h), which has NE = 1 between them
enum { VH_GSUB_EQ = 0, VH_GSUB_LT = 2, VH_GSUB_LE = 3, VH_GSUB_GT = 4, VH_GSUB_GE = 5 };
VH_GROUP_HD bool vh_gsub_op_ok(int op) { return op == VH_GSUB_EQ || op == VH_GSUB_LT || op == VH_GSUB_LE || op == VH_GSUB_GT || op == VH_GSUB_GE; }
// the composite key of a row (at most VH_GROUP_MAX_BITS + VH_GSUB_MAX_BITS = 20 bits), and the word the builder sorts (row < 2048)
VH_GROUP_HD uint32_t vh_gsub_key(uint32_t gval, uint32_t sub, uint32_t sub_bits) { return (gval << sub_bits) | sub; }
VH_GROUP_HD uint32_t vh_gsub_sort_word(uint32_t key, uint32_t row, bool valid) { return valid ? (key << 11) | row : 0x80000000u | row; }
VH_GROUP_HD uint32_t vh_gsub_sorted_row(uint32_t sort_word) { return sort_word & (VH_GROUP_TILE - 1u); }
VH_GROUP_HD uint32_t vh_gsub_sorted_sub(uint32_t sort_word, uint32_t sub_bits) { return (sort_word >> 11) & ((1u << sub_bits) - 1u); }
// where a segment's boundary keys begin in its share of the header arena (behind the headers of its `tiles` tiles, 64-byte aligned), the
// share's bytes with them, and where tile `tile`'s 64 keys lie
VH_GROUP_HD uint64_t vh_gsub_keys_off(uint64_t tiles, uint32_t bits) { return (tiles * vh_grouped_hdr_bytes(bits) + 63u) / 64u * 64u; }
VH_GROUP_HD uint64_t vh_gsub_hdr_stride(uint64_t tiles, uint32_t bits) { return vh_gsub_keys_off(tiles, bits) + tiles * VH_GSUB_KEYS_BYTES; }
VH_GROUP_HD uint64_t vh_gsub_tile_off(uint64_t tiles, uint32_t bits, uint32_t tile) { return vh_gsub_keys_off(tiles, bits) + (uint64_t)tile * VH_GSUB_KEYS_BYTES; }
// The stretch [*s2, *e2) of the run [start, end) that holds every place whose key satisfies `key op lit` (lit in field space). kfirst: the
// tile's boundary keys; only entries of places inside the run are read. Keys ascend along the run, so a word w that begins inside the run
// (32 w >= start) with kfirst[w] already past the literal ends the stretch at 32 w, and one with kfirst[w] still short of it lets the stretch
// begin at 32 w — both found by binary search over the run's words (at most six steps each). A trimmed side is a multiple of 32, the other
// the run's own bound; the stretch is conservative (the leaf is still evaluated on every word kept), never tight.
VH_GROUP_HD void vh_gsub_trim(const uint16_t* kfirst, uint32_t start, uint32_t end, int op, uint32_t lit, uint32_t* s2, uint32_t* e2) {
  *s2 = start; *e2 = end;
  if (start >= end || !vh_gsub_op_ok(op)) return;
  const uint32_t w0 = (start + 31u) >> 5, w1 = (end + 31u) >> 5;       // the words that BEGIN inside the run: w0 .. w1 (exclusive)
  if (op == VH_GSUB_LT || op == VH_GSUB_LE || op == VH_GSUB_EQ) {      // the back: the first such word whose first key is past the literal
    uint32_t lo = w0, hi = w1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t k = kfirst[mid];
      if (op == VH_GSUB_LT ? k >= lit : k > lit) hi = mid; else lo = mid + 1u;
    }
    if (lo < w1) *e2 = lo * 32u;
  }
  if (op == VH_GSUB_GT || op == VH_GSUB_GE || op == VH_GSUB_EQ) {      // the front: the last such word whose first key is still short of it
    uint32_t lo = w0, hi = w1;                                          // (lo: the first word whose first key is NOT short)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t k = kfirst[mid];
      if (op == VH_GSUB_GT ? k <= lit : k < lit) lo = mid + 1u; else hi = mid;
    }
    if (lo > w0) *s2 = (lo - 1u) * 32u;
  }
  if (*s2 > *e2) *s2 = *e2;
}

// ---- tile groups that SPAN segments (VhJitShape::gp_span): the clustered scan keeps, per tile, values with the segment already folded in, so
// that a group of tiles — and the queue of survivors behind it — may cross segments. With rec_units = (the records' segment stride) / 4 and
// pl_units = (the planes' segment stride) / 16:
//     a record's table-wide INDEX    seg * rec_units + place in the segment          (byte offset from the arena's base: 4 x index),
//     a tile's planes, in 16-byte units    seg * pl_units + tile * (a tile's block / 16),
// both in 32 bits. The host lets a plan span when the strides divide and no index or unit of the scanned segments reaches `bound` (2^32; a
// test knob lowers it); tests/gspan_host.cc checks the sums against the per-segment addresses as plain C++.
#define VH_GSPAN_BOUND (1ull << 32)
VH_GROUP_HD bool vh_gspan_ok(uint64_t nseg, uint64_t rec_stride, uint64_t planes_stride, uint64_t bound) {
  if (rec_stride % 4u || planes_stride % 16u || bound > VH_GSPAN_BOUND) return false;
  return nseg * (rec_stride / 4u) <= bound && nseg * (planes_stride / 16u) <= bound;
}
VH_GROUP_HD uint32_t vh_gspan_rec(uint32_t seg, uint32_t rec_units, uint32_t place) { return seg * rec_units + place; }
VH_GROUP_HD uint32_t vh_gspan_tile(uint32_t seg, uint32_t pl_units, uint32_t tile, uint32_t G) { return seg * pl_units + tile * (VH_GROUP_WORDS * (G / 4u)); }
// byte offset, from the planes' base, of word `word` of the tile whose planes begin at unit `tile_unit` (G is a multiple of 4)
VH_GROUP_HD uint64_t vh_gspan_word_off(uint32_t tile_unit, uint32_t word, uint32_t G) { return (uint64_t)(tile_unit + word * (G / 4u)) * 16u; }
