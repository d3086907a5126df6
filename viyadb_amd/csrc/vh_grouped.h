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
