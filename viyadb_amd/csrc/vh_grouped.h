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
