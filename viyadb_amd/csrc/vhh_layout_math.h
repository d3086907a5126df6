// vhh_layout_math.h — the arithmetic of the derived layouts that needs no device: which rows a layout has to re-derive (the job cutter), the
// value range of a column over the mirrored segments, and what a range means for a layout (stored bytes, bits, narrow width). Plain C++ with
// no HIP in it: the library includes it (vh_small_kernels.h for VhJob, vhh_table.h / vhh_derived.h for the rest) and tests/layout_math_host.cc
// compiles it with g++ under the sanitizers and checks it against brute force.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "../../include/viya_hip.h"
#include "vh_grouped.h"

// One unit of work of the derived-layout kernels: rows [first, first + count) of segment `seg` (first a multiple of 256, count a multiple of 4
// and at most VH_JOB_ROWS), of which the segment holds `seg_rows`. The host cuts what changed since a layout was last refreshed — whole
// segments when it is built, the row ranges an upsert batch touched afterwards (vh_table::journal) — into such jobs; one block each.
#define VH_JOB_ROWS 16384u
struct VhJob { uint32_t seg, first, count, seg_rows; };
// What a sync did to a segment's columns: rows [first, last) at sync epoch `epoch` (the table's journal; derived layouts replay it).
struct VhChange { uint64_t epoch; uint32_t seg, first, last; };

// ------------------------------------------------------------------------------------------------------------------- the job cutter
// The table's side of a refresh (journal entries ascending by epoch; entries at or below `floor` were dropped) and the layout's.
struct VhCutTable { const VhChange* journal; size_t njournal; uint64_t floor; const uint64_t* seg_mod; const uint64_t* seg_rows; uint32_t nseg; };
struct VhCutLayout { const uint64_t* seg_mod; size_t nseg_mod; uint64_t applied_epoch; uint64_t row_limit; };
// What a derived layout that was current at `applied_epoch` (per segment: at `seg_mod[s]`) has to re-derive, as jobs for its kernel: the
// row ranges journalled since, cut at 256-row boundaries, merged, and split into pieces of VH_JOB_ROWS; whole segments for a layout that
// is new, or so far behind that the journal no longer reaches back to it — those whose stamp differs from the table's. `row_limit`: rows a
// segment of the layout has room for (a projection's stride is padded to 256 rows, a narrow copy's to 64).
// whole_tiles (the grouped form: one changed row moves the places of its tile's rows behind it): the ranges widened to whole tiles of
// VH_GROUP_TILE rows, every tile once, one job per tile.
static inline void vh_cut_jobs(const VhCutTable& T, const VhCutLayout& L, bool whole_tiles, std::vector<VhJob>* jobs) {
  jobs->clear();
  std::vector<std::pair<uint64_t, uint64_t>> ranges;      // (seg << 32 | first, last)
  auto whole = [&](uint32_t s) { if (s < L.nseg_mod && L.seg_mod[s] != T.seg_mod[s]) ranges.emplace_back((uint64_t)s << 32, L.row_limit); };
  if (L.applied_epoch == 0 || L.applied_epoch < T.floor) {
    for (uint32_t s = 0; s < T.nseg; ++s) whole(s);
  } else {
    const VhChange* end = T.journal + T.njournal;
    const VhChange* it = std::upper_bound(T.journal, end, L.applied_epoch, [](uint64_t e, const VhChange& c) { return e < c.epoch; });
    for (; it != end; ++it) {
      if (it->seg >= T.nseg || it->seg >= L.nseg_mod) continue;
      if (L.seg_mod[it->seg] == 0) { whole(it->seg); continue; }          // a segment this layout never held (the table grew)
      const uint64_t a = it->first & ~255ull, b = std::min<uint64_t>(((uint64_t)it->last + 255) & ~255ull, L.row_limit);
      if (a < b) ranges.emplace_back(((uint64_t)it->seg << 32) | a, b);
    }
  }
  if (ranges.empty()) return;
  std::sort(ranges.begin(), ranges.end());
  size_t o = 0;
  for (size_t i = 1; i < ranges.size(); ++i) {
    if ((ranges[i].first >> 32) == (ranges[o].first >> 32) && (ranges[i].first & 0xFFFFFFFFull) <= ranges[o].second) ranges[o].second = std::max(ranges[o].second, ranges[i].second);
    else ranges[++o] = ranges[i];
  }
  ranges.resize(o + 1);
  for (const auto& r : ranges) {          // (merged and ascending: a tile two ranges share follows itself)
    const uint32_t seg = (uint32_t)(r.first >> 32), rows = (uint32_t)T.seg_rows[seg];
    const uint64_t a = r.first & 0xFFFFFFFFull, b = std::min(r.second, L.row_limit);
    if (!whole_tiles) {
      for (uint64_t f = a; f < b; f += VH_JOB_ROWS) jobs->push_back(VhJob{seg, (uint32_t)f, (uint32_t)std::min<uint64_t>(VH_JOB_ROWS, b - f), rows});
      continue;
    }
    for (uint64_t f = a / VH_GROUP_TILE * VH_GROUP_TILE; f < b; f += VH_GROUP_TILE)
      if (jobs->empty() || jobs->back().seg != seg || jobs->back().first != f) jobs->push_back(VhJob{seg, (uint32_t)f, VH_GROUP_TILE, rows});
  }
}

// ------------------------------------------------------------------------------------------------- value ranges and what they need
struct VhSegStat {          // order keys as produced by seg_minmax_kernel: unsigned values as they are, signed ones with the sign bit flipped
  uint64_t lo = ~0ull, hi = 0;
};
struct VhRange {            // the same over several segments; lo > hi: no rows yet
  uint64_t lo = ~0ull, hi = 0;
  bool empty() const { return lo > hi; }
  void add(uint64_t l, uint64_t h) { lo = std::min(lo, l); hi = std::max(hi, h); }
};
static inline VhRange vh_range_over(const VhSegStat* stats, size_t nseg) {
  VhRange r;
  for (size_t s = 0; s < nseg; ++s) {
    const VhSegStat& st = stats[s];
    if (st.lo > st.hi) continue;          // an empty segment adds nothing
    r.add(st.lo, st.hi);
  }
  return r;
}
static inline bool vh_elem_signed(int elem) { return elem == VH_I8 || elem == VH_I16 || elem == VH_I32 || elem == VH_I64; }
static inline bool vh_elem_float(int elem) { return elem == VH_F32 || elem == VH_F64; }
static inline int64_t vh_signed_of_key(uint64_t k) { return (int64_t)(k ^ (1ull << 63)); }      // (order key of a signed integer: the value with its sign bit flipped)

// Bytes the values of an integer column need in a compressed record: 1, 2, 4 or 8, never more than the element (`esize` bytes); the element
// size for floating point. No rows yet: 1 — anything fits, and a later value that does not voids the projection.
static inline int vh_range_stored_bytes(int elem, int esize, const VhRange& r) {
  if (vh_elem_float(elem) || esize == 1) return esize;
  if (r.empty()) return 1;
  int w;
  if (vh_elem_signed(elem)) {
    const int64_t a = vh_signed_of_key(r.lo), b = vh_signed_of_key(r.hi);
    w = (a >= INT8_MIN && b <= INT8_MAX) ? 1 : (a >= INT16_MIN && b <= INT16_MAX) ? 2 : (a >= INT32_MIN && b <= INT32_MAX) ? 4 : 8;
  } else {
    w = r.hi < 256 ? 1 : r.hi < 65536 ? 2 : r.hi <= 0xFFFFFFFFull ? 4 : 8;
  }
  return std::min(w, esize);
}
// Bits the values need as a bit field: 1..64, or 0 — no bit field for this column: floating point, a bitset, a negative value, or no rows
// yet. (A record projection takes "no rows yet" as the value 0, vh_range_of_zero; a predicate projection takes it as nothing to gain.)
static inline int vh_range_bits(int elem, const VhRange& r) {
  if (vh_elem_float(elem) || elem == VH_BITSET32 || elem == VH_BITSET64 || r.empty()) return 0;
  const bool sgn = vh_elem_signed(elem);
  if (sgn && vh_signed_of_key(r.lo) < 0) return 0;
  const uint64_t vmax = sgn ? (uint64_t)vh_signed_of_key(r.hi) : r.hi;
  int b = 1;
  while (b < 64 && (vmax >> b)) ++b;
  return b;
}
static inline VhRange vh_range_of_zero(int elem) {
  VhRange r;
  r.lo = r.hi = vh_elem_signed(elem) ? 1ull << 63 : 0;
  return r;
}
// Width of a narrow copy: 1 or 2 bytes, or 0 — not an unsigned 32-bit column, no rows yet, or the values need more than 16 bits.
static inline int vh_range_narrow_width(int elem, const VhRange& r) {
  if (elem != VH_U32 || r.empty()) return 0;
  return r.hi < 256 ? 1 : r.hi < 65536 ? 2 : 0;
}

// ---------------------------------------------------------------- which layouts leave when a byte budget is short (derived_make_room, vhh_derived.h)
// One entry per layout: every arena it holds (a projection's grouped form counted with it), the table's query tick at the last plan that read
// it (0: never), its serial, and whether it may leave at all — not pinned, and no plan of the current tick reads it.
struct VhEvictEntry { uint64_t bytes, last_use, serial; bool evictable; };
// The victims that free at least `deficit` bytes, as indices into `e`: the evictable entries by ascending (last_use, serial) — least recently
// used first, the older layout first among equals — and of that order the shortest prefix that covers the deficit. false: impossible — every
// evictable entry together frees less than the deficit; `victims` is then empty (nothing is evicted for a build that will not fit anyway).
static inline bool vh_evict_pick(const VhEvictEntry* e, size_t n, uint64_t deficit, std::vector<size_t>* victims) {
  victims->clear();
  if (!deficit) return true;
  std::vector<size_t> order;
  for (size_t i = 0; i < n; ++i) if (e[i].evictable) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return e[a].last_use != e[b].last_use ? e[a].last_use < e[b].last_use : e[a].serial != e[b].serial ? e[a].serial < e[b].serial : a < b;
  });
  uint64_t freed = 0;
  for (size_t i : order) {
    victims->push_back(i);
    if (e[i].bytes >= deficit - freed) return true;      // (no sum that could wrap: what is still missing shrinks)
    freed += e[i].bytes;
  }
  victims->clear();
  return false;
}
