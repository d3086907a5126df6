// vh_bits_agg.h — aggregates computed ON the bit-sliced predicate planes (VhPredPack::sliced), 32 rows per call: the sum, the smallest and the
// largest value of a field over the rows of a mask, the rows that belong to one group, and — the other way round, for the row sink — one
// row's record and group id out of the plane words. Plain C++ for host and device, like
// vh_bits_eval.h, whose layout of the planes it shares: the aggregate scan on the planes includes it (vh_scan_planes.hip), and a
// host-compiled check holds it against a per-row evaluation (tests/bits_agg_host.cc). No row is materialised and nothing here is floating point.
//
// A field is `nb` <= VH_BITS_MAX_FIELD consecutive planes, the least significant first, and holds a column's non-negative value as it is.
// The functions come in two forms. The `_at` form takes the plane words of the WHOLE projection for the lane's 32 rows, v[0 .. 32), and
// the field's first plane `off`: a projection has at most 32 planes, so a kernel that aggregates several fields over several masks loads
// every plane once and indexes the array with constants only (it stays in registers). The plain form takes the field's own planes, x[b]
// = plane b of the field: the `_at` form with off = 0. Planes outside the field are not looked at, whatever they hold.
//
// WRAPPING. The reference adds in the metric's own type (src/codegen/db/store.cc:131-161), so a u32 sum wraps. vh_bits_sum returns the
// exact sum of the 32 rows' values — below 2^37, no wrap — as 64 bits; whoever adds such sums up does so modulo 2^64, and vh_state_update
// truncates the total to the state's width when it adds it in. Addition modulo 2^64 followed by truncation to w bits equals w-bit additions
// in any order, so the state equals the reference's sequential adds bit for bit.
#pragma once
#include <stdint.h>
#include "vh_bits_eval.h"

// Σ_b popcount(m & plane b) << b: the sum of the field's values over the rows of m.
VH_BITS_FN uint64_t vh_bits_sum_at(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t off, uint32_t nb, uint32_t m) {
  uint64_t s = 0;
  VH_BITS_UNROLL
  for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) {
    if ((uint32_t)p < off || (uint32_t)p - off >= nb) continue;
    s += (uint64_t)(uint32_t)__builtin_popcount(m & v[p]) << ((uint32_t)p - off);
  }
  return s;
}
// The largest / smallest value of the field among the rows of m; *empty: m has no row (the value then means nothing). From the top plane down
// a candidate mask is narrowed: MAX keeps the candidates that have the bit when any has it, MIN those that lack it when any lacks it. The
// steps are selects on the data, not branches; the branches are on `off` and `nb`, uniform over a wave.
VH_BITS_FN uint32_t vh_bits_max_at(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t off, uint32_t nb, uint32_t m, bool* empty) {
  uint32_t cand = m, val = 0u;
  VH_BITS_UNROLL
  for (int p = VH_BITS_MAX_FIELD - 1; p >= 0; --p) {
    if ((uint32_t)p < off || (uint32_t)p - off >= nb) continue;
    const uint32_t t = cand & v[p];
    const bool any = t != 0u;
    cand = any ? t : cand;
    val |= (any ? 1u : 0u) << ((uint32_t)p - off);
  }
  *empty = m == 0u;
  return val;
}
VH_BITS_FN uint32_t vh_bits_min_at(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t off, uint32_t nb, uint32_t m, bool* empty) {
  uint32_t cand = m, val = 0u;
  VH_BITS_UNROLL
  for (int p = VH_BITS_MAX_FIELD - 1; p >= 0; --p) {
    if ((uint32_t)p < off || (uint32_t)p - off >= nb) continue;
    const uint32_t t = cand & ~v[p];
    const bool any = t != 0u;
    cand = any ? t : cand;
    val |= (any ? 0u : 1u) << ((uint32_t)p - off);
  }
  *empty = m == 0u;
  return val;
}
// The CONSTANT-PARAMETER forms of the three: the field's place is a template argument — what a kernel compiled for one plan's shape knows
// (vh_jit_planes.h) —, so the loop has exactly NB steps and no test per plane: a 10-bit SUM is ten popcounts. Same values as the `_at` forms
// for every (OFF, NB) with OFF + NB <= VH_BITS_MAX_FIELD (tests/plane_jit_host.cc holds them to each other).
template <int OFF, int NB>
VH_BITS_FN uint64_t vh_bits_sum_c(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m) {
  static_assert(OFF >= 0 && NB >= 0 && OFF + NB <= VH_BITS_MAX_FIELD, "a field lies within the projection's planes");
  uint64_t s = 0;
  VH_BITS_UNROLL
  for (int b = 0; b < NB; ++b) s += (uint64_t)(uint32_t)__builtin_popcount(m & v[OFF + b]) << b;
  return s;
}
template <int OFF, int NB>
VH_BITS_FN uint32_t vh_bits_max_c(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m, bool* empty) {
  static_assert(OFF >= 0 && NB >= 0 && OFF + NB <= VH_BITS_MAX_FIELD, "a field lies within the projection's planes");
  uint32_t cand = m, val = 0u;
  VH_BITS_UNROLL
  for (int b = NB - 1; b >= 0; --b) {
    const uint32_t t = cand & v[OFF + b];
    const bool any = t != 0u;
    cand = any ? t : cand;
    val |= (any ? 1u : 0u) << b;
  }
  *empty = m == 0u;
  return val;
}
template <int OFF, int NB>
VH_BITS_FN uint32_t vh_bits_min_c(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t m, bool* empty) {
  static_assert(OFF >= 0 && NB >= 0 && OFF + NB <= VH_BITS_MAX_FIELD, "a field lies within the projection's planes");
  uint32_t cand = m, val = 0u;
  VH_BITS_UNROLL
  for (int b = NB - 1; b >= 0; --b) {
    const uint32_t t = cand & ~v[OFF + b];
    const bool any = t != 0u;
    cand = any ? t : cand;
    val |= (any ? 0u : 1u) << b;
  }
  *empty = m == 0u;
  return val;
}
VH_BITS_FN uint64_t vh_bits_sum(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint32_t m) { return vh_bits_sum_at(x, 0u, nb, m); }
VH_BITS_FN uint32_t vh_bits_max(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint32_t m, bool* empty) { return vh_bits_max_at(x, 0u, nb, m, empty); }
VH_BITS_FN uint32_t vh_bits_min(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint32_t m, bool* empty) { return vh_bits_min_at(x, 0u, nb, m, empty); }

// The rows of one group value: those whose field equals lo + digit (VhGroupDev: the dense digit of a value is value - lo). A value beyond the
// field's range is held by no row (vh_bits_eq).
VH_BITS_FN uint32_t vh_bits_group(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint64_t lo, uint64_t digit) {
  return vh_bits_eq(x, nb, lo + digit, false);
}
// ... and of one group id over SEVERAL group columns at once: `care` has a bit for every plane of the projection that belongs to a group
// column's field, `pat` the columns' values at their fields' places. The AND of vh_bits_group over the columns, for values within their
// fields; care == 0 (no group column): every row.
VH_BITS_FN uint32_t vh_bits_match(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t care, uint32_t pat) {
  uint32_t eq = ~0u;
  VH_BITS_UNROLL
  for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) {
    if (!((care >> p) & 1u)) continue;
    eq &= ((pat >> p) & 1u) ? v[p] : ~v[p];
  }
  return eq;
}

// ---- one row back out of the planes: what the row sink of the aggregate on the planes (vh_plane_agg.h: vh_plane_agg_rows) computes per
// surviving row, where the loop over group ids computes per id.
// Bit p of a row's RECORD is the row's bit of plane p: the record is the row word the planes were sliced from, over the planes of `need`.
// vh_bits_row_bit is one plane's share of it — the kernel fetches the word from the row's source lane plane by plane and ORs the shares —,
// vh_bits_row the whole record of row r out of one lane's own plane words.
VH_BITS_FN uint32_t vh_bits_row_bit(uint32_t word, uint32_t r, uint32_t p) { return ((word >> (r & 31u)) & 1u) << p; }
VH_BITS_FN uint32_t vh_bits_row(const uint32_t (&v)[VH_BITS_MAX_FIELD], uint32_t need, uint32_t r) {
  uint32_t rec = 0u;
  VH_BITS_UNROLL
  for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) {
    if (!((need >> p) & 1u)) continue;
    rec |= vh_bits_row_bit(v[p], r, (uint32_t)p);
  }
  return rec;
}
// A field's value out of a record: nb <= 32 planes from plane off on.
VH_BITS_FN uint32_t vh_bits_row_field(uint32_t rec, uint32_t off, uint32_t nb) {
  return nb == 0u ? 0u : (rec >> off) & (nb >= 32u ? ~0u : (1u << nb) - 1u);
}
// The dense group id of a record: per group column i, digit_i = field_i - g[i].lo, and gid = Σ digit_i * g[i].stride (VhGroupDev: any type
// with lo, extent and stride serves; goff / gbits: the columns' fields, VhPlaneAggDesc). false: a field below lo, or a digit at or beyond
// extent — the row belongs to no id (a value outside the planned range), *gid is not to be used.
template <class GROUP>
VH_BITS_FN bool vh_bits_row_gid(uint32_t rec, int ngroup, const GROUP* g, const uint32_t* goff, const uint32_t* gbits, uint64_t* gid) {
  uint64_t id = 0;
  bool ok = true;
  for (int i = 0; i < ngroup; ++i) {
    const uint64_t field = vh_bits_row_field(rec, goff[i], gbits[i]);
    const uint64_t digit = field - g[i].lo;
    ok = ok && field >= g[i].lo && digit < g[i].extent;
    id += digit * g[i].stride;
  }
  *gid = id;
  return ok;
}
