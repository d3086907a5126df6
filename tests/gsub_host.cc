// gsub_host.cc — the sub-sorted grouped form of viyadb_amd/csrc/vh_grouped.h as plain C++ (tests/test_gsub_host.py compiles this plain and
// with -fsanitize=address,undefined and runs it).
//
// For synthetic tiles the program does what group_bits_kernel does when a sub column is set — the rows' vh_gsub_sort_word() sorted as plain
// integers, start[] counted from the values, a row's place = where its word came to lie, kfirst[w] = the sub key at place 32 w — and checks
// the order ((grouping value, sub key, row), valid rows first), the header and the boundary keys against a plain reading of the tile. Then,
// for every run, every relation and EVERY literal of the field, it asks vh_gsub_trim() for the stretch and compares with brute force: every
// place of the run whose key satisfies the relation lies inside it, a trimmed side is a multiple of 32, the other the run's own bound.
// The boundary keys are a vector of exactly 64 entries and only those of places inside the run may be read: the others are poisoned with a
// value that would cut wrongly (and the sanitizer sees a step outside the vector).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vh_grouped.h"

struct Tile {
  uint32_t gbits = 2, sbits = 10, valid = VH_GROUP_TILE;
  std::vector<uint32_t> g = std::vector<uint32_t>(VH_GROUP_TILE, 0), k = g;
};

struct Built {
  std::vector<uint32_t> row_at, start;
  std::vector<uint16_t> kfirst;
};

static bool build(const Tile& t, Built* B) {
  const uint32_t nv = 1u << t.gbits;
  std::vector<uint32_t> words(VH_GROUP_TILE);
  for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) words[i] = vh_gsub_sort_word(vh_gsub_key(t.g[i], t.k[i], t.sbits), i, i < t.valid);
  std::sort(words.begin(), words.end());
  B->row_at.assign(VH_GROUP_TILE, ~0u);
  std::vector<bool> seen(VH_GROUP_TILE, false);
  for (uint32_t at = 0; at < VH_GROUP_TILE; ++at) {
    const uint32_t row = vh_gsub_sorted_row(words[at]);
    if (seen[row]) { printf("builder: row %u has two places\n", row); return false; }
    seen[row] = true;
    if ((at < t.valid) != (row < t.valid)) { printf("builder: place %u holds row %u of %u valid rows\n", at, row, t.valid); return false; }
    B->row_at[at] = row;
    if (at < t.valid && vh_gsub_sorted_sub(words[at], t.sbits) != t.k[row]) { printf("builder: place %u: key %u, row %u has %u\n", at, vh_gsub_sorted_sub(words[at], t.sbits), row, t.k[row]); return false; }
  }
  // the composite order: (grouping value, sub key, row), strictly ascending
  for (uint32_t at = 1; at < t.valid; ++at) {
    const uint32_t a = B->row_at[at - 1], b = B->row_at[at];
    const bool asc = t.g[a] != t.g[b] ? t.g[a] < t.g[b] : t.k[a] != t.k[b] ? t.k[a] < t.k[b] : a < b;
    if (!asc) { printf("builder: places %u, %u hold rows %u, %u out of order\n", at - 1, at, a, b); return false; }
  }
  B->start.assign(nv, 0);
  for (uint32_t v = 0; v < nv; ++v) for (uint32_t i = 0; i < t.valid; ++i) if (t.g[i] < v) ++B->start[v];
  for (uint32_t v = 0; v < nv; ++v) {
    const uint32_t end = v + 1u < nv ? B->start[v + 1u] : t.valid;
    for (uint32_t at = B->start[v]; at < end; ++at) if (t.g[B->row_at[at]] != v) { printf("builder: place %u of run %u holds value %u\n", at, v, t.g[B->row_at[at]]); return false; }
  }
  B->kfirst.assign(VH_GROUP_WORDS, 0);          // (exactly the tile's 128 bytes)
  if (B->kfirst.size() * sizeof(uint16_t) != VH_GSUB_KEYS_BYTES) { printf("builder: %zu boundary keys\n", B->kfirst.size()); return false; }
  for (uint32_t w = 0; w < VH_GROUP_WORDS; ++w) B->kfirst[w] = (uint16_t)vh_gsub_sorted_sub(words[32u * w], t.sbits);
  for (uint32_t w = 0; 32u * w < t.valid; ++w) if (B->kfirst[w] != t.k[B->row_at[32u * w]]) { printf("builder: kfirst[%u]\n", w); return false; }
  return true;
}

static bool satisfies(int op, uint32_t key, uint32_t lit) {
  switch (op) {
    case VH_GSUB_EQ: return key == lit;
    case VH_GSUB_LT: return key < lit;
    case VH_GSUB_LE: return key <= lit;
    case VH_GSUB_GT: return key > lit;
    default: return key >= lit;
  }
}

static bool trims(const Tile& t, const Built& B) {
  const uint32_t nv = 1u << t.gbits, kmax = (1u << t.sbits) - 1u;
  static const int ops[5] = {VH_GSUB_EQ, VH_GSUB_LT, VH_GSUB_LE, VH_GSUB_GT, VH_GSUB_GE};
  unsigned long long kept = 0, whole = 0;
  for (uint32_t v = 0; v < nv; ++v) {
    const uint32_t start = B.start[v], end = v + 1u < nv ? B.start[v + 1u] : t.valid;
    std::vector<uint32_t> key(end - start);
    for (uint32_t at = start; at < end; ++at) key[at - start] = t.k[B.row_at[at]];
    for (int op : ops) {
      // only boundary keys of places inside the run may be read: the others would cut everything away (a key past any literal in front of
      // the run, one short of any literal behind it)
      std::vector<uint16_t> kf = B.kfirst;
      for (uint32_t w = 0; w < VH_GROUP_WORDS; ++w) if (32u * w < start || 32u * w >= end) kf[w] = (uint16_t)(32u * w < start ? kmax : 0u);
      for (uint32_t lit = 0; lit <= kmax; ++lit) {
        uint32_t s2 = ~0u, e2 = ~0u;
        vh_gsub_trim(kf.data(), start, end, op, lit, &s2, &e2);
        if (s2 < start || s2 > e2 || e2 > end) { printf("run [%u, %u) op %d literal %u: stretch [%u, %u)\n", start, end, op, lit, s2, e2); return false; }
        if ((s2 != start && s2 % 32u) || (e2 != end && e2 % 32u)) { printf("run [%u, %u) op %d literal %u: stretch [%u, %u) is cut inside a word\n", start, end, op, lit, s2, e2); return false; }
        for (uint32_t at = start; at < end; ++at)          // brute force
          if (satisfies(op, key[at - start], lit) && (at < s2 || at >= e2)) { printf("run [%u, %u) op %d literal %u: place %u (key %u) lies outside [%u, %u)\n", start, end, op, lit, at, key[at - start], s2, e2); return false; }
        kept += e2 - s2; whole += end - start;
      }
    }
    // a relation the order says nothing about (NE) leaves the run alone
    uint32_t s2 = ~0u, e2 = ~0u;
    vh_gsub_trim(B.kfirst.data(), start, end, 1, 0u, &s2, &e2);
    if (s2 != start || e2 != end) { printf("run [%u, %u): NE cut it to [%u, %u)\n", start, end, s2, e2); return false; }
  }
  if (whole && t.valid >= 512u && kept * 10ull > whole * 9ull) { printf("the trims keep %llu of %llu places: they cut nothing\n", kept, whole); return false; }
  return true;
}

static bool check(const char* name, const Tile& t) {
  Built B;
  const bool ok = build(t, &B) && trims(t, B);
  printf("%s: %s\n", name, ok ? "ok" : "FAILED");
  return ok;
}

int main() {
  bool ok = true;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 11); };
  auto keys = [&](Tile& t) { for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) t.k[i] = rnd() & ((1u << t.sbits) - 1u); };
  // `pre` rows of value 0, `n` of value 1, the rest of value `rest`, in random order among the valid rows: the run of 1 is [pre, pre + n)
  auto run_tile = [&](uint32_t pre, uint32_t n, uint32_t rest, uint32_t valid) {
    Tile t; t.valid = valid; keys(t);
    for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) t.g[i] = i < pre ? 0u : i < pre + n ? 1u : rest;
    for (uint32_t i = valid; i > 1; --i) std::swap(t.g[i - 1], t.g[rnd() % i]);
    return t;
  };
  char name[160];
  for (uint32_t n : {0u, 1u, 31u, 32u, 33u}) {
    snprintf(name, sizeof(name), "a run of %u places at place 700", n);
    ok &= check(name, run_tile(700, n, 2, VH_GROUP_TILE));
  }
  { Tile t; keys(t); for (auto& v : t.g) v = 1; ok &= check("a run of 2048 places", t); }
  for (uint32_t pre : {31u, 32u, 33u}) {
    snprintf(name, sizeof(name), "a run of 500 places that starts at place %u", pre);
    ok &= check(name, run_tile(pre, 500, 3, VH_GROUP_TILE));
    snprintf(name, sizeof(name), "a run of 33 places that starts at place %u", pre);
    ok &= check(name, run_tile(pre, 33, 3, VH_GROUP_TILE));
  }
  { Tile t; for (auto& v : t.g) v = rnd() & 3; for (auto& v : t.k) v = 447; ok &= check("all keys equal", t); }
  {   // ties at places 32 w - 1 and 32 w: run 1 starts at place 0 (no value-0 rows); keys 100 on places [0, 31), 447 on [31, 97), 800 behind
    Tile t;
    for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) { t.g[i] = i < 1200 ? 1u : 2u; t.k[i] = i < 31 ? 100u : i < 97 ? 447u : i < 1200 ? 800u : (rnd() & 1023u); }
    for (uint32_t i = 1200; i > 1; --i) { const uint32_t j = rnd() % i; std::swap(t.k[i - 1], t.k[j]); }
    ok &= check("a key repeated across two word boundaries (ties at 32 w - 1 and 32 w)", t);
  }
  { Tile t; keys(t); for (auto& v : t.g) v = rnd() & 3; t.k[5] = 0; t.k[6] = 1023; t.g[5] = t.g[6] = 2; t.k[7] = 0; t.k[8] = 1023; t.g[7] = t.g[8] = 0; ok &= check("keys 0 and the field maximum present, 10 bits", t); }
  { Tile t; t.sbits = 16; t.valid = 300; keys(t); for (auto& v : t.g) v = rnd() & 1; t.k[5] = 0; t.k[6] = 65535; t.g[5] = t.g[6] = 1; ok &= check("keys 0 and the field maximum present, 16 bits (300 valid rows)", t); }
  { Tile t; t.sbits = 16; t.gbits = 4; t.valid = 700; keys(t); for (auto& v : t.g) v = rnd() & 15; t.k[9] = 0; t.k[10] = 65535; t.g[9] = t.g[10] = 15; ok &= check("16 values, 16-bit keys (700 valid rows)", t); }
  { Tile t; t.valid = 904; keys(t); for (auto& v : t.g) v = rnd() & 3; ok &= check("a last tile of 904 valid rows", t); }
  { Tile t = run_tile(300, 604, 1, 904); ok &= check("904 valid rows, the run of 1 ends with them", t); }
  { Tile t; keys(t); for (auto& v : t.g) v = (rnd() & 1) ? 0u : 3u; ok &= check("values no row has (1, 2)", t); }
  { Tile t; keys(t); for (auto& v : t.g) v = rnd() & 3; for (auto& v : t.k) if (v == 447u) v = 448u; ok &= check("a key value no row has (447)", t); }
  { Tile t; t.gbits = 1; t.valid = 0; keys(t); ok &= check("an empty tile", t); }
  return ok ? 0 : 1;
}
