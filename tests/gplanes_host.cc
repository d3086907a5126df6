// gplanes_host.cc — the clustered predicate planes of viyadb_amd/csrc/vh_grouped.h as plain C++ (tests/test_gplanes_host.py compiles this
// with -fsanitize=address,undefined and runs it).
//
// A row's predicate word here is [a: 5 bits][g: the grouping field][b: 10 bits], so the squeeze has fields on both sides of the one it takes
// out (15 planes: a word group of 16 dwords, one of them padding). For synthetic tiles the program does what group_bits_kernel does — the
// permutation through vh_grouped_pos(), the header start[], then the tile's block: every place's squeezed word spread over the planes at
// vh_gplanes_off() — and then what the scan does for `g == literal AND a < ca AND b >= cb`: start[literal] and end from the header, the
// run's words from vh_gplanes_first_word() / vh_gplanes_last_word(), per word the planes the filter reads (found through vh_gplanes_plane())
// under vh_gplanes_word_mask(); a survivor's place is its bit position. The rows behind the places found must be exactly the rows a plain
// row-order evaluation passes; no byte outside the tile's block is touched; places at or beyond the valid rows hold zeros.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vh_grouped.h"

static const uint32_t NL = VH_GROUP_TILE / 32u, ABITS = 5, BBITS = 10;

struct Tile {
  uint32_t bits = 2, valid = VH_GROUP_TILE;
  std::vector<uint32_t> g = std::vector<uint32_t>(VH_GROUP_TILE, 0), a = g, b = g;
  uint32_t goff() const { return ABITS; }
  uint32_t nplanes() const { return ABITS + BBITS; }            // without the grouping field
  uint32_t word(uint32_t i) const { return a[i] | (g[i] << ABITS) | (b[i] << (ABITS + bits)); }
};

struct Built {
  std::vector<uint32_t> row_at;      // place -> row
  std::vector<uint32_t> start;       // the header
  std::vector<uint32_t> block;       // the tile's block, 64 x G dwords
  uint32_t G = 0;
};

static bool build(const Tile& t, Built* B) {
  const uint32_t nv = 1u << t.bits;
  std::vector<uint32_t> eq(nv * NL, 0), before(nv * NL, 0), total(nv, 0);
  for (uint32_t i = 0; i < t.valid; ++i) eq[t.g[i] * NL + (i >> 5)] |= 1u << (i & 31);
  for (uint32_t v = 0; v < nv; ++v) { uint32_t run = 0; for (uint32_t l = 0; l < NL; ++l) { before[v * NL + l] = run; run += (uint32_t)__builtin_popcount(eq[v * NL + l]); } total[v] = run; }
  B->start.assign(nv, 0);
  for (uint32_t v = 1; v < nv; ++v) B->start[v] = B->start[v - 1] + total[v - 1];
  B->row_at.assign(VH_GROUP_TILE, ~0u);
  B->G = vh_gplanes_group(t.nplanes());
  if (B->G % 4u || B->G < t.nplanes()) { printf("builder: a word group of %u dwords for %u planes\n", B->G, t.nplanes()); return false; }
  if (vh_gplanes_tile_bytes(B->G) != 256ull * B->G || vh_gplanes_tile_bytes(B->G) % 128ull) { printf("builder: a block of %llu bytes\n", (unsigned long long)vh_gplanes_tile_bytes(B->G)); return false; }
  B->block.assign((size_t)VH_GROUP_WORDS * B->G, 0u);          // (exactly the block: the sanitizer sees a step outside it)
  for (uint32_t i = 0; i < t.valid; ++i) {
    const uint32_t v = t.g[i], l = i >> 5;
    const uint32_t pos = vh_grouped_pos(eq[v * NL + l], before[v * NL + l], B->start[v], i & 31u);
    if (pos >= t.valid || B->row_at[pos] != ~0u) { printf("builder: row %u -> place %u\n", i, pos); return false; }
    B->row_at[pos] = i;
    const uint32_t w = vh_gplanes_squeeze(t.word(i), t.goff(), t.bits);
    if (w >> t.nplanes()) { printf("builder: row %u: squeezed word %#x has bits beyond plane %u\n", i, w, t.nplanes()); return false; }
    const uint64_t off = vh_gplanes_off(0u, pos >> 5, B->G);
    if (off % 16u || off + 4ull * B->G > vh_gplanes_tile_bytes(B->G)) { printf("builder: word %u at byte %llu\n", pos >> 5, (unsigned long long)off); return false; }
    for (uint32_t p = 0; p < t.nplanes(); ++p) if ((w >> p) & 1u) B->block[off / 4u + p] |= 1u << (pos & 31u);
  }
  // the second tile of a segment begins where the first ends, and a segment holds whole tiles
  if (vh_gplanes_off(1u, 0u, B->G) != vh_gplanes_tile_bytes(B->G) || vh_gplanes_seg_bytes(VH_GROUP_TILE + 1u, B->G) != 2u * vh_gplanes_tile_bytes(B->G) ||
      vh_gplanes_seg_bytes(VH_GROUP_TILE, B->G) != vh_gplanes_tile_bytes(B->G)) { printf("builder: tiles do not tile\n"); return false; }
  return true;
}

// a field of `bits` bits whose row-order planes begin at `off`, for the place `bit` of a word group
static uint32_t field_of(const Tile& t, const uint32_t* grp, uint32_t off, uint32_t bits, uint32_t bit) {
  uint32_t v = 0;
  for (uint32_t k = 0; k < bits; ++k) v |= ((grp[vh_gplanes_plane(off + k, t.goff(), t.bits)] >> bit) & 1u) << k;
  return v;
}

static bool scan(const Tile& t, const Built& B, uint64_t lit, uint32_t ca, uint32_t cb) {
  const uint32_t nv = 1u << t.bits;
  std::vector<uint32_t> want, found;
  for (uint32_t i = 0; i < t.valid; ++i) if (t.g[i] == lit && t.a[i] < ca && t.b[i] >= cb) want.push_back(i);
  if ((lit >> t.bits) == 0) {         // (a literal no value of the field can equal queues nothing: the header is never indexed with it)
    const uint32_t l = (uint32_t)lit, start = B.start[l], end = l + 1u < nv ? B.start[l + 1u] : t.valid;
    if (start > end || end > t.valid) { printf("scan: literal %u: run [%u, %u) of %u valid rows\n", l, start, end, t.valid); return false; }
    const uint32_t first = vh_gplanes_first_word(start), last = vh_gplanes_last_word(start, end);
    if (last < first || last > VH_GROUP_WORDS || (start == end) != (first == last)) { printf("scan: run [%u, %u): words [%u, %u)\n", start, end, first, last); return false; }
    uint32_t covered = 0;
    for (uint32_t w = 0; w < VH_GROUP_WORDS; ++w) {       // the mask function over EVERY word: inside the run's words it covers the run, outside it is empty
      const uint32_t m = vh_gplanes_word_mask(w, start, end);
      covered += (uint32_t)__builtin_popcount(m);
      if ((w < first || w >= last) && m) { printf("scan: run [%u, %u): word %u outside [%u, %u) has mask %#x\n", start, end, w, first, last, m); return false; }
      if (w >= first && w < last && !m) { printf("scan: run [%u, %u): word %u of the run has an empty mask\n", start, end, w); return false; }
      for (uint32_t bit = 0; bit < 32; ++bit) if (((m >> bit) & 1u) != (uint32_t)(w * 32u + bit >= start && w * 32u + bit < end)) { printf("scan: run [%u, %u): word %u mask %#x\n", start, end, w, m); return false; }
    }
    if (covered != end - start) { printf("scan: run [%u, %u): masks cover %u places\n", start, end, covered); return false; }
    for (uint32_t w = first; w < last; ++w) {
      const uint32_t* grp = B.block.data() + vh_gplanes_off(0u, w, B.G) / 4u;
      for (uint32_t m = vh_gplanes_word_mask(w, start, end); m; m &= m - 1u) {
        const uint32_t bit = (uint32_t)__builtin_ctz(m), place = w * 32u + bit;
        const uint32_t a = field_of(t, grp, 0u, ABITS, bit), b = field_of(t, grp, ABITS + t.bits, BBITS, bit);
        const uint32_t row = B.row_at[place];
        if (row == ~0u || a != t.a[row] || b != t.b[row] || t.g[row] != l) { printf("scan: literal %u place %u: row %u, a %u b %u\n", l, place, row, a, b); return false; }
        if (a < ca && b >= cb) found.push_back(row);
      }
    }
  }
  std::sort(found.begin(), found.end());
  if (found != want) { printf("scan: literal %llu: %zu rows found, %zu pass in row order\n", (unsigned long long)lit, found.size(), want.size()); return false; }
  return true;
}

static bool check(const char* name, const Tile& t) {
  Built B;
  bool ok = build(t, &B);
  // places at or beyond the valid rows hold zeros, and so does the padding
  for (uint32_t place = t.valid; ok && place < VH_GROUP_TILE; ++place)
    for (uint32_t p = 0; p < B.G; ++p) if ((B.block[vh_gplanes_off(0u, place >> 5, B.G) / 4u + p] >> (place & 31u)) & 1u) { printf("place %u of %u valid rows holds a bit of plane %u\n", place, t.valid, p); ok = false; }
  for (uint32_t w = 0; ok && w < VH_GROUP_WORDS; ++w) for (uint32_t p = t.nplanes(); p < B.G; ++p) if (B.block[(size_t)w * B.G + p]) { printf("padding plane %u of word %u is not zero\n", p, w); ok = false; }
  for (uint64_t lit = 0; ok && lit < (1ull << t.bits) + 2; ++lit) {          // (the last two lie beyond the field)
    ok = ok && scan(t, B, lit, 1u << ABITS, 0u);        // every row of the run passes
    ok = ok && scan(t, B, lit, 13u, 553u);
    ok = ok && scan(t, B, lit, 0u, 0u);                 // none does
  }
  ok = ok && scan(t, B, ~0ull, 13u, 553u);
  printf("%s: %s\n", name, ok ? "ok" : "FAILED");
  return ok;
}

int main() {
  bool ok = true;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 11); };
  auto payload = [&](Tile& t) { for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) { t.a[i] = rnd() & ((1u << ABITS) - 1u); t.b[i] = rnd() & ((1u << BBITS) - 1u); } };
  // `pre` rows of value 0, `n` of value 1, the rest of value `rest`, in random order among the tile's valid rows: the run of 1 is [pre, pre + n)
  auto run_tile = [&](uint32_t pre, uint32_t n, uint32_t rest, uint32_t valid) {
    Tile t; t.valid = valid; payload(t);
    for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) t.g[i] = i < pre ? 0u : i < pre + n ? 1u : rest;
    for (uint32_t i = valid; i > 1; --i) std::swap(t.g[i - 1], t.g[rnd() % i]);
    return t;
  };
  { Tile t; payload(t); for (auto& v : t.g) v = 1; ok &= check("all rows one value (a run of 64 words, every other run empty)", t); }
  { Tile t; payload(t); for (auto& v : t.g) v = 3; ok &= check("all rows the field's last value", t); }
  { Tile t; payload(t); for (auto& v : t.g) v = (rnd() & 1) ? 0 : 3; ok &= check("values with no rows (1, 2) between two that have them", t); }
  for (uint32_t n : {1u, 31u, 32u, 33u, 2047u}) {
    char name[128];
    for (uint32_t pre : {0u, 1u, 31u, 32u, 33u, 1000u}) {
      if (pre + n > VH_GROUP_TILE) continue;
      snprintf(name, sizeof(name), "a run of exactly %u places that starts at place %u", n, pre);
      ok &= check(name, run_tile(pre, n, 2, VH_GROUP_TILE));
    }
    snprintf(name, sizeof(name), "a run of exactly %u places that ends at place 2048", n);
    ok &= check(name, run_tile(VH_GROUP_TILE - n, n, 2, VH_GROUP_TILE));
    snprintf(name, sizeof(name), "a run of exactly %u places that ends one short of 2048", n);
    if (n < 2047u) ok &= check(name, run_tile(VH_GROUP_TILE - n - 1u, n, 3, VH_GROUP_TILE));
  }
  { Tile t; t.valid = 904; payload(t); for (auto& v : t.g) v = rnd() & 3; ok &= check("904 valid rows, the last value's run ends with them", t); }
  { Tile t = run_tile(300, 604, 1, 904); ok &= check("904 valid rows, the run of 1 ends with them and 2, 3 have none", t); }
  { Tile t; t.bits = 4; payload(t); for (auto& v : t.g) v = rnd() & 15; ok &= check("all 16 values of a 4-bit field", t); }
  { Tile t; t.bits = 4; t.valid = 1000; payload(t); for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) t.g[i] = i % 16; ok &= check("16 values, 1000 valid rows", t); }
  { Tile t; t.bits = 1; t.valid = 0; payload(t); ok &= check("an empty tile", t); }
  return ok ? 0 : 1;
}
