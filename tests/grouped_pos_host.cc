// grouped_pos_host.cc — viyadb_amd/csrc/vh_grouped.h as plain C++ (tests/test_grouped_pos.py compiles and runs this with g++).
//
// For synthetic tiles it does what group_bits_kernel does — the lanes' equality masks, their exclusive prefix, start[] — builds the
// permutation with vh_grouped_pos(), then does what the scan does: for a literal, a snapshot and the planes' bits (which also hold zeros
// for the rows behind the mirrored ones, and for lanes wholly behind the snapshot whatever the scan's zero-filled loads give) it finds
// every valid row's record again through the SAME function, and checks that no place reaches the tile's valid-row count.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vh_grouped.h"

static const uint32_t NL = VH_GROUP_TILE / 32u;

struct Tile {
  uint32_t bits = 2, valid = VH_GROUP_TILE;      // rows below `valid` are mirrored
  std::vector<uint32_t> val = std::vector<uint32_t>(VH_GROUP_TILE, 0);
};

// the builder: out[place] = row, start[v]
static bool build(const Tile& t, std::vector<uint32_t>* out, std::vector<uint32_t>* start) {
  const uint32_t nv = 1u << t.bits;
  std::vector<uint32_t> eq(nv * NL, 0), before(nv * NL, 0), total(nv, 0);
  for (uint32_t i = 0; i < t.valid; ++i) eq[(t.val[i] & (nv - 1)) * NL + (i >> 5)] |= 1u << (i & 31);
  for (uint32_t v = 0; v < nv; ++v) { uint32_t run = 0; for (uint32_t l = 0; l < NL; ++l) { before[v * NL + l] = run; run += (uint32_t)__builtin_popcount(eq[v * NL + l]); } total[v] = run; }
  start->assign(nv, 0);
  for (uint32_t v = 1; v < nv; ++v) (*start)[v] = (*start)[v - 1] + total[v - 1];
  out->assign(t.valid, ~0u);
  for (uint32_t i = 0; i < t.valid; ++i) {
    const uint32_t v = t.val[i] & (nv - 1), l = i >> 5;
    const uint32_t pos = vh_grouped_pos(eq[v * NL + l], before[v * NL + l], (*start)[v], i & 31u);
    if (pos >= t.valid) { printf("builder: row %u -> place %u of %u valid rows\n", i, pos, t.valid); return false; }
    if ((*out)[pos] != ~0u) { printf("builder: place %u taken twice (rows %u and %u)\n", pos, (*out)[pos], i); return false; }
    (*out)[pos] = i;
  }
  return true;
}

// the scan, for one literal and one snapshot (rows below `snap` <= valid are scanned): every scanned row that holds the literal must be found
static bool scan(const Tile& t, const std::vector<uint32_t>& out, const std::vector<uint32_t>& start, uint64_t lit, uint32_t snap) {
  const uint32_t nv = 1u << t.bits;
  // the planes: the field of every mirrored row, zeros behind them; a lane wholly behind the snapshot loads zeros instead
  std::vector<uint32_t> geq(NL, 0);
  const bool in_range = (lit >> t.bits) == 0;
  for (uint32_t l = 0; l < NL; ++l) {
    if (l * 32u >= snap) { geq[l] = (in_range && lit == 0) ? ~0u : 0u; continue; }
    for (uint32_t b = 0; b < 32; ++b) { const uint32_t i = l * 32u + b; const uint32_t field = i < t.valid ? (t.val[i] & (nv - 1)) : 0u; if (in_range && field == (uint32_t)lit) geq[l] |= 1u << b; }
  }
  const uint32_t st = in_range ? start[(uint32_t)lit] : 0u;      // (never indexed with a literal outside the field)
  uint32_t run = 0, found = 0, want = 0;
  for (uint32_t i = 0; i < snap; ++i) want += in_range && (t.val[i] & (nv - 1)) == (uint32_t)lit;
  for (uint32_t l = 0; l < NL; ++l) {
    const uint32_t before = run;
    run += (uint32_t)__builtin_popcount(geq[l]);
    uint32_t smask = geq[l];
    if (l * 32u + 32u > snap) smask &= l * 32u < snap ? (1u << (snap - l * 32u)) - 1u : 0u;
    for (uint32_t m = smask; m; m &= m - 1u) {
      const uint32_t b = (uint32_t)__builtin_ctz(m), pos = vh_grouped_pos(geq[l], before, st, b);
      if (pos >= t.valid) { printf("scan: literal %llu row %u -> place %u of %u valid rows\n", (unsigned long long)lit, l * 32u + b, pos, t.valid); return false; }
      if (out[pos] != l * 32u + b) { printf("scan: literal %llu row %u -> place %u holds row %u\n", (unsigned long long)lit, l * 32u + b, pos, out[pos]); return false; }
      ++found;
    }
  }
  if (found != want) { printf("scan: literal %llu snapshot %u: %u of %u rows found\n", (unsigned long long)lit, snap, found, want); return false; }
  return true;
}

static bool check(const char* name, const Tile& t, const std::vector<uint32_t>& snaps) {
  std::vector<uint32_t> out, start;
  bool ok = build(t, &out, &start);
  for (uint64_t lit = 0; ok && lit < (1ull << t.bits) + 2; ++lit)         // (the last two lie beyond the field)
    for (uint32_t s : snaps) if (s <= t.valid) ok = ok && scan(t, out, start, lit, s);
  ok = ok && scan(t, out, start, ~0ull, t.valid);
  printf("%s: %s\n", name, ok ? "ok" : "FAILED");
  return ok;
}

int main() {
  bool ok = true;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 11); };
  const std::vector<uint32_t> full{0, 1, 31, 32, 33, 37, 904, 1024, 2047, 2048};
  { Tile t; for (auto& v : t.val) v = 1; ok &= check("every row equal to the literal", t, full); }
  { Tile t; for (auto& v : t.val) v = 2 + (rnd() & 1); ok &= check("no row equal to the literal (0, 1)", t, full); }
  { Tile t; for (auto& v : t.val) v = 3; t.val[0] = 1; ok &= check("one equal row, lane 0 bit 0", t, full); }
  { Tile t; for (auto& v : t.val) v = 3; t.val[2047] = 1; ok &= check("one equal row, lane 63 bit 31", t, full); }
  { Tile t; t.valid = 904; for (auto& v : t.val) v = rnd() & 3; ok &= check("a partial tile of 904 valid rows", t, full); }
  { Tile a, b; for (auto& v : a.val) v = rnd() & 3; for (auto& v : b.val) v = rnd() & 3; b.valid = 37;
    ok &= check("2048 + 37 valid rows: the full tile", a, full); ok &= check("2048 + 37 valid rows: the tile that ends inside a lane", b, full); }
  { Tile t; t.bits = 4; for (auto& v : t.val) v = rnd() & 15; ok &= check("all 16 values of a 4-bit field", t, full); }
  { Tile t; t.bits = 4; t.valid = 1000; for (uint32_t i = 0; i < VH_GROUP_TILE; ++i) t.val[i] = i % 16; ok &= check("16 values, 1000 valid rows", t, full); }
  { Tile t; t.bits = 1; t.valid = 0; ok &= check("an empty tile", t, full); }
  return ok ? 0 : 1;
}
