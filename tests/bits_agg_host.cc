// Host check of the aggregates on the bit-sliced planes (viyadb_amd/csrc/vh_bits_agg.h, plain C++, no GPU): for random plane words the sum,
// the smallest and the largest value of a field over the rows of a mask, and the rows of a group value, must agree with an evaluation row
// by row. A stand-alone program (tests/test_bits_agg_host.py compiles and runs it, once plain and once with -fsanitize=address,undefined).
// The 32 plane words of a lane are an exact-size heap block: a read outside them is the sanitizer's to find. Planes outside the field under
// test hold random bits, which no result may depend on.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "vh_bits_agg.h"

static long g_checks = 0;
static int g_fail = 0;
static std::mt19937_64 rng(20261020);

typedef uint32_t Planes[VH_BITS_MAX_FIELD];
struct Word {      // 32 rows: their values of one field, and the projection's 32 plane words
  std::unique_ptr<uint32_t[]> mem{new uint32_t[VH_BITS_MAX_FIELD]};
  uint64_t val[32] = {};
  Planes& v() { return *reinterpret_cast<Planes*>(mem.get()); }
  void noise() { for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) mem[p] = (uint32_t)rng(); }
  // write the rows' values into planes [off, off + nb)
  void put(uint32_t off, uint32_t nb, const uint64_t* values) {
    for (uint32_t b = 0; b < nb; ++b) {
      uint32_t w = 0;
      for (int i = 0; i < 32; ++i) w |= (uint32_t)((values[i] >> b) & 1u) << i;
      mem[off + b] = w;
    }
  }
};

static void fail(const char* what, uint32_t off, uint32_t nb, uint32_t m, uint64_t got, uint64_t want) {
  if (++g_fail <= 20) printf("FAIL %s off=%u nb=%u mask=%08x: got %llu, want %llu\n", what, off, nb, m, (unsigned long long)got, (unsigned long long)want);
}

static void check_word(Word& w, uint32_t off, uint32_t nb, uint32_t m) {
  uint64_t sum = 0, mx = 0, mn = ~0ull;
  for (int i = 0; i < 32; ++i) {
    if (!((m >> i) & 1u)) continue;
    sum += w.val[i];
    if (w.val[i] > mx) mx = w.val[i];
    if (w.val[i] < mn) mn = w.val[i];
  }
  bool e1 = false, e2 = false;
  const uint64_t s = vh_bits_sum_at(w.v(), off, nb, m);
  const uint32_t hi = vh_bits_max_at(w.v(), off, nb, m, &e1), lo = vh_bits_min_at(w.v(), off, nb, m, &e2);
  ++g_checks;
  if (s != sum) fail("sum", off, nb, m, s, sum);
  if (e1 != (m == 0) || e2 != (m == 0)) fail("empty", off, nb, m, e1 * 2 + e2, m == 0);
  if (m && hi != mx) fail("max", off, nb, m, hi, mx);
  if (m && lo != mn) fail("min", off, nb, m, lo, mn);
  if (off == 0) {      // the field's own planes: the plain forms
    bool e3 = true, e4 = true;
    if (vh_bits_sum(w.v(), nb, m) != sum) fail("sum (plain)", off, nb, m, vh_bits_sum(w.v(), nb, m), sum);
    const uint32_t h2 = vh_bits_max(w.v(), nb, m, &e3), l2 = vh_bits_min(w.v(), nb, m, &e4);
    if (e3 != (m == 0) || e4 != (m == 0) || (m && (h2 != mx || l2 != mn))) fail("min / max (plain)", off, nb, m, h2, mx);
  }
}

static void fields() {
  const uint32_t widths[] = {1, 5, 10, 11, 31, 32};
  for (uint32_t nb : widths) {
    const uint64_t top = nb == 32 ? 0xFFFFFFFFull : (1ull << nb) - 1;
    std::vector<uint32_t> offs = {0u};
    if (nb < 32) { offs.push_back(32u - nb); if (nb + 1 < 32) offs.push_back(1u); }
    for (uint32_t off : offs)
      for (int round = 0; round < 200; ++round) {
        Word w;
        w.noise();
        const int kind = round % 5;
        for (int i = 0; i < 32; ++i) {
          uint64_t x = rng() & top;
          if (kind == 1) x = top;                              // every row the largest value: ties everywhere
          if (kind == 2) x = 0;                                // MAX of all zeros is 0, and so is the sum
          if (kind == 3) x = (rng() & 1) ? top : (top >> 1);   // two values, many ties
          w.val[i] = x;
        }
        if (kind == 4) { w.val[0] = 0; w.val[31] = top; w.val[rng() % 30 + 1] = 0; w.val[rng() % 30 + 1] = top; }      // planted: 0 and the top value, twice each
        w.put(off, nb, w.val);
        const uint32_t masks[] = {0u, 1u, 1u << 31, ~0u, (uint32_t)rng(), (uint32_t)rng() & (uint32_t)rng(), (uint32_t)rng() | (uint32_t)rng(), 1u | 1u << 31};
        for (uint32_t m : masks) check_word(w, off, nb, m);
      }
  }
}

// 2^20 words of all-ones 32-bit values under the full mask: the total passes 2^32 many times over. Added up modulo 2^64 and truncated to 32
// bits at the end it must equal a u32 that every row was added to in turn (the reference's SUM in the metric's own type).
static void wrap() {
  Word w;
  for (int i = 0; i < 32; ++i) w.val[i] = 0xFFFFFFFFull;
  w.put(0, 32, w.val);
  uint64_t total = 0;
  uint32_t seq = 0;
  for (long k = 0; k < (1l << 20); ++k) {
    total += vh_bits_sum(w.v(), 32, ~0u);
    for (int i = 0; i < 32; ++i) seq += (uint32_t)w.val[i];
  }
  ++g_checks;
  if (total <= 0xFFFFFFFFull) fail("wrap: the total does not pass 2^32", 0, 32, ~0u, total, 0);
  if ((uint32_t)total != seq) fail("wrap", 0, 32, ~0u, (uint32_t)total, seq);
  // ... and with a partial mask per word, so that the partial sums differ
  total = 0; seq = 0;
  for (long k = 0; k < (1l << 16); ++k) {
    const uint32_t m = (uint32_t)rng();
    total += vh_bits_sum(w.v(), 32, m);
    for (int i = 0; i < 32; ++i) if ((m >> i) & 1u) seq += (uint32_t)w.val[i];
  }
  ++g_checks;
  if ((uint32_t)total != seq) fail("wrap (random masks)", 0, 32, 0, (uint32_t)total, seq);
}

// Two group columns: a 2-bit field at plane 3 whose ids are the values 1 .. 3 (lo = 1, extent 3) and a 3-bit field at plane 9 whose ids are
// 2 .. 6 (lo = 2, extent 5). The rows hold any value their fields can, so some lie outside [lo, lo + extent): those are in no id's mask.
static void groups() {
  const uint32_t off1 = 3, nb1 = 2, off2 = 9, nb2 = 3;
  const uint64_t lo1 = 1, ext1 = 3, lo2 = 2, ext2 = 5;
  const uint32_t care = ((1u << nb1) - 1u) << off1 | ((1u << nb2) - 1u) << off2;
  for (int round = 0; round < 500; ++round) {
    Word w, x1, x2;      // w: the projection; x1 / x2: each field's own planes, for the plain form
    w.noise(); x1.noise(); x2.noise();
    uint64_t a[32], b[32];
    for (int i = 0; i < 32; ++i) { a[i] = rng() & 3; b[i] = rng() & 7; }
    w.put(off1, nb1, a); w.put(off2, nb2, b);
    x1.put(0, nb1, a); x2.put(0, nb2, b);
    const uint32_t m = round % 3 == 0 ? ~0u : (uint32_t)rng();
    uint32_t seen = 0, outside = 0;
    for (int i = 0; i < 32; ++i) if (a[i] < lo1 || a[i] >= lo1 + ext1 || b[i] < lo2 || b[i] >= lo2 + ext2) outside |= 1u << i;
    for (uint64_t d1 = 0; d1 < ext1; ++d1)
      for (uint64_t d2 = 0; d2 < ext2; ++d2) {
        uint32_t want = 0;
        for (int i = 0; i < 32; ++i) if (a[i] == lo1 + d1 && b[i] == lo2 + d2) want |= 1u << i;
        const uint32_t one = vh_bits_group(x1.v(), nb1, lo1, d1) & vh_bits_group(x2.v(), nb2, lo2, d2);
        const uint32_t pat = (uint32_t)(lo1 + d1) << off1 | (uint32_t)(lo2 + d2) << off2;
        const uint32_t both = vh_bits_match(w.v(), care, pat);
        ++g_checks;
        if (one != want) fail("group (per column)", off1, nb1, m, one, want);
        if (both != want) fail("group (match)", off2, nb2, m, both, want);
        if (seen & both) fail("group: two ids share a row", 0, 0, m, seen & both, 0);
        seen |= both;
      }
    if ((seen & outside) != 0 || (seen | outside) != ~0u) fail("group: rows outside the range", 0, 0, m, seen, ~outside);
    if ((m & ~seen) != (m & outside)) fail("group: the passing rows of no id", 0, 0, m, m & ~seen, m & outside);
    // a value beyond the field: no row
    if (vh_bits_group(x1.v(), nb1, 3, 1) != 0u) fail("group: value 4 in a 2-bit field", 0, nb1, m, vh_bits_group(x1.v(), nb1, 3, 1), 0);
  }
  Word w;
  w.noise();
  ++g_checks;
  if (vh_bits_match(w.v(), 0u, 0u) != ~0u) fail("group: no group column", 0, 0, 0, vh_bits_match(w.v(), 0u, 0u), ~0u);
}

int main() {
  fields();
  wrap();
  groups();
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("ok: %ld checks\n", g_checks);
  return 0;
}
