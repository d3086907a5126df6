// Host check of the truth-table form of a set leaf (viyadb_amd/csrc/vh_inset.h, plain C++, no GPU): for every field width NB from 1 to 10,
// vh_inset_bits<NB> over the table vh_inset_truth_build wrote must agree, row by row, with a linear search over the list as the caller gave it.
// A stand-alone program (tests/test_inset_bits_host.py compiles and runs it, once plain and once with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vh_inset.h"

static long g_checks = 0, g_sets = 0;
static int g_fail = 0;

// elem: VH_U32 = 2, VH_I32 = 6 (the literal's low bytes hold the value, as the C ABI carries it)
template <int NB> static void check_set(const std::vector<int64_t>& list, int elem, std::mt19937_64& rng, const char* what) {
  std::vector<uint64_t> bits;
  for (int64_t m : list) { uint64_t b = 0; if (elem == 2) { const uint32_t v = (uint32_t)m; memcpy(&b, &v, 4); } else { const int32_t v = (int32_t)m; memcpy(&b, &v, 4); } bits.push_back(b); }
  VhSetHost h;
  vh_inset_build(elem, bits.data(), bits.size(), false, &h);
  const size_t plain_words = h.words.size();
  vh_inset_truth_build(elem, NB, &h);
  ++g_sets;
  const size_t nw = h.words.size() - h.truth_word;
  if (h.truth_word != plain_words || h.truth_bits != NB || nw % 2 != 0 || nw < 2 || nw != (size_t)(NB <= 6 ? 2 : 1 << (NB - 5))) {
    printf("FAIL NB %d %s: table of %zu words at word %zu (ordinary table: %zu words)\n", NB, what, nw, h.truth_word, plain_words); ++g_fail; return;
  }
  // building it again replaces it: the set keeps one truth table
  vh_inset_truth_build(elem, NB, &h);
  if (h.words.size() != plain_words + nw) { printf("FAIL NB %d %s: a second build left %zu words\n", NB, what, h.words.size()); ++g_fail; return; }
  // an exact-size heap copy of what the kernel reads (for NB <= 5 the one word; the pad word is never read): a read past the end is the sanitizer's to find
  const size_t used = NB <= 5 ? 1 : (size_t)1 << (NB - 5);
  std::vector<uint32_t> truth(h.words.begin() + (long)h.truth_word, h.words.begin() + (long)(h.truth_word + used));
  // ... and the descriptor's address is that of the table behind the ordinary one
  std::vector<uint32_t> all(h.words);
  const VhSetDev d = h.dev(all.data());
  if (d.truth != all.data() + plain_words) { printf("FAIL NB %d %s: descriptor's truth address\n", NB, what); ++g_fail; }
  for (int round = 0; round < 24; ++round) {
    uint32_t x[NB], value[32] = {};
    for (int b = 0; b < NB; ++b) {
      x[b] = round == 0 ? 0u : round == 1 ? ~0u : (uint32_t)rng();
      if (round >= 2 && round < 8 && !list.empty()) x[b] = 0u;      // (filled below: rows that hold members and their neighbours)
    }
    if (round >= 2 && round < 8 && !list.empty())
      for (int k = 0; k < 32; ++k) {
        const int64_t m = list[(size_t)(rng() % list.size())] + (int64_t)(rng() % 3) - 1;
        const uint32_t v = (uint32_t)m & ((1u << NB) - 1u);
        for (int b = 0; b < NB; ++b) x[b] |= ((v >> b) & 1u) << k;
      }
    for (int k = 0; k < 32; ++k) for (int b = 0; b < NB; ++b) value[k] |= ((x[b] >> k) & 1u) << b;
    const uint32_t got = vh_inset_bits<NB>(x, truth.data());
    for (int k = 0; k < 32; ++k) {
      bool want = false;
      for (int64_t m : list) want |= m == (int64_t)value[k];
      ++g_checks;
      if ((bool)((got >> k) & 1u) != want) {
        if (g_fail < 20) printf("FAIL NB %d %s elem %d: row value %u -> %d, linear search says %d\n", NB, what, elem, value[k], (int)!want, (int)want);
        ++g_fail;
      }
    }
  }
}

template <int NB> static void check_width(std::mt19937_64& rng) {
  const int64_t top = (1ll << NB) - 1;
  char what[64];
  for (int elem : {2, 6}) {
    std::vector<int64_t> beyond = {top + 1, 5000 + top, 1ll << 20};      // empty after clipping: every member out of range
    if (elem == 6) { beyond.push_back(-1); beyond.push_back(-(top + 1)); beyond.push_back(INT32_MIN); }
    check_set<NB>(beyond, elem, rng, "empty after clipping");
    check_set<NB>({top / 3}, elem, rng, "one member");
    check_set<NB>({0}, elem, rng, "member 0");
    check_set<NB>({top}, elem, rng, "member 2^NB - 1");
    check_set<NB>({31, 32, 33}, elem, rng, "the word edge");                // (those beyond the field are clipped)
    check_set<NB>({31, 32, 33, 63, 64, top, top + 1, 0}, elem, rng, "word edges, ends and one beyond");
    std::vector<int64_t> every, other;
    for (int64_t v = 0; v <= top; ++v) { every.push_back(v); if (v & 1) other.push_back(v); }
    check_set<NB>(every, elem, rng, "every value");
    check_set<NB>(other, elem, rng, "every other value");
    for (int pct : {1, 10, 50, 90, 99}) {
      std::vector<int64_t> list;
      for (int64_t v = (elem == 6 ? -8 : 0); v <= top + 8; ++v) if ((int)(rng() % 100) < pct) list.push_back(v);
      if (list.empty()) list.push_back(top / 2);
      list.push_back(list[0]);                                               // a duplicate
      snprintf(what, sizeof(what), "density %d%%", pct);
      check_set<NB>(list, elem, rng, what);
    }
    {   // one non-empty table word, the last one: every other word is skipped
      std::vector<int64_t> list;
      for (int64_t v = top - (top < 31 ? top : 31); v <= top; v += 3) list.push_back(v);
      check_set<NB>(list, elem, rng, "last word only");
    }
  }
}

int main() {
  std::mt19937_64 rng(20241019);
  check_width<1>(rng); check_width<2>(rng); check_width<3>(rng); check_width<4>(rng); check_width<5>(rng);
  check_width<6>(rng); check_width<7>(rng); check_width<8>(rng); check_width<9>(rng); check_width<10>(rng);
  printf("%s: %ld rows over %ld sets, %d wrong\n", g_fail ? "FAILED" : "ok", g_checks, g_sets, g_fail);
  return g_fail ? 1 : 0;
}
