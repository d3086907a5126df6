// The victim choice of the layout budget (vh_evict_pick, viyadb_amd/csrc/vhh_layout_math.h) against a brute-force model: a stand-alone
// program (tests/test_evict_pick_host.py builds it under AddressSanitizer and UBSan and runs it). One line per check, "<name>: ok".
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "vhh_layout_math.h"

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_failed; } } while (0)

struct Rng {      // splitmix64: the same sets on every machine
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  uint64_t below(uint64_t n) { return next() % n; }
};
struct Layout { uint64_t bytes, last_use, serial; bool pinned; };
static VhEvictEntry entry_of(const Layout& l, uint64_t tick) { return VhEvictEntry{l.bytes, l.last_use, l.serial, !l.pinned && l.last_use != tick}; }

// The model: try every subset size k of the candidates in (last_use, serial) order — the answer is the smallest k whose first k candidates cover
// the deficit; candidates and order are found by selection, not by the sort under test.
static bool model(const std::vector<Layout>& ls, uint64_t tick, uint64_t deficit, std::vector<size_t>* out) {
  out->clear();
  std::vector<size_t> cand;
  std::vector<bool> taken(ls.size(), false);
  for (;;) {
    size_t best = ls.size();
    for (size_t i = 0; i < ls.size(); ++i) {
      if (taken[i] || ls[i].pinned || ls[i].last_use == tick) continue;
      if (best == ls.size() || ls[i].last_use < ls[best].last_use || (ls[i].last_use == ls[best].last_use && ls[i].serial < ls[best].serial)) best = i;
    }
    if (best == ls.size()) break;
    taken[best] = true; cand.push_back(best);
  }
  unsigned __int128 all = 0;
  for (size_t i : cand) all += ls[i].bytes;
  if (all < deficit) return false;
  unsigned __int128 sum = 0;
  for (size_t k = 0; k <= cand.size(); ++k) {
    if (sum >= deficit) { out->assign(cand.begin(), cand.begin() + (long)k); return true; }
    if (k < cand.size()) sum += ls[cand[k]].bytes;
  }
  return false;
}

static void check_one(const std::vector<Layout>& ls, uint64_t tick, uint64_t deficit, const char* what) {
  std::vector<VhEvictEntry> e;
  for (const Layout& l : ls) e.push_back(entry_of(l, tick));
  std::vector<size_t> got{12345}, want;      // (what a caller left in the list must not survive)
  const bool ok = vh_evict_pick(e.data(), e.size(), deficit, &got);
  const bool wok = model(ls, tick, deficit, &want);
  unsigned __int128 evictable = 0;
  for (const Layout& l : ls) if (!l.pinned && l.last_use != tick) evictable += l.bytes;
  CHECK(ok == !(evictable < deficit), "%s: possible %d, evictable bytes %s the deficit", what, (int)ok, evictable < deficit ? "below" : "cover");
  CHECK(ok == wok, "%s: possible %d, model %d", what, (int)ok, (int)wok);
  if (!ok) { CHECK(got.empty(), "%s: impossible, yet %zu victims", what, got.size()); return; }
  CHECK(got == want, "%s: %zu victims, the model names %zu (or others)", what, got.size(), want.size());
  unsigned __int128 freed = 0;
  for (size_t k = 0; k < got.size(); ++k) {
    const size_t i = got[k];
    CHECK(i < ls.size(), "%s: victim index %zu", what, i);
    if (i >= ls.size()) return;
    CHECK(!ls[i].pinned, "%s: victim %zu is pinned", what, i);
    CHECK(ls[i].last_use != tick, "%s: victim %zu carries the current tick", what, i);
    if (k) {
      const Layout &a = ls[got[k - 1]], &b = ls[i];
      CHECK(a.last_use < b.last_use || (a.last_use == b.last_use && a.serial < b.serial), "%s: victims %zu, %zu out of (last_use, serial) order", what, k - 1, k);
    }
    // a prefix of the order: no candidate that is not a victim comes before a victim
    for (size_t o = 0; o < ls.size(); ++o) {
      if (ls[o].pinned || ls[o].last_use == tick || std::find(got.begin(), got.end(), o) != got.end()) continue;
      CHECK(!(ls[o].last_use < ls[i].last_use || (ls[o].last_use == ls[i].last_use && ls[o].serial < ls[i].serial)), "%s: candidate %zu was passed over for %zu", what, o, i);
    }
    if (k + 1 == got.size()) CHECK(freed < deficit, "%s: the last victim was not needed", what);      // minimal
    freed += ls[i].bytes;
  }
  CHECK(freed >= deficit, "%s: the victims do not cover the deficit", what);
}

int main() {
  for (int seed = 0; seed < 64; ++seed) {
    Rng r{(uint64_t)seed * 7919 + 1};
    const int before = g_failed;
    for (int round = 0; round < 200; ++round) {
      const size_t n = (size_t)r.below(13);      // 0..12 entries
      const uint64_t tick = 1 + r.below(8);
      std::vector<Layout> ls;
      uint64_t total = 0;
      for (size_t i = 0; i < n; ++i) {
        Layout l{r.below(4) ? 256 + r.below(1 << 20) : r.below(3), r.below(tick + 1), (uint64_t)i + 1, r.below(4) == 0};
        if (r.below(8) == 0 && i) l.last_use = ls[i - 1].last_use;      // equal ticks: the serial decides
        total += l.bytes; ls.push_back(l);
      }
      for (size_t i = n; i > 1; --i) std::swap(ls[i - 1], ls[r.below(i)]);      // (the order of the entries is not the order of the serials)
      const uint64_t deficits[] = {0, 1, total / 3, total / 2, total, total + 1, r.below(total + 2), ~0ull};
      for (uint64_t d : deficits) check_one(ls, tick, d, "random set");
    }
    printf("seed %d: %s\n", seed, g_failed == before ? "ok" : "FAILED");
  }
  {
    const int before = g_failed;
    std::vector<Layout> none;
    check_one(none, 3, 0, "empty set, deficit 0");
    check_one(none, 3, 1, "empty set, deficit 1");
    std::vector<size_t> v{7};
    CHECK(vh_evict_pick(nullptr, 0, 0, &v) && v.empty(), "empty set: nothing to do is possible");
    CHECK(!vh_evict_pick(nullptr, 0, 1, &v) && v.empty(), "empty set: a deficit is impossible");
    printf("empty set: %s\n", g_failed == before ? "ok" : "FAILED");
  }
  {
    const int before = g_failed;
    std::vector<Layout> ls{{100, 1, 1, false}, {200, 2, 2, false}};
    check_one(ls, 9, 0, "deficit 0");
    std::vector<VhEvictEntry> e{entry_of(ls[0], 9), entry_of(ls[1], 9)};
    std::vector<size_t> v{7};
    CHECK(vh_evict_pick(e.data(), 2, 0, &v) && v.empty(), "deficit 0 evicts nothing");
    printf("deficit 0: %s\n", g_failed == before ? "ok" : "FAILED");
  }
  {
    const int before = g_failed;
    std::vector<Layout> ls{{100, 1, 1, true}, {200, 2, 2, true}, {300, 0, 3, true}};
    check_one(ls, 9, 1, "everything pinned");
    check_one(ls, 9, 0, "everything pinned, deficit 0");
    std::vector<Layout> cur{{100, 9, 1, false}, {200, 9, 2, false}};
    check_one(cur, 9, 1, "everything stamped with the current tick");
    printf("everything pinned: %s\n", g_failed == before ? "ok" : "FAILED");
  }
  {
    const int before = g_failed;
    std::vector<Layout> ls{{100, 4, 5, false}, {100, 4, 2, false}, {100, 4, 9, false}, {100, 0, 11, false}, {100, 4, 1, true}};
    for (uint64_t d : {1ull, 100ull, 101ull, 200ull, 201ull, 400ull, 401ull}) check_one(ls, 7, d, "equal ticks");
    std::vector<VhEvictEntry> e;
    for (const Layout& l : ls) e.push_back(entry_of(l, 7));
    std::vector<size_t> v;
    CHECK(vh_evict_pick(e.data(), e.size(), 250, &v) && v == (std::vector<size_t>{3, 1, 0}), "equal ticks: never used first, then ascending serial");
    std::vector<Layout> big{{~0ull, 1, 1, false}, {~0ull, 2, 2, false}};      // sums past 2^64 must not wrap
    check_one(big, 7, ~0ull, "bytes near 2^64");
    printf("equal ticks: %s\n", g_failed == before ? "ok" : "FAILED");
  }
  return g_failed ? 1 : 0;
}
