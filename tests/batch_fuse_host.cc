// The grouping of a batch's members into fused launches (viyadb_amd/csrc/vh_batch.h: vh_batch_group), run on the CPU over hand-made and random
// descriptor lists. A stand-alone program: tests/test_batch_fuse_host.py builds it plain and with AddressSanitizer / UndefinedBehaviorSanitizer
// (the lists are exact-size heap blocks, so an index outside them is an error).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "vh_batch.h"

static int g_checks = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
  } while (0)

static VhFuseDesc cand(uint64_t v, uint32_t lds, uint32_t scope = 0, uint32_t nseg = 3, uint32_t cps = 4) {
  VhFuseDesc d{};
  d.candidate = 1; d.scope = scope; d.v_serial = v; d.nseg = nseg; d.chunks_per_seg = cps; d.lds_bytes = lds;
  return d;
}
static VhFuseDesc other() { VhFuseDesc d{}; d.v_serial = 1; d.nseg = 3; d.chunks_per_seg = 4; d.lds_bytes = 64; return d; }

// the properties every answer has, whatever the list
static uint32_t check_list(const std::vector<VhFuseDesc>& in, std::vector<int32_t>* out_groups = nullptr) {
  const uint32_t n = (uint32_t)in.size();
  VhFuseDesc* d = (VhFuseDesc*)malloc(sizeof(VhFuseDesc) * (n ? n : 1));      // exact size: the sanitizer sees an index past the end
  int32_t* g = (int32_t*)malloc(sizeof(int32_t) * (n ? n : 1));
  for (uint32_t i = 0; i < n; ++i) d[i] = in[i];
  const uint32_t ng = vh_batch_group(d, n, g);
  std::map<int32_t, std::vector<uint32_t>> members;
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(g[i] >= -1 && g[i] < (int32_t)ng, "member %u: group %d of %u", i, g[i], ng);      // exactly one group, or single
    if (!d[i].candidate) CHECK(g[i] == -1, "member %u is no candidate and in group %d", i, g[i]);
    if (g[i] >= 0) members[g[i]].push_back(i);      // (ascending i: plan order is kept inside a group by construction of this list ...)
  }
  CHECK(members.size() == ng, "%zu groups with members, %u reported", members.size(), ng);
  uint32_t first_prev = 0;
  for (uint32_t k = 0; k < ng; ++k) {
    const std::vector<uint32_t>& m = members[(int32_t)k];
    CHECK(m.size() >= 2, "group %u has %zu member(s): a lone candidate is single", k, m.size());
    CHECK(m.size() <= VH_BATCH_MAX, "group %u has %zu members", k, m.size());
    uint64_t lds = 0;
    for (uint32_t i : m) {
      CHECK(vh_fuse_same_key(d[m[0]], d[i]), "group %u: members %u and %u differ in the key", k, m[0], i);
      lds += d[i].lds_bytes;
    }
    CHECK(lds <= VH_BATCH_LDS_CAP, "group %u: %llu bytes of LDS", k, (unsigned long long)lds);
    if (k) CHECK(m[0] > first_prev, "groups are numbered by their first members: %u then %u", first_prev, m[0]);      // (... and the groups' order too)
    first_prev = m[0];
  }
  // plan order: the groups of one key are filled one after the other, so along the list a key's group numbers never go down
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = i + 1; j < n; ++j)
      if (g[i] >= 0 && g[j] >= 0 && vh_fuse_same_key(d[i], d[j])) CHECK(g[i] <= g[j], "members %u and %u of one key are in groups %d and %d", i, j, g[i], g[j]);
  // the first two candidates of a key share a group whenever they fit together
  for (uint32_t i = 0; i < n; ++i) {
    if (!d[i].candidate) continue;
    bool first = true;
    for (uint32_t j = 0; j < i; ++j) if (d[j].candidate && vh_fuse_same_key(d[i], d[j])) first = false;
    if (!first) continue;
    for (uint32_t j = i + 1; j < n; ++j) {
      if (!d[j].candidate || !vh_fuse_same_key(d[i], d[j])) continue;
      if ((uint64_t)d[i].lds_bytes + d[j].lds_bytes <= VH_BATCH_LDS_CAP) CHECK(g[i] >= 0 && g[i] == g[j], "members %u and %u open their key and fit: groups %d and %d", i, j, g[i], g[j]);
      else CHECK(g[i] == -1, "member %u cannot take the next candidate of its key and is in group %d", i, g[i]);
      break;
    }
  }
  if (out_groups) out_groups->assign(g, g + n);
  free(d); free(g);
  return ng;
}

int main() {
  std::vector<int32_t> g;
  // no member, one member
  CHECK(check_list({}) == 0, "empty list");
  CHECK(check_list({cand(1, 64)}, &g) == 0 && g[0] == -1, "a lone candidate is single");
  CHECK(check_list({other()}, &g) == 0 && g[0] == -1, "a non-candidate is single");
  // 8 equal candidates: one group, plan order
  {
    std::vector<VhFuseDesc> l(8, cand(7, 1024));
    CHECK(check_list(l, &g) == 1, "8 equal candidates make one group");
    for (int i = 0; i < 8; ++i) CHECK(g[i] == 0, "member %d in group %d", i, g[i]);
  }
  // 8 candidates whose tables sum past 48 KB split: 7 KB each -> 6 fit (42 KB), the seventh opens the next group
  {
    std::vector<VhFuseDesc> l(8, cand(7, 7 * 1024));
    CHECK(check_list(l, &g) == 2, "8 x 7 KB split");
    for (int i = 0; i < 8; ++i) CHECK(g[i] == (i < 6 ? 0 : 1), "member %d in group %d", i, g[i]);
  }
  // ... and where the remainder is ONE member, it is single
  {
    std::vector<VhFuseDesc> l(7, cand(7, 8 * 1024));
    CHECK(check_list(l, &g) == 1, "7 x 8 KB: six and one");
    CHECK(g[6] == -1, "the seventh is alone: single, not a group of one (%d)", g[6]);
  }
  // exactly 48 KB fits; one byte more does not
  {
    CHECK(check_list({cand(1, 24 * 1024), cand(1, 24 * 1024)}, &g) == 1 && g[0] == 0 && g[1] == 0, "48 KB fits");
    CHECK(check_list({cand(1, 24 * 1024), cand(1, 24 * 1024 + 16)}, &g) == 0 && g[0] == -1 && g[1] == -1, "48 KB + 16 does not");
    CHECK(check_list({cand(1, 64 * 1024), cand(1, 64), cand(1, 64)}, &g) == 1 && g[0] == -1 && g[1] == 0 && g[2] == 0, "a member past the cap alone is single, the others group");
  }
  // more than VH_BATCH_MAX members of one key (longer lists than the entry point takes: the function is general)
  {
    std::vector<VhFuseDesc> l(19, cand(3, 64));
    CHECK(check_list(l, &g) == 3, "19 members: 8 + 8 + 3");
    for (int i = 0; i < 19; ++i) CHECK(g[i] == i / 8, "member %d in group %d", i, g[i]);
    l.assign(17, cand(3, 64));
    CHECK(check_list(l, &g) == 2 && g[16] == -1, "17 members: 8 + 8 and a single");
  }
  // every component of the key separates; non-candidates in between are never grouped and break nothing
  {
    std::vector<VhFuseDesc> l = {cand(1, 64), other(), cand(2, 64), cand(1, 64, 1), cand(1, 64), cand(1, 64, 0, 4), cand(1, 64, 0, 3, 5), cand(2, 64), other(), cand(1, 64, 1)};
    CHECK(check_list(l, &g) == 3, "mixed keys");
    const int32_t want[] = {0, -1, 1, 2, 0, -1, -1, 1, -1, 2};
    for (int i = 0; i < 10; ++i) CHECK(g[i] == want[i], "member %d in group %d, expected %d", i, g[i], want[i]);
  }
  // a batch with exactly one candidate among others
  CHECK(check_list({other(), cand(1, 64), other(), other()}, &g) == 0 && g[1] == -1, "one candidate: nothing fused");

  // random lists
  std::mt19937 rng(12345);
  for (int round = 0; round < 20000; ++round) {
    const uint32_t n = rng() % 25;
    std::vector<VhFuseDesc> l;
    for (uint32_t i = 0; i < n; ++i) {
      VhFuseDesc d = cand(1 + rng() % 3, 0, rng() % 2, 3 + rng() % 2, 4 + rng() % 2);
      const uint32_t kind = rng() % 8;
      d.lds_bytes = kind == 0 ? 16 * (1 + rng() % 4096) : kind == 1 ? 24 * 1024 : 16 * (1 + rng() % 64);
      d.candidate = rng() % 4 != 0;
      if (round % 2) { d.scope = 0; d.nseg = 3; d.chunks_per_seg = 4; d.v_serial = 1 + rng() % 2; }      // (few keys: long groups, cap breaks)
      l.push_back(d);
    }
    check_list(l);
  }
  printf("ok: %d checks\n", g_checks);
  return 0;
}
