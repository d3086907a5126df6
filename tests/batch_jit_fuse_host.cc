// Compiled and pre-built candidates of a batch (viyadb_amd/csrc/vh_batch.h: VhFuseDesc::compiled, VhShareDesc::filter_shape), run on the CPU over
// hand-made and random lists. A stand-alone program in the style of tests/batch_fuse_host.cc: tests/test_batch_jit_fuse_host.py builds it plain
// and with AddressSanitizer / UndefinedBehaviorSanitizer (the lists are exact-size heap blocks, so an index outside them is an error).
//   * vh_batch_group: compiled candidates group with compiled candidates only, pre-built ones with pre-built ones; the caps (VH_BATCH_MAX members,
//     VH_BATCH_LDS_CAP bytes) apply per group; a lone candidate of either kind stays -1. Every output equals that of a brute-force restatement:
//     the list split by kind, each half grouped without the field, the groups numbered by their first members.
//   * vh_batch_share with the stricter rule: members of unequal filter member-shapes never share, equal ones share exactly as without the field,
//     and mask_of[k] <= k, mask_of[mask_of[k]] == mask_of[k] throughout.
#include <algorithm>
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

static VhFuseDesc cand(uint32_t compiled, uint64_t v, uint32_t lds, uint32_t scope = 0) {
  VhFuseDesc d{};
  d.candidate = 1; d.scope = scope; d.v_serial = v; d.nseg = 3; d.chunks_per_seg = 4; d.lds_bytes = lds; d.compiled = compiled;
  return d;
}
static VhFuseDesc other(uint32_t compiled = 0) { VhFuseDesc d{}; d.v_serial = 1; d.nseg = 3; d.chunks_per_seg = 4; d.lds_bytes = 64; d.compiled = compiled; return d; }

// the grouping written out naively: ONE kind's candidates at a time, by the rule without the field (an opener takes the later candidates of
// its key while the caps hold and stops at the first that does not fit); then the groups of both kinds numbered by their first members
static std::vector<int32_t> brute(const std::vector<VhFuseDesc>& d) {
  const size_t n = d.size();
  std::vector<int32_t> first(n, -1);      // the group's first member, -1: single
  for (uint32_t kind = 0; kind < 2; ++kind) {
    std::vector<char> taken(n, 0);
    for (size_t i = 0; i < n; ++i) {
      if (!d[i].candidate || (d[i].compiled != 0) != (kind != 0) || taken[i]) continue;
      std::vector<size_t> g = {i};
      uint64_t lds = d[i].lds_bytes;
      for (size_t k = i + 1; k < n; ++k) {
        if (!d[k].candidate || (d[k].compiled != 0) != (kind != 0) || taken[k]) continue;
        if (d[k].v_serial != d[i].v_serial || d[k].scope != d[i].scope || d[k].nseg != d[i].nseg || d[k].chunks_per_seg != d[i].chunks_per_seg) continue;
        if (g.size() == VH_BATCH_MAX || lds + d[k].lds_bytes > VH_BATCH_LDS_CAP) break;
        g.push_back(k); lds += d[k].lds_bytes;
      }
      if (g.size() > 1) for (size_t k : g) { taken[k] = 1; first[k] = (int32_t)i; }
    }
  }
  std::vector<int32_t> firsts;
  for (size_t i = 0; i < n; ++i) if (first[i] == (int32_t)i) firsts.push_back((int32_t)i);
  std::vector<int32_t> out(n, -1);
  for (size_t i = 0; i < n; ++i)
    if (first[i] >= 0) out[i] = (int32_t)(std::find(firsts.begin(), firsts.end(), first[i]) - firsts.begin());
  return out;
}

static uint32_t check_list(const std::vector<VhFuseDesc>& in, std::vector<int32_t>* out_groups = nullptr) {
  const uint32_t n = (uint32_t)in.size();
  VhFuseDesc* d = (VhFuseDesc*)malloc(sizeof(VhFuseDesc) * (n ? n : 1));      // exact size: the sanitizer sees an index past the end
  int32_t* g = (int32_t*)malloc(sizeof(int32_t) * (n ? n : 1));
  for (uint32_t i = 0; i < n; ++i) d[i] = in[i];
  const uint32_t ng = vh_batch_group(d, n, g);
  const std::vector<int32_t> want = brute(in);
  int32_t top = -1;
  std::map<int32_t, std::vector<uint32_t>> members;
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(g[i] == want[i], "member %u: group %d, the restatement says %d", i, g[i], want[i]);
    top = std::max(top, g[i]);
    if (!d[i].candidate) CHECK(g[i] == -1, "member %u is no candidate and in group %d", i, g[i]);
    if (g[i] >= 0) members[g[i]].push_back(i);
  }
  CHECK((uint32_t)(top + 1) == ng && members.size() == ng, "%u groups reported, the largest number is %d", ng, top);
  for (auto& kv : members) {
    const std::vector<uint32_t>& m = kv.second;
    CHECK(m.size() >= 2 && m.size() <= VH_BATCH_MAX, "group %d has %zu members", kv.first, m.size());
    uint64_t lds = 0;
    for (uint32_t i : m) {
      CHECK((d[i].compiled != 0) == (d[m[0]].compiled != 0), "group %d mixes a compiled and a pre-built candidate (%u, %u)", kv.first, m[0], i);
      CHECK(vh_fuse_same_key(d[m[0]], d[i]), "group %d: members %u and %u differ in the key", kv.first, m[0], i);
      lds += d[i].lds_bytes;
    }
    CHECK(lds <= VH_BATCH_LDS_CAP, "group %d: %llu bytes of LDS", kv.first, (unsigned long long)lds);
  }
  if (out_groups) out_groups->assign(g, g + n);
  free(d); free(g);
  return ng;
}

// ---- the share rule: members are (has_filter, filter_shape, program id); equal program ids stand for equal staged programs and literals
struct Sh { uint32_t has_filter, shape, prog, rows; };
static void check_share(const std::vector<Sh>& ms) {
  const uint32_t n = (uint32_t)ms.size();
  // one REL op per member: w0 = kind, w1 = literal 0; the literal carries the program id
  uint32_t* ops = (uint32_t*)malloc(sizeof(uint32_t) * 2 * (n ? n : 1));
  uint64_t* lits = (uint64_t*)malloc(sizeof(uint64_t) * (n ? n : 1));
  uint32_t* rows = (uint32_t*)malloc(sizeof(uint32_t) * (n ? n : 1));
  VhShareDesc* d = (VhShareDesc*)malloc(sizeof(VhShareDesc) * (n ? n : 1));
  uint32_t* idx = (uint32_t*)malloc(sizeof(uint32_t) * (n ? n : 1));
  uint32_t* mo = (uint32_t*)malloc(sizeof(uint32_t) * (n ? n : 1));
  for (uint32_t i = 0; i < n; ++i) {
    ops[2 * i] = VH_SHARE_KIND_REL; ops[2 * i + 1] = 0; lits[i] = ms[i].prog; rows[i] = ms[i].rows; idx[i] = i;
    VhShareDesc s{};
    s.has_filter = ms[i].has_filter; s.f_serial = 7; s.f_planes = 0x1000; s.f_stride = 4096; s.f_pitch = 256;
    s.nprog = 1; s.flat = 1; s.ops = ops + 2 * i; s.lits = lits + i; s.nlits = 1; s.nseg = 1; s.seg_rows = rows + i;
    s.filter_shape = ms[i].shape;
    d[i] = s;
  }
  auto same = [&](uint32_t a, uint32_t b) {
    if (ms[a].has_filter != ms[b].has_filter || ms[a].shape != ms[b].shape || ms[a].rows != ms[b].rows) return false;
    return !ms[a].has_filter || ms[a].prog == ms[b].prog;
  };
  const uint32_t classes = vh_batch_share(d, idx, n, mo);
  uint32_t own = 0;
  for (uint32_t k = 0; k < n; ++k) {
    CHECK(mo[k] <= k, "member %u uses the mask of a later member %u", k, mo[k]);
    CHECK(mo[mo[k]] == mo[k], "member %u uses member %u, which does not evaluate its own", k, mo[k]);
    own += mo[k] == k;
    uint32_t want = k;
    for (uint32_t j = 0; j < k; ++j) if (same(j, k)) { want = j; break; }
    CHECK(mo[k] == want, "member %u: mask_of %u, the pairwise comparison says %u", k, mo[k], want);
    if (mo[k] != k) CHECK(ms[mo[k]].shape == ms[k].shape, "members %u and %u share across filter shapes %u and %u", mo[k], k, ms[mo[k]].shape, ms[k].shape);
  }
  CHECK(classes == own, "%u classes reported, %u members evaluate", classes, own);
  free(ops); free(lits); free(rows); free(d); free(idx); free(mo);
}

int main() {
  std::vector<int32_t> g;
  // a mixed list forms separate groups, numbered by their first members
  {
    std::vector<VhFuseDesc> l = {cand(1, 7, 64), cand(0, 7, 64), cand(1, 7, 64), cand(0, 7, 64), other(1), cand(1, 7, 64)};
    CHECK(check_list(l, &g) == 2, "two kinds, two groups");
    const int32_t want[] = {0, 1, 0, 1, -1, 0};
    for (int i = 0; i < 6; ++i) CHECK(g[i] == want[i], "member %d in group %d, expected %d", i, g[i], want[i]);
  }
  // lone candidates of either kind stay -1, next to a group of the other kind
  CHECK(check_list({cand(1, 7, 64), cand(0, 7, 64)}, &g) == 0 && g[0] == -1 && g[1] == -1, "one of each kind: nothing fused");
  CHECK(check_list({cand(1, 7, 64), cand(0, 7, 64), cand(0, 7, 64)}, &g) == 1 && g[0] == -1 && g[1] == 0 && g[2] == 0, "a lone compiled candidate beside a pre-built pair");
  CHECK(check_list({cand(0, 7, 64), cand(1, 7, 64), cand(1, 7, 64)}, &g) == 1 && g[0] == -1 && g[1] == 0 && g[2] == 0, "a lone pre-built candidate beside a compiled pair");
  // the caps apply per group: 8 + 8 members of the two kinds interleaved make two full groups, a ninth of one kind is single
  {
    std::vector<VhFuseDesc> l;
    for (int i = 0; i < 16; ++i) l.push_back(cand(i % 2, 3, 64));
    l.push_back(cand(1, 3, 64));
    CHECK(check_list(l, &g) == 2, "8 + 8 interleaved");
    for (int i = 0; i < 16; ++i) CHECK(g[i] == (i % 2 ? 1 : 0), "member %d in group %d", i, g[i]);
    CHECK(g[16] == -1, "the ninth compiled candidate is alone (%d)", g[16]);
  }
  // ... and the LDS cap: 24 KB tables — two of a kind fill a group, whatever the other kind holds
  {
    std::vector<VhFuseDesc> l = {cand(1, 1, 24 * 1024), cand(0, 1, 24 * 1024), cand(1, 1, 24 * 1024), cand(0, 1, 24 * 1024), cand(1, 1, 24 * 1024), cand(1, 1, 24 * 1024)};
    CHECK(check_list(l, &g) == 3, "48 KB per group");
    const int32_t want[] = {0, 1, 0, 1, 2, 2};
    for (int i = 0; i < 6; ++i) CHECK(g[i] == want[i], "member %d in group %d, expected %d", i, g[i], want[i]);
  }
  // any non-zero value means compiled
  CHECK(check_list({cand(1, 7, 64), cand(2, 7, 64)}, &g) == 1 && g[0] == 0 && g[1] == 0, "compiled is a truth value");

  std::mt19937 rng(4242);
  for (int round = 0; round < 6000; ++round) {
    const uint32_t n = rng() % 25;
    std::vector<VhFuseDesc> l;
    for (uint32_t i = 0; i < n; ++i) {
      VhFuseDesc d = cand(rng() % 2, 1 + rng() % 2, 0, round % 2 ? 0 : rng() % 2);
      const uint32_t kind = rng() % 8;
      d.lds_bytes = kind == 0 ? 16 * (1 + rng() % 4096) : kind == 1 ? 24 * 1024 : 16 * (1 + rng() % 64);
      d.candidate = rng() % 4 != 0;
      l.push_back(d);
    }
    check_list(l);
  }

  // the share rule
  check_share({});
  check_share({{1, 1, 5, 5000}, {1, 1, 5, 5000}});                        // equal in everything: they share
  check_share({{1, 1, 5, 5000}, {1, 2, 5, 5000}});                        // the same staged program under another filter text: they do not
  check_share({{1, 1, 5, 5000}, {1, 2, 5, 5000}, {1, 1, 5, 5000}, {1, 2, 5, 5000}, {0, 3, 0, 5000}, {0, 3, 1, 5000}, {0, 4, 0, 5000}});
  for (int round = 0; round < 4000; ++round) {
    const uint32_t n = rng() % (VH_BATCH_MAX + 1);
    std::vector<Sh> ms;
    for (uint32_t i = 0; i < n; ++i) ms.push_back(Sh{rng() % 4 != 0, 1 + rng() % 3, rng() % 3, 5000 - rng() % 2});
    check_share(ms);
  }
  printf("ok: %d checks\n", g_checks);
  return 0;
}
