// Which members of one fused launch share a pass mask (viyadb_amd/csrc/vh_batch.h: vh_batch_share), run on the CPU over hand-made and random
// member lists. A stand-alone program: tests/test_batch_share_host.py builds it plain and with AddressSanitizer / UndefinedBehaviorSanitizer
// (programs, literals, snapshots and the lists themselves are exact-size heap blocks, so a read outside the used part is an error).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "vh_batch.h"

static int g_checks = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
  } while (0)

enum { K_TRUE = 0, K_REL = 1, K_IN = 2, K_AND = 3, K_OR = 4, K_INSET = 5 };      // enum vh_fkind
enum { OP_LT = 2, OP_LE = 3 };                                                   // (any two relations: the rule compares the word)

struct Op { uint32_t w0, w1; };
static Op op(uint32_t kind, uint32_t rel, uint32_t count, uint32_t lit, uint32_t off, uint32_t bits) {      // vh_bits_op (vh_bits_eval.h), type u32 = 2
  return Op{kind | 2u << 8 | rel << 16 | count << 24, lit | off << 16 | bits << 24};
}

// A member as the test holds it; desc() lays it out in exact-size blocks of its own.
struct Member {
  uint32_t has_filter = 1;
  uint64_t serial = 7, planes = 0x1000, stride = 4096, pitch = 256;
  int32_t flat = 1;
  std::vector<Op> ops;             // the used ops
  std::vector<uint64_t> lits;      // the literals there is room for
  std::vector<uint32_t> rows;
};
struct Laid {
  std::unique_ptr<uint32_t[]> ops; std::unique_ptr<uint64_t[]> lits; std::unique_ptr<uint32_t[]> rows;
  VhShareDesc d{};
};
// `slack_ops`: staged ops beyond nprog, filled with `junk` — the staging block is larger than the used part and the rule must not look there.
static Laid lay(const Member& m, uint32_t slack_ops = 0, uint32_t junk = 0) {
  Laid l;
  const size_t no = m.ops.size() + slack_ops;
  l.ops.reset(new uint32_t[no ? 2 * no : 1]);
  for (size_t k = 0; k < m.ops.size(); ++k) { l.ops[2 * k] = m.ops[k].w0; l.ops[2 * k + 1] = m.ops[k].w1; }
  for (size_t k = m.ops.size(); k < no; ++k) { l.ops[2 * k] = junk; l.ops[2 * k + 1] = junk * 3u + 1u; }
  l.lits.reset(new uint64_t[m.lits.size() ? m.lits.size() : 1]);
  for (size_t k = 0; k < m.lits.size(); ++k) l.lits[k] = m.lits[k];
  l.rows.reset(new uint32_t[m.rows.size() ? m.rows.size() : 1]);
  for (size_t k = 0; k < m.rows.size(); ++k) l.rows[k] = m.rows[k];
  VhShareDesc& d = l.d;
  d.has_filter = m.has_filter; d.f_serial = m.serial; d.f_planes = m.planes; d.f_stride = m.stride; d.f_pitch = m.pitch;
  d.nprog = (int32_t)m.ops.size(); d.flat = m.flat; d.ops = l.ops.get(); d.lits = l.lits.get(); d.nlits = (uint32_t)m.lits.size();
  d.nseg = (uint32_t)m.rows.size(); d.seg_rows = l.rows.get();
  return l;
}

// C3's filter: d2 == 1 & d3 < 447 & d4 >= 553, over fields of 2, 10 and 10 planes
static Member c3() {
  Member m;
  m.ops = {op(K_REL, 0, 0, 0, 0, 2), op(K_REL, OP_LT, 0, 1, 2, 10), op(K_REL, 5, 0, 2, 12, 10), op(K_AND, 0, 3, 0, 0, 0)};
  m.lits = {1, 447, 553};
  m.rows = {5000, 5000, 5000};
  return m;
}
static Member none() { Member m; m.has_filter = 0; m.flat = 0; m.rows = {5000, 5000, 5000}; return m; }

// the key of §"which members share" written out naively on the test's own representation
static bool naive_same(const Member& a, const Member& b) {
  if (a.has_filter != b.has_filter || a.rows != b.rows) return false;
  if (!a.has_filter) return true;
  if (a.serial != b.serial || a.planes != b.planes || a.stride != b.stride || a.pitch != b.pitch || a.flat != b.flat || a.ops.size() != b.ops.size()) return false;
  for (size_t k = 0; k < a.ops.size(); ++k) {
    if (a.ops[k].w0 != b.ops[k].w0 || a.ops[k].w1 != b.ops[k].w1) return false;
    const uint32_t kind = a.ops[k].w0 & 0xFF;
    if (kind == K_INSET) return false;
    const uint32_t n = kind == K_REL ? 1 : kind == K_IN ? a.ops[k].w0 >> 24 : 0, first = a.ops[k].w1 & 0xFFFF;
    if (first + n > a.lits.size() || first + n > b.lits.size()) return false;      // (a program nobody may share with: the rule refuses it too)
    for (uint32_t i = 0; i < n; ++i) if (a.lits[first + i] != b.lits[first + i]) return false;
  }
  return true;
}

// the properties every answer has, and the answer itself; `order`: the launch's members as indices into the list
static std::vector<uint32_t> share(const std::vector<Member>& ms, std::vector<uint32_t> order = {}, uint32_t* classes_out = nullptr) {
  if (order.empty()) for (uint32_t i = 0; i < ms.size(); ++i) order.push_back(i);
  std::vector<Laid> laid;
  for (size_t i = 0; i < ms.size(); ++i) laid.push_back(lay(ms[i], (uint32_t)(i % 3), 0xA5A50000u + (uint32_t)i));      // (unused ops differ from member to member)
  const uint32_t n = (uint32_t)ms.size(), cnt = (uint32_t)order.size();
  VhShareDesc* d = (VhShareDesc*)malloc(sizeof(VhShareDesc) * (n ? n : 1));
  uint32_t* idx = (uint32_t*)malloc(sizeof(uint32_t) * (cnt ? cnt : 1));
  uint32_t* mo = (uint32_t*)malloc(sizeof(uint32_t) * (cnt ? cnt : 1));
  for (uint32_t i = 0; i < n; ++i) d[i] = laid[i].d;
  for (uint32_t k = 0; k < cnt; ++k) idx[k] = order[k];
  const uint32_t classes = vh_batch_share(d, idx, cnt, mo);
  uint32_t own = 0;
  for (uint32_t k = 0; k < cnt; ++k) {
    CHECK(mo[k] <= k, "member %u uses the mask of a later member %u", k, mo[k]);
    CHECK(mo[mo[k]] == mo[k], "member %u uses member %u, which does not evaluate its own", k, mo[k]);
    own += mo[k] == k;
    // it shares with the FIRST member of an equal key, and with nobody where there is none
    uint32_t want = k;
    for (uint32_t j = 0; j < k; ++j) if (naive_same(ms[order[j]], ms[order[k]])) { want = j; break; }
    CHECK(mo[k] == want, "member %u: mask_of %u, the pairwise comparison says %u", k, mo[k], want);
    for (uint32_t j = 0; j < cnt; ++j)
      if (j != k) CHECK((mo[j] == mo[k]) == naive_same(ms[order[j]], ms[order[k]]), "members %u and %u: classes %u and %u", j, k, mo[j], mo[k]);
  }
  CHECK(classes == own, "%u classes reported, %u members evaluate", classes, own);
  if (classes_out) *classes_out = classes;
  std::vector<uint32_t> out(mo, mo + cnt);
  free(d); free(idx); free(mo);
  return out;
}
static bool shares(const Member& a, const Member& b) { return share({a, b})[1] == 0; }

int main() {
  uint32_t classes = 0;
  CHECK(share({}, {}, &classes).empty() && classes == 0, "no member");
  CHECK(share({c3()}, {}, &classes)[0] == 0 && classes == 1, "one member");
  CHECK(shares(c3(), c3()), "identical twins share");

  // every part of the key separates
  { Member b = c3(); b.lits[1] = 448; CHECK(!shares(c3(), b), "d3 < 447 / d3 < 448"); }
  { Member b = c3(); b.ops[1] = op(K_REL, OP_LE, 0, 1, 2, 10); CHECK(!shares(c3(), b), "lt / le"); }
  { Member b = c3(); b.ops[3] = op(K_OR, 0, 3, 0, 0, 0); b.flat = 2; CHECK(!shares(c3(), b), "AND / OR"); }
  { Member b = c3(); b.flat = 0; CHECK(!shares(c3(), b), "flat"); }
  { Member b = c3(); b.serial = 8; CHECK(!shares(c3(), b), "F's serial"); }
  { Member b = c3(); b.pitch = 512; CHECK(!shares(c3(), b), "F's pitch"); }
  { Member b = c3(); b.stride = 8192; CHECK(!shares(c3(), b), "F's stride"); }
  { Member b = c3(); b.planes = 0x2000; CHECK(!shares(c3(), b), "F's planes"); }
  { Member b = c3(); b.rows[2] = 4999; CHECK(!shares(c3(), b), "one row fewer in the last segment"); }
  { Member b = c3(); b.rows[1] = 0; CHECK(!shares(c3(), b), "a skipped segment"); }
  { Member b = c3(); b.rows.push_back(0); CHECK(!shares(c3(), b), "another number of segments"); }
  { Member b = c3(); b.ops.pop_back(); b.ops.pop_back(); b.ops.push_back(op(K_AND, 0, 2, 0, 0, 0)); CHECK(!shares(c3(), b), "a shorter program"); }
  { Member b = c3(); b.has_filter = 0; CHECK(!shares(c3(), b), "has_filter"); CHECK(!shares(none(), c3()), "has_filter, the other way"); }

  // no filter: equal rows share whatever else the descriptor holds; other rows do not
  { Member b = none(); b.serial = 99; b.pitch = 1; CHECK(shares(none(), b), "no filter, equal rows"); }
  { Member b = none(); b.rows[0] = 4096; CHECK(!shares(none(), b), "no filter, other rows"); }

  // what the program does not use does not matter: a literal no op refers to (the ops beyond nprog differ in every list: share())
  { Member a = c3(), b = c3(); a.lits.push_back(1); b.lits.push_back(2); CHECK(shares(a, b), "an unused literal"); }
  // an IN leaf: all of its literals count, the ones behind them do not
  {
    Member a = c3(); a.ops[1] = op(K_IN, 1, 3, 2, 2, 10); a.lits = {1, 5, 10, 20, 30, 40};      // the list: lits[2 .. 5)
    a.ops[2] = op(K_TRUE, 0, 0, 0, 0, 0);
    Member b = a; b.lits[5] = 41; CHECK(shares(a, b), "IN: a literal behind the list");
    b = a; b.lits[4] = 31; CHECK(!shares(a, b), "IN: the last literal of the list");
    b = a; b.lits[2] = 11; CHECK(!shares(a, b), "IN: the first literal of the list");
    b = a; b.lits[1] = 6; CHECK(shares(a, b), "IN: a literal in front of the list");
  }
  // a set leaf never shares, even with an identical twin
  {
    Member a = c3(); a.ops[1] = op(K_INSET, 1, 8, 0, 2, 10);
    CHECK(!shares(a, a), "a set leaf and its twin");
    std::vector<uint32_t> mo = share({a, c3(), a, c3()}, {}, &classes);
    CHECK(mo[0] == 0 && mo[1] == 1 && mo[2] == 2 && mo[3] == 1 && classes == 3, "set leaves among others");
  }
  // an op whose literals lie beyond the program's: nobody shares with it, and nothing is read there
  { Member a = c3(); a.ops[1] = op(K_REL, OP_LT, 0, 3, 2, 10); CHECK(!shares(a, a), "a literal index past the end"); }

  // eight equal members: one class; eight different ones: eight
  {
    std::vector<Member> l(8, c3());
    std::vector<uint32_t> mo = share(l, {}, &classes);
    CHECK(classes == 1, "8 equal members: %u classes", classes);
    for (int k = 0; k < 8; ++k) CHECK(mo[k] == 0, "member %d uses %u", k, mo[k]);
    for (int k = 0; k < 8; ++k) l[k].lits[1] = 440 + k;
    mo = share(l, {}, &classes);
    CHECK(classes == 8, "8 different members: %u classes", classes);
    for (int k = 0; k < 8; ++k) CHECK(mo[k] == (uint32_t)k, "member %d uses %u", k, mo[k]);
  }
  // A, B, A, none, B, none, A: three classes, the followers point at the first of theirs; mask_of is a position in the LAUNCH, not in the list
  {
    Member A = c3(), B = c3(); B.lits[1] = 448;
    std::vector<Member> l = {A, B, A, none(), B, none(), A};
    std::vector<uint32_t> mo = share(l, {}, &classes);
    const uint32_t want[] = {0, 1, 0, 3, 1, 3, 0};
    CHECK(classes == 3, "%u classes", classes);
    for (int k = 0; k < 7; ++k) CHECK(mo[k] == want[k], "member %d uses %u, expected %u", k, mo[k], want[k]);
    mo = share(l, {4, 6, 1, 5, 2}, &classes);      // B A B none A
    const uint32_t want2[] = {0, 1, 0, 3, 1};
    CHECK(classes == 3, "%u classes of a sub-list", classes);
    for (int k = 0; k < 5; ++k) CHECK(mo[k] == want2[k], "sub-list member %d uses %u, expected %u", k, mo[k], want2[k]);
  }

  // random lists of few variants: every answer against the pairwise comparison (share() checks)
  std::mt19937 rng(4242);
  for (int round = 0; round < 20000; ++round) {
    const uint32_t n = rng() % 9;
    std::vector<Member> l;
    for (uint32_t i = 0; i < n; ++i) {
      Member m = rng() % 4 == 0 ? none() : c3();
      switch (rng() % 12) {
        case 0: if (m.has_filter) m.lits[rng() % 3] ^= 1; break;
        case 1: if (m.has_filter) m.ops[1] = op(K_REL, OP_LE, 0, 1, 2, 10); break;
        case 2: m.flat = m.has_filter ? 0 : m.flat; break;
        case 3: m.serial = 8; break;
        case 4: m.pitch = 512; break;
        case 5: m.rows[rng() % 3] -= 1; break;
        case 6: m.rows[rng() % 3] = 0; break;
        case 7: if (m.has_filter) m.ops[1] = op(K_INSET, 1, 8, 0, 2, 10); break;
        case 8: m.lits.push_back(rng()); break;
        default: break;
      }
      l.push_back(m);
    }
    share(l);
    if (n > 2) { std::vector<uint32_t> sub; for (uint32_t i = 0; i < n; ++i) if (rng() % 2) sub.push_back(i); if (!sub.empty()) share(l, sub); }
  }
  printf("ok: %d checks\n", g_checks);
  return 0;
}
