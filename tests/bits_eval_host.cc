// Host check of the bit-serial filter evaluator (viyadb_amd/csrc/vh_bits_eval.h, plain C++, no GPU): for random plane words, vh_bits_eval over
// a postfix program must agree, row by row, with an evaluation of the same program on each row's values in the columns' own types.
// A stand-alone program (tests/test_bits_eval_host.py compiles and runs it, once plain and once with -fsanitize=address,undefined).
// The planes are an exact-size heap block (nplanes x pitch bytes): a read outside a field's planes or past the last word is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vh_bits_eval.h"

static long g_rows = 0, g_progs = 0;
static int g_fail = 0;

struct Field { int off, bits, type; };      // planes [off, off + bits) hold a column of element type `type`

struct Leaf { int kind, field, op; std::vector<uint64_t> lits; };      // lits: raw bits as the C ABI carries them (the value's low bytes)

// the literal as the column's type sees it
static void decode(int type, uint64_t bits, bool* sgn, int64_t* s, uint64_t* u) {
  *sgn = type >= VH_I8 && type <= VH_I64;
  switch (type) {
    case VH_U8: *u = (uint8_t)bits; break;
    case VH_U16: *u = (uint16_t)bits; break;
    case VH_U32: *u = (uint32_t)bits; break;
    case VH_U64: *u = bits; break;
    case VH_I8: *s = (int8_t)bits; break;
    case VH_I16: *s = (int16_t)bits; break;
    case VH_I32: *s = (int32_t)bits; break;
    default: *s = (int64_t)bits; break;
  }
}
// (value OP literal) in the column's type: the value is non-negative and fits the type
static bool row_rel(int type, uint64_t v, int op, uint64_t litbits) {
  bool sgn; int64_t s = 0; uint64_t u = 0;
  decode(type, litbits, &sgn, &s, &u);
  int r;
  if (sgn) r = (int64_t)v < s ? -1 : (int64_t)v > s ? 1 : 0;
  else r = v < u ? -1 : v > u ? 1 : 0;
  switch (op) {
    case VH_OP_EQ: return r == 0;
    case VH_OP_NE: return r != 0;
    case VH_OP_LT: return r < 0;
    case VH_OP_LE: return r <= 0;
    case VH_OP_GT: return r > 0;
    default: return r >= 0;
  }
}
static bool row_leaf(const Leaf& l, const Field& f, uint64_t v) {
  if (l.kind == VH_F_REL) return row_rel(f.type, v, l.op, l.lits[0]);
  bool any = false;      // IN, and a set leaf: membership, the list as the caller gave it
  for (uint64_t b : l.lits) any |= row_rel(f.type, v, VH_OP_EQ, b);
  return l.op ? any : !any;
}

// A program as the test writes it: leaves by index, AND / OR nodes as (-kind, count)
struct Node { int leaf; int kind, count; };

struct Case {
  std::vector<Field> fields;
  std::vector<Leaf> leaves;
  std::vector<Node> prog;
  int flat = 0;
};

static bool row_eval(const Case& c, const std::vector<uint64_t>& vals) {
  std::vector<bool> st;
  for (const Node& n : c.prog) {
    if (n.leaf >= 0) { const Leaf& l = c.leaves[(size_t)n.leaf]; st.push_back(row_leaf(l, c.fields[(size_t)l.field], vals[(size_t)l.field])); continue; }
    bool a = st.back(); st.pop_back();
    for (int i = 1; i < n.count; ++i) { const bool b = st.back(); st.pop_back(); a = n.kind == VH_F_AND ? (a & b) : (a | b); }
    st.push_back(a);
  }
  return st[0];
}

static void run_case(const Case& c, std::mt19937_64& rng, const char* what) {
  ++g_progs;
  int nplanes = 0;
  for (const Field& f : c.fields) nplanes = f.off + f.bits > nplanes ? f.off + f.bits : nplanes;
  const uint32_t nwords = 3;
  const uint64_t pitch = nwords * 4;
  std::vector<uint32_t> planes((size_t)nplanes * nwords);      // exact size
  for (uint32_t& w : planes) { const int mode = (int)(rng() % 8); w = mode == 0 ? 0u : mode == 1 ? ~0u : (uint32_t)rng(); }
  // ... and some rows that hold a leaf's literals and their neighbours (random 31-bit values would never meet them)
  for (const Leaf& l : c.leaves) {
    const Field& f = c.fields[(size_t)l.field];
    for (int k = 0; k < 8; ++k) {
      bool sgn; int64_t s = 0; uint64_t u = 0;
      decode(f.type, l.lits[(size_t)(rng() % l.lits.size())], &sgn, &s, &u);
      const uint64_t v = ((sgn ? (uint64_t)s : u) + (uint64_t)(rng() % 3) - 1u) & ((1ull << f.bits) - 1ull);
      const uint32_t w = (uint32_t)(rng() % nwords), i = (uint32_t)(rng() % 32);
      for (int b = 0; b < f.bits; ++b) {
        uint32_t& word = planes[(size_t)(f.off + b) * nwords + w];
        word = (word & ~(1u << i)) | (uint32_t)((v >> b) & 1u) << i;
      }
    }
  }
  // the program, its literals and its sets
  VhBitsProg B{};
  std::vector<VhSetHost> sets;
  std::vector<std::vector<uint32_t>> tables;
  std::vector<VhSetDev> devs;
  int nlits = 0, maxdepth = 0, depth = 0;
  B.nprog = (int32_t)c.prog.size(); B.flat = c.flat;
  if (c.prog.size() > VH_BITS_MAX_PROG) { printf("FAIL %s: the test's program is too long\n", what); ++g_fail; return; }
  for (const Leaf& l : c.leaves) if (l.kind == VH_F_INSET) {
    const Field& f = c.fields[(size_t)l.field];
    sets.emplace_back();
    vh_inset_build(f.type, l.lits.data(), l.lits.size(), false, &sets.back());
    vh_inset_truth_build(f.type, f.bits, &sets.back());
  }
  for (const VhSetHost& h : sets) tables.emplace_back(h.words);
  for (size_t k = 0; k < sets.size(); ++k) devs.push_back(sets[k].dev(tables[k].data()));
  B.set = devs.data();
  std::vector<int> set_of(c.leaves.size(), -1);
  { int k = 0; for (size_t i = 0; i < c.leaves.size(); ++i) if (c.leaves[i].kind == VH_F_INSET) set_of[i] = k++; }
  std::vector<int> lit_of(c.leaves.size(), 0);
  for (size_t i = 0; i < c.leaves.size(); ++i) {
    if (c.leaves[i].kind == VH_F_INSET) continue;
    lit_of[i] = nlits;
    for (uint64_t b : c.leaves[i].lits) { if (nlits >= VH_BITS_MAX_LITS) { printf("FAIL %s: too many literals\n", what); ++g_fail; return; } B.lits[nlits++] = b; }
  }
  for (size_t k = 0; k < c.prog.size(); ++k) {
    const Node& n = c.prog[k];
    if (n.leaf >= 0) {
      const Leaf& l = c.leaves[(size_t)n.leaf];
      const Field& f = c.fields[(size_t)l.field];
      B.op[k] = vh_bits_op((uint32_t)l.kind, (uint32_t)f.type, (uint32_t)l.op, l.kind == VH_F_IN ? (uint32_t)l.lits.size() : 0u,
                           (uint32_t)(l.kind == VH_F_INSET ? set_of[(size_t)n.leaf] : lit_of[(size_t)n.leaf]), (uint32_t)f.off, (uint32_t)f.bits);
      ++depth;
    } else {
      B.op[k] = vh_bits_op((uint32_t)n.kind, 0, 0, (uint32_t)n.count, 0, 0, 0);
      depth -= n.count - 1;
    }
    maxdepth = depth > maxdepth ? depth : maxdepth;
  }
  if (depth != 1 || maxdepth > VH_MAX_STACK) { printf("FAIL %s: the test's program has depth %d, ends at %d\n", what, maxdepth, depth); ++g_fail; return; }
  for (uint32_t w = 0; w < nwords; ++w) {
    const uint32_t got = vh_bits_eval(B, reinterpret_cast<const char*>(planes.data()), pitch, w * 4u);
    for (int i = 0; i < 32; ++i) {
      std::vector<uint64_t> vals;
      for (const Field& f : c.fields) {
        uint64_t v = 0;
        for (int b = 0; b < f.bits; ++b) v |= (uint64_t)((planes[(size_t)(f.off + b) * nwords + w] >> i) & 1u) << b;
        vals.push_back(v);
      }
      const bool want = row_eval(c, vals);
      ++g_rows;
      if ((bool)((got >> i) & 1u) != want) {
        if (g_fail < 20) printf("FAIL %s: word %u row %d (first field's value %llu) -> %d, per-row evaluation says %d\n", what, w, i, (unsigned long long)vals[0], (int)!want, (int)want);
        ++g_fail;
      }
    }
  }
}

static uint64_t lit_bits(int type, int64_t v) {      // the literal's low bytes, as db::AnyNum holds a value of the column's type
  const int bytes = 1 << (type & 3);
  uint64_t b = 0;
  memcpy(&b, &v, (size_t)bytes);
  return b;
}
static bool fits(int type, int nb) {      // a field of nb bits holds non-negative values of the type
  const int tb = 8 << (type & 3);
  return nb <= (type >= VH_I8 ? tb - 1 : tb);
}
static Case single(const Field& f, const Leaf& l, int flat) {
  Case c;
  c.fields = {Field{0, 3, VH_U8}, f};      // (a field in front: the leaf's planes do not begin at plane 0)
  c.leaves = {l};
  c.leaves[0].field = 1;
  c.prog = {Node{0, 0, 0}};
  c.flat = flat;
  return c;
}

int main() {
  std::mt19937_64 rng(20261019);
  char what[128];
  const int types[] = {VH_U32, VH_U64, VH_I32, VH_I64, VH_U16, VH_I8};
  // ---- every relation x field width x literal, single-leaf programs (as a flat program and through the stack)
  for (int nb : {1, 5, 10, 11, 31, 32})
    for (int type : types) {
      if (!fits(type, nb)) continue;
      std::vector<int64_t> lits = {0, 1, (int64_t)((1ull << nb) - 1), (int64_t)(1ull << nb), (int64_t)1 << 40, (int64_t)(rng() & ((1ull << nb) - 1))};
      if (type >= VH_I8) { lits.push_back(-1); lits.push_back(INT64_MIN); }
      for (int64_t lit : lits)
        for (int op = VH_OP_EQ; op <= VH_OP_GE; ++op)
          for (int flat : {1, 0}) {
            snprintf(what, sizeof(what), "rel op %d, %d bits, type %d, literal %lld, flat %d", op, nb, type, (long long)lit, flat);
            run_case(single(Field{3, nb, type}, Leaf{VH_F_REL, 0, op, {lit_bits(type, lit)}}, flat), rng, what);
          }
    }
  // ---- IN / NOT IN of 1, 2 and 8 values with duplicates
  for (int nb : {1, 5, 10, 11, 31, 32})
    for (int type : {VH_U32, VH_I64})
      for (int n : {1, 2, 8})
        for (int in : {1, 0}) {
          std::vector<uint64_t> l;
          for (int k = 0; k < n; ++k) l.push_back(lit_bits(type, (int64_t)(rng() % 6 == 0 ? (1ull << nb) + k : rng() & ((1ull << nb) - 1) & (nb > 4 ? 7u : ~0u))));
          if (n > 1) l[(size_t)n - 1] = l[0];                                   // a duplicate
          if (type == VH_I64 && n == 8) l[3] = lit_bits(type, -1);
          snprintf(what, sizeof(what), "%s of %d values, %d bits, type %d", in ? "IN" : "NOT IN", n, nb, type);
          run_case(single(Field{3, nb, type}, Leaf{VH_F_IN, 0, in, l}, 1), rng, what);
          run_case(single(Field{3, nb, type}, Leaf{VH_F_IN, 0, in, l}, 0), rng, what);
        }
  // ---- set leaves on 1-, 6- and 10-bit fields (and every width between, the widest truth table included)
  for (int nb = 1; nb <= VH_INSET_TRUTH_BITS; ++nb)
    for (int type : {VH_U32, VH_I32})
      for (int in : {1, 0})
        for (int dens : {1, 4, 64}) {
          std::vector<uint64_t> l;
          const int top = (1 << nb) - 1;
          for (int v = (type == VH_I32 ? -2 : 0); v <= top + 2; ++v) if ((int)(rng() % 64) < dens) l.push_back(lit_bits(type, v));
          if (l.empty()) l.push_back(lit_bits(type, top / 2));
          l.push_back(l[0]);
          snprintf(what, sizeof(what), "set leaf (%s), %d bits, type %d, %zu members", in ? "IN" : "NOT IN", nb, type, l.size());
          run_case(single(Field{3, nb, type}, Leaf{VH_F_INSET, 0, in, l}, 1), rng, what);
          run_case(single(Field{3, nb, type}, Leaf{VH_F_INSET, 0, in, l}, 0), rng, what);
        }
  // ---- programs over three fields (C3's: 2 + 10 + 10 bits): flat AND / OR, and nests up to the stack's depth
  const std::vector<Field> c3 = {Field{0, 2, VH_U32}, Field{2, 10, VH_U32}, Field{12, 10, VH_I32}};
  auto random_leaf = [&](int field) {
    const Field& f = c3[(size_t)field];
    const int kind = (int)(rng() % 4);
    if (kind == 0) { std::vector<uint64_t> l; for (int k = 0; k < 3; ++k) l.push_back(lit_bits(f.type, (int64_t)(rng() % (1u << f.bits)))); return Leaf{VH_F_IN, field, (int)(rng() & 1), l}; }
    if (kind == 1) { std::vector<uint64_t> l; for (int k = 0; k < 40; ++k) l.push_back(lit_bits(f.type, (int64_t)(rng() % (1u << f.bits)))); return Leaf{VH_F_INSET, field, (int)(rng() & 1), l}; }
    return Leaf{VH_F_REL, field, (int)(rng() % 6), {lit_bits(f.type, (int64_t)(rng() % (1u << f.bits)))}};
  };
  for (int round = 0; round < 200; ++round) {
    for (int flat : {1, 2}) {      // leaves + one AND (flat 1) / OR (flat 2) over all of them, also run through the stack
      Case c; c.fields = c3;
      const int n = 2 + (int)(rng() % 3);      // (the planner folds wider composites pairwise)
      int nsets = 0;
      for (int k = 0; k < n; ++k) { Leaf l = random_leaf(k % 3); if (l.kind == VH_F_INSET && ++nsets > VH_MAX_SETS) l = Leaf{VH_F_REL, k % 3, VH_OP_NE, {0}}; c.leaves.push_back(l); c.prog.push_back(Node{k, 0, 0}); }
      c.prog.push_back(Node{-1, flat == 1 ? VH_F_AND : VH_F_OR, n});
      c.flat = flat;
      snprintf(what, sizeof(what), "flat %s of %d leaves", flat == 1 ? "AND" : "OR", n);
      run_case(c, rng, what);
      c.flat = 0;
      run_case(c, rng, "a flat program through the stack");
    }
    {   // VH_MAX_STACK leaves pushed, then folded from the top by two- and three-operand nodes: the deepest stack the planner admits
      Case c; c.fields = c3;
      int depth = 0, nsets = 0;
      for (int k = 0; k < VH_MAX_STACK; ++k) { Leaf l = random_leaf(k % 3); if (l.kind == VH_F_INSET && ++nsets > VH_MAX_SETS) l = Leaf{VH_F_REL, k % 3, VH_OP_LT, {3}}; c.leaves.push_back(l); c.prog.push_back(Node{k, 0, 0}); ++depth; }
      while (depth > 1) { const int cnt = depth >= 3 && (rng() & 1) ? 3 : 2; c.prog.push_back(Node{-1, (rng() & 1) ? VH_F_AND : VH_F_OR, cnt}); depth -= cnt - 1; }
      run_case(c, rng, "a nest of VH_MAX_STACK operands");
    }
    {   // a random tree: (a OP b) OP2 (c OP3 d) ...
      Case c; c.fields = c3;
      int depth = 0, nleaf = 0, nsets = 0, nlits = 0;
      while ((int)c.prog.size() < VH_BITS_MAX_PROG - VH_MAX_STACK && nleaf < 10) {
        if (depth >= 2 && (depth >= VH_MAX_STACK || rng() % 3 == 0)) { const int cnt = depth >= 3 && (rng() & 1) ? 3 : 2; c.prog.push_back(Node{-1, (rng() & 1) ? VH_F_AND : VH_F_OR, cnt}); depth -= cnt - 1; continue; }
        Leaf l = random_leaf((int)(rng() % 3));
        if (l.kind == VH_F_INSET && ++nsets > VH_MAX_SETS) l = Leaf{VH_F_REL, l.field, VH_OP_GE, {2}};
        if (l.kind != VH_F_INSET) { if (nlits + (int)l.lits.size() > VH_BITS_MAX_LITS) break; nlits += (int)l.lits.size(); }
        c.leaves.push_back(l); c.prog.push_back(Node{nleaf++, 0, 0}); ++depth;
      }
      while (depth > 1) { const int cnt = depth >= 3 ? 3 : 2; c.prog.push_back(Node{-1, (rng() & 1) ? VH_F_AND : VH_F_OR, cnt}); depth -= cnt - 1; }
      run_case(c, rng, "a random tree");
    }
  }
  printf("%s: %ld rows over %ld programs, %d wrong\n", g_fail ? "FAILED" : "ok", g_rows, g_progs, g_fail);
  return g_fail ? 1 : 0;
}
