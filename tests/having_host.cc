// The HAVING comparison and its postfix evaluation (viyadb_amd/csrc/vh_having.h) on the CPU, against the typed C++ comparisons.
// Stand-alone: g++ -I viyadb_amd/csrc tests/having_host.cc. Prints one "<check>: ok" line per check; exit status 1 on the first mismatch.
//
//   pairs       every element type x every relation x every ordered pair of the type's edge values (the values of tests/extremes.py, written
//               out below; floats with NaN added: -0.0 against +0.0 is equal, NaN against everything is unordered — `ne` holds, the rest fail)
//   truncation  a 64-bit raw state whose upper bits are set, compared in a narrower type: the low bytes decide (a `byte` sum that wrapped)
//   in          IN and NOT IN with 0, 1 and 24 literals
//   andor       AND and OR of 1, 2 and 8 operands
//   program     16 nodes at stack depth 8, against an independent evaluation of the same tree
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <vector>

#include "vh_having.h"

// a node as vh_having_eval reads it: the accessors of VhProgOp (vh_internal.h)
struct Op {
  uint32_t k, o, c, s, l;
  uint32_t kind() const { return k; }
  uint32_t op() const { return o; }
  uint32_t count() const { return c; }
  uint32_t slot() const { return s; }
  uint32_t lit() const { return l; }
};
static Op leaf(uint32_t kind, uint32_t op, uint32_t count, uint32_t slot, uint32_t lit) { return Op{kind, op, count, slot, lit}; }
static Op node(uint32_t kind, uint32_t count) { return Op{kind, 0, count, 0, 0}; }

static int fail(const char* what, const char* detail) { printf("%s: MISMATCH %s\n", what, detail); return 1; }

template <typename T> static uint64_t bits_of(T v) { uint64_t b = 0; memcpy(&b, &v, sizeof(T)); return b; }
template <typename T> static bool typed(T a, T b, int op) {
  switch (op) {
    case VH_OP_EQ: return a == b;
    case VH_OP_NE: return a != b;
    case VH_OP_LT: return a < b;
    case VH_OP_LE: return a <= b;
    case VH_OP_GT: return a > b;
    default: return a >= b;
  }
}

// tests/extremes.py, int_edges: min, min + 1, -1, 0, 1, 2^k - 1 and 2^k for k in {7, 8, 15, 16, 31, 32, 62, 63} clipped to the type, max - 1, max
struct IntEdge { bool neg; uint64_t mag; };
static const IntEdge kIntEdges[] = {
    {true, 1ull}, {false, 0ull}, {false, 1ull},
    {false, 127ull}, {false, 128ull}, {false, 255ull}, {false, 256ull},
    {false, 32767ull}, {false, 32768ull}, {false, 65535ull}, {false, 65536ull},
    {false, 2147483647ull}, {false, 2147483648ull}, {false, 4294967295ull}, {false, 4294967296ull},
    {false, 4611686018427387903ull}, {false, 4611686018427387904ull}, {false, 9223372036854775807ull}, {false, 9223372036854775808ull},
};
template <typename T> static std::vector<T> int_edges() {
  typedef std::numeric_limits<T> L;
  std::vector<T> out = {L::min(), (T)(L::min() + 1), (T)(L::max() - 1), L::max()};
  for (const IntEdge& e : kIntEdges) {
    if (e.neg) { if (L::is_signed) out.push_back((T)-1); continue; }
    if (e.mag <= (uint64_t)L::max()) out.push_back((T)e.mag);
  }
  return out;
}
// tests/extremes.py, float_edges: +-0.0, 1 and 1 +- 1 ulp, +-inf, +-smallest and +-largest subnormal, +-FLT_MIN / DBL_MIN, +-FLT_MAX / DBL_MAX,
// 0.1 * k for k in {-7, -3, 1, 3, 9}; and NaN, which the tables leave out and a float SUM can still produce (opposite infinities)
template <typename T> static std::vector<T> float_edges() {
  typedef std::numeric_limits<T> L;
  const T one = 1, sub_min = L::denorm_min(), sub_max = std::nextafter(L::min(), (T)0);
  std::vector<T> out = {(T)0.0, (T)-0.0, std::nextafter(one, (T)0), one, std::nextafter(one, (T)2), L::infinity(), -L::infinity(),
                        sub_min, -sub_min, sub_max, -sub_max, L::min(), -L::min(), L::max(), -L::max(),
                        (T)(0.1 * -7), (T)(0.1 * -3), (T)(0.1 * 1), (T)(0.1 * 3), (T)(0.1 * 9), L::quiet_NaN(), -L::quiet_NaN()};
  return out;
}

static const uint64_t kUpper = 0xA5C3F00DDEADBEEFull;      // what a wider raw state may hold above the compared type's bytes

template <typename T> static int check_type(int type, const char* name, const std::vector<T>& e, long* pairs) {
  char what[64], detail[160];
  for (int op = VH_OP_EQ; op <= VH_OP_GE; ++op)
    for (T a : e)
      for (T b : e) {
        const bool want = typed<T>(a, b, op);
        const uint64_t ba = bits_of(a), bb = bits_of(b);
        bool got = vh_cmp_bits(type, ba, bb, op);
        if (got != want) {
          snprintf(what, sizeof(what), "pairs %s", name);
          snprintf(detail, sizeof(detail), "op %d a %016llx b %016llx: got %d want %d", op, (unsigned long long)ba, (unsigned long long)bb, got, want);
          return fail(what, detail);
        }
        if (sizeof(T) < 8) {      // truncation is the contract: the bytes above the type's own do not take part, on either side
          const uint64_t up = kUpper << (8 * sizeof(T)), up2 = ~kUpper << (8 * sizeof(T));
          got = vh_cmp_bits(type, ba | up, bb | up2, op);
          if (got != want) {
            snprintf(what, sizeof(what), "truncation %s", name);
            snprintf(detail, sizeof(detail), "op %d a %016llx b %016llx: got %d want %d", op, (unsigned long long)(ba | up), (unsigned long long)(bb | up2), got, want);
            return fail(what, detail);
          }
        }
        ++*pairs;
      }
  printf("pairs %s (%zu values): ok\n", name, e.size());
  return 0;
}

// an independent evaluation of a postfix program: a vector as the stack, the typed comparison at the leaves
static bool plain_eval(const std::vector<Op>& prog, const std::vector<uint32_t>& type, const std::vector<uint64_t>& lits, const std::vector<uint64_t>& col) {
  std::vector<bool> st;
  for (size_t pc = 0; pc < prog.size(); ++pc) {
    const Op& o = prog[pc];
    if (o.k == VH_F_TRUE) st.push_back(true);
    else if (o.k == VH_F_AND || o.k == VH_F_OR) {
      bool a = o.k == VH_F_AND;
      for (uint32_t k = 0; k < o.c; ++k) { const bool b = st.back(); st.pop_back(); a = o.k == VH_F_AND ? (a && b) : (a || b); }
      st.push_back(a);
    } else {
      const int64_t v = (int64_t)col[o.s];      // (the programs below compare in VH_I64)
      (void)type;
      bool r;
      if (o.k == VH_F_REL) r = typed<int64_t>(v, (int64_t)lits[o.l], (int)o.o);
      else {
        bool any = false;
        for (uint32_t k = 0; k < o.c; ++k) any = any || v == (int64_t)lits[o.l + k];
        r = o.o ? any : !any;
      }
      st.push_back(r);
    }
  }
  return st.size() == 1 && st[0];
}
static bool run(const std::vector<Op>& prog, const std::vector<uint32_t>& type, const std::vector<uint64_t>& lits, const std::vector<uint64_t>& col) {
  return vh_having_eval(prog.data(), (int)prog.size(), type.data(), lits.data(), [&](int c) { return col[(size_t)c]; });
}

int main() {
  long pairs = 0;
  if (check_type<uint8_t>(VH_U8, "u8", int_edges<uint8_t>(), &pairs)) return 1;
  if (check_type<uint16_t>(VH_U16, "u16", int_edges<uint16_t>(), &pairs)) return 1;
  if (check_type<uint32_t>(VH_U32, "u32", int_edges<uint32_t>(), &pairs)) return 1;
  if (check_type<uint64_t>(VH_U64, "u64", int_edges<uint64_t>(), &pairs)) return 1;
  if (check_type<int8_t>(VH_I8, "i8", int_edges<int8_t>(), &pairs)) return 1;
  if (check_type<int16_t>(VH_I16, "i16", int_edges<int16_t>(), &pairs)) return 1;
  if (check_type<int32_t>(VH_I32, "i32", int_edges<int32_t>(), &pairs)) return 1;
  if (check_type<int64_t>(VH_I64, "i64", int_edges<int64_t>(), &pairs)) return 1;
  if (check_type<float>(VH_F32, "f32", float_edges<float>(), &pairs)) return 1;
  if (check_type<double>(VH_F64, "f64", float_edges<double>(), &pairs)) return 1;

  // the literal cases of the contract, spelled out: NaN, the zeros, a byte sum that wrapped
  {
    const uint64_t nan32 = bits_of(std::numeric_limits<float>::quiet_NaN()), one32 = bits_of(1.0f);
    const uint64_t nan64 = bits_of(std::numeric_limits<double>::quiet_NaN()), one64 = bits_of(1.0);
    for (int op = VH_OP_EQ; op <= VH_OP_GE; ++op) {
      const bool want = op == VH_OP_NE;
      if (vh_cmp_bits(VH_F32, nan32, one32, op) != want || vh_cmp_bits(VH_F32, one32, nan32, op) != want || vh_cmp_bits(VH_F32, nan32, nan32, op) != want ||
          vh_cmp_bits(VH_F64, nan64, one64, op) != want || vh_cmp_bits(VH_F64, one64, nan64, op) != want || vh_cmp_bits(VH_F64, nan64, nan64, op) != want)
        return fail("nan", "a NaN operand: ne holds, every other relation fails");
    }
    if (!vh_cmp_bits(VH_F32, bits_of(-0.0f), bits_of(0.0f), VH_OP_EQ) || !vh_cmp_bits(VH_F64, bits_of(0.0), bits_of(-0.0), VH_OP_EQ) ||
        vh_cmp_bits(VH_F64, bits_of(-0.0), bits_of(0.0), VH_OP_LT) || !vh_cmp_bits(VH_F32, bits_of(-0.0f), bits_of(0.0f), VH_OP_GE))
      return fail("zeros", "-0.0 and +0.0 compare equal");
    const int64_t wrapped = 127 + 127 + 46;      // 300: a byte SUM's raw state; the byte it wrapped to is 44
    if (!vh_cmp_bits(VH_I8, (uint64_t)wrapped, bits_of((int8_t)44), VH_OP_EQ) || vh_cmp_bits(VH_I8, (uint64_t)wrapped, bits_of((int8_t)127), VH_OP_GT) ||
        !vh_cmp_bits(VH_I8, (uint64_t)(int64_t)-129, bits_of((int8_t)127), VH_OP_EQ) || !vh_cmp_bits(VH_U8, 256ull + 7ull, 7ull, VH_OP_EQ) ||
        !vh_cmp_bits(VH_U16, 0xFFFFFFFFFFFF0000ull, 0ull, VH_OP_EQ) || !vh_cmp_bits(VH_I32, 0x0000000180000000ull, bits_of((int32_t)-2147483647 - 1), VH_OP_EQ))
      return fail("truncation", "the low bytes decide");
    printf("nan, zeros, truncation (%ld pairs above): ok\n", pairs);
  }

  // IN / NOT IN with 0, 1 and 24 literals
  for (uint32_t n : {0u, 1u, 24u}) {
    std::vector<uint64_t> lits;
    for (uint32_t k = 0; k < n; ++k) lits.push_back((uint64_t)(int64_t)(3 * (int64_t)k - 30));      // -30, -27, ... 39
    for (int64_t v = -33; v <= 42; ++v) {
      bool member = false;
      for (uint64_t l : lits) member |= (int64_t)l == v;
      const std::vector<uint64_t> col = {(uint64_t)v};
      const std::vector<uint32_t> type = {VH_I64};
      if (run({leaf(VH_F_IN, 1, n, 0, 0)}, type, lits, col) != member) return fail("in", "IN is the OR of == (none: false)");
      if (run({leaf(VH_F_IN, 0, n, 0, 0)}, type, lits, col) != !member) return fail("in", "NOT IN is the AND of != (none: true)");
    }
    printf("in, not in with %u literals: ok\n", n);
  }

  // AND / OR of 1, 2 and 8 operands: every combination of operand values (leaves `col[k] == 1`)
  for (uint32_t n : {1u, 2u, 8u}) {
    for (uint32_t m = 0; m < (1u << n); ++m) {
      std::vector<Op> pa, po;
      std::vector<uint32_t> type;
      std::vector<uint64_t> col;
      for (uint32_t k = 0; k < n; ++k) {
        pa.push_back(leaf(VH_F_REL, VH_OP_EQ, 1, k, 0)); po.push_back(pa.back());
        type.push_back(VH_I64); col.push_back((m >> k) & 1u);
      }
      pa.push_back(node(VH_F_AND, n)); po.push_back(node(VH_F_OR, n)); type.push_back(0);
      const std::vector<uint64_t> lits = {1};
      if (run(pa, type, lits, col) != (m == (1u << n) - 1u)) return fail("andor", "AND");
      if (run(po, type, lits, col) != (m != 0)) return fail("andor", "OR");
    }
    printf("and, or of %u: ok\n", n);
  }

  // 16 nodes at stack depth 8: eight leaves (depth 8), AND of 3 (6), a TRUE and an IN (8), four ANDs / ORs of 2 (4), an OR of 4 (1)
  {
    std::vector<Op> prog;
    for (uint32_t k = 0; k < 8; ++k) prog.push_back(leaf(VH_F_REL, k % 6, 1, k, k));
    prog.push_back(node(VH_F_AND, 3));
    prog.push_back(node(VH_F_TRUE, 0));
    prog.push_back(leaf(VH_F_IN, 1, 3, 8, 8));
    prog.push_back(node(VH_F_AND, 2));
    prog.push_back(node(VH_F_OR, 2));
    prog.push_back(node(VH_F_AND, 2));
    prog.push_back(node(VH_F_AND, 2));
    prog.push_back(node(VH_F_OR, 4));
    if (prog.size() != 16) return fail("program", "16 nodes");
    int depth = 0, deepest = 0;
    for (const Op& o : prog) { depth += o.k == VH_F_AND || o.k == VH_F_OR ? 1 - (int)o.c : 1; if (depth > deepest) deepest = depth; }
    if (depth != 1 || deepest != 8) return fail("program", "one value left, depth 8");
    const std::vector<uint32_t> type(16, VH_I64);
    const std::vector<uint64_t> lits = {0, 1, 2, 3, 4, 5, 6, 7, 2, 5, (uint64_t)(int64_t)-1};
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    int kept = 0;
    for (int trial = 0; trial < 20000; ++trial) {
      std::vector<uint64_t> col(9);
      for (uint64_t& c : col) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; c = (uint64_t)((int64_t)((seed >> 33) % 10) - 1); }
      const bool want = plain_eval(prog, type, lits, col), got = run(prog, type, lits, col);
      if (got != want) return fail("program", "16 nodes at depth 8");
      kept += got;
    }
    if (kept == 0 || kept == 20000) return fail("program", "the trials decide nothing");
    printf("program of 16 nodes at depth 8 (%d of 20000 kept): ok\n", kept);
  }
  return 0;
}
