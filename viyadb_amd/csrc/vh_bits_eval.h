// vh_bits_eval.h — a filter program evaluated BIT-SERIALLY on the bit-sliced predicate planes (VhPredPack::sliced), 32 rows per call.
// Plain C++ for host and device, like vh_inset.h: the select kernels include it (vh_small_kernels.h: select_count_sliced_kernel,
// select_emit_sliced_kernel) and so does the pre-built aggregate scan (vh_scan_sliced.hip), the planner fills its program (vhh_plan.h), and a host-compiled check holds it against a per-row evaluation
// of the same program (tests/bits_eval_host.cc).
//
// The per-query compiled scan reads the planes through code generated for the plan's shape (vh_jit_body.h: vj_bits_rel<NB, OP>,
// vj_bits_inset<NB>). This is the same arithmetic as an INTERPRETER: field widths, relations and the tree are run-time data. That costs
// little here, because the dispatch is paid once per 32 rows and plane, not once per row: a comparison with a literal is a walk over the
// field's planes from the top bit down, a few bitwise operations per plane; every branch is on the program or on a literal, so it is
// uniform over a wave. Nothing is compiled at run time.
//
// Layout of the planes, as predslice_kernel (vh_small_kernels.h) writes it: a segment's planes begin at plane[0].ptr + seg * plane[0].stride;
// plane b lies b * pitch bytes further on; rows 32w .. 32w + 31 are u32 word w of a plane, row 32w + i being bit i. A field of a column is
// `bits` consecutive planes from plane `off` on, the least significant first, and holds the column's non-negative value as it is.
//
// Semantics of a leaf (those of vj_bits_lt_eq / vj_bits_eq): the literal is decoded to the column's element type (its low bytes, as
// db::AnyNum carries it); a negative literal of a signed type equals no value and has no value below it; a literal beyond the field's range
// equals no value and has every value below it. IN is the OR of `==`, NOT IN the AND of `!=`. A set leaf (VH_F_INSET) reads the truth
// table the planner built over its field (vh_inset.h: vh_inset_bits<NB>, NB <= VH_INSET_TRUTH_BITS).
#pragma once
#include <stdint.h>
#ifdef __HIPCC_RTC__
#include "viya_hip.h"      // (a compiled kernel's frame: the headers are handed to hipRTC by name, vh_jit.hip)
#else
#include "../../include/viya_hip.h"
#endif
#include "vh_inset.h"

#if defined(__HIPCC__)
#define VH_BITS_FN __host__ __device__ __forceinline__
#else
#define VH_BITS_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// (the column-stream load of the compiled scan's preload: non-temporal, off a device allocation — global_load, not flat_load)
#define VH_BITS_LOAD(p) __builtin_nontemporal_load((const uint32_t __attribute__((address_space(1)))*)(p))
#define VH_BITS_UNIFORM(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#define VH_BITS_UNROLL _Pragma("unroll")
#else
#define VH_BITS_LOAD(p) (*(const uint32_t*)(p))
#define VH_BITS_UNIFORM(v) ((uint32_t)(v))
#define VH_BITS_UNROLL
#endif

#ifndef VH_MAX_STACK
#define VH_MAX_STACK 8           // operand stack of the program (= vh_internal.h)
#endif
#define VH_BITS_MAX_PROG 24      // = VH_INLINE_PROG, VH_INLINE_LITS (vh_internal.h; vh_sliced.h asserts both): the program travels in the
#define VH_BITS_MAX_LITS 32      //   kernel arguments
#define VH_BITS_MAX_FIELD 32     // planes of one field: a row word of the projection has 32 bits

// One node of the postfix program: 8 bytes, words only (see VH_PACKED_FIELD in vh_internal.h on sub-dword members of kernel arguments).
//   w0: kind (enum vh_fkind) | element type of the column << 8 | relation / IN polarity << 16 | count << 24 (IN: literals; AND / OR: operands)
//   w1: first literal, or the set's index for VH_F_INSET | first plane of the leaf's field << 16 | planes of the field << 24
struct VhBitsOp { uint32_t w0, w1; };
VH_BITS_FN VhBitsOp vh_bits_op(uint32_t kind, uint32_t type, uint32_t op, uint32_t count, uint32_t lit, uint32_t off, uint32_t bits) {
  VhBitsOp o;
  o.w0 = (kind & 0xFFu) | (type & 0xFFu) << 8 | (op & 0xFFu) << 16 | (count & 0xFFu) << 24;
  o.w1 = (lit & 0xFFFFu) | (off & 0xFFu) << 16 | (bits & 0xFFu) << 24;
  return o;
}
VH_BITS_FN uint32_t vh_bits_kind(VhBitsOp o) { return o.w0 & 0xFFu; }
VH_BITS_FN uint32_t vh_bits_type(VhBitsOp o) { return (o.w0 >> 8) & 0xFFu; }
VH_BITS_FN uint32_t vh_bits_relop(VhBitsOp o) { return (o.w0 >> 16) & 0xFFu; }
VH_BITS_FN uint32_t vh_bits_count(VhBitsOp o) { return o.w0 >> 24; }
VH_BITS_FN uint32_t vh_bits_lit(VhBitsOp o) { return o.w1 & 0xFFFFu; }
VH_BITS_FN uint32_t vh_bits_off(VhBitsOp o) { return (o.w1 >> 16) & 0xFFu; }
VH_BITS_FN uint32_t vh_bits_width(VhBitsOp o) { return o.w1 >> 24; }

struct VhBitsProg {
  int32_t nprog;
  int32_t flat;                  // VhPlanDev::prog_flat: 1 = leaves and one AND over all of them (or a single leaf), 2 = ... one OR, 0 = anything else (the stack)
  VhBitsOp op[VH_BITS_MAX_PROG];
  uint64_t lits[VH_BITS_MAX_LITS];
  const VhSetDev* set;           // the plan's set descriptors (VhPlanDev::set); a set leaf reads `truth` alone
};

// the literal as a value of element type `type` (integer types only: nothing else has a field): its value as 64 bits, and whether it is negative
VH_BITS_FN uint64_t vh_bits_literal(uint32_t type, uint64_t bits, bool* neg) {
  int64_t s;
  switch (type) {
    case VH_U8: *neg = false; return (uint8_t)bits;
    case VH_U16: *neg = false; return (uint16_t)bits;
    case VH_U32: *neg = false; return (uint32_t)bits;
    case VH_I8: s = (int8_t)bits; break;
    case VH_I16: s = (int16_t)bits; break;
    case VH_I32: s = (int32_t)bits; break;
    case VH_I64: s = (int64_t)bits; break;
    default: *neg = false; return bits;
  }
  *neg = s < 0;
  return (uint64_t)s;
}

// x[b]: plane b of the field for the lane's 32 rows (0 for b >= nb). -> the rows whose value is below c / equals c.
VH_BITS_FN void vh_bits_lt_eq(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint64_t c, bool neg, uint32_t* lt_out, uint32_t* eq_out) {
  if (neg) { *lt_out = 0u; *eq_out = 0u; return; }                   // a negative literal: no (non-negative) value is below it or equals it
  if ((c >> nb) != 0ull) { *lt_out = ~0u; *eq_out = 0u; return; }    // beyond the field's range: every value is below it (nb <= 32: a defined shift)
  const uint32_t cs = VH_BITS_UNIFORM((uint32_t)c);
  uint32_t lt = 0u, eq = ~0u;
  VH_BITS_UNROLL
  for (int b = VH_BITS_MAX_FIELD - 1; b >= 0; --b) {
    if ((uint32_t)b >= nb) continue;
    const uint32_t xb = x[b];
    if ((cs >> b) & 1u) { lt |= eq & ~xb; eq &= xb; } else { eq &= ~xb; }
  }
  *lt_out = lt; *eq_out = eq;
}
VH_BITS_FN uint32_t vh_bits_eq(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint64_t c, bool neg) {
  if (neg || (c >> nb) != 0ull) return 0u;
  const uint32_t cs = VH_BITS_UNIFORM((uint32_t)c);
  uint32_t eq = ~0u;
  VH_BITS_UNROLL
  for (int b = VH_BITS_MAX_FIELD - 1; b >= 0; --b) {
    if ((uint32_t)b >= nb) continue;
    eq &= ((cs >> b) & 1u) ? x[b] : ~x[b];
  }
  return eq;
}
// op: enum vh_relop. The mask of the lane's 32 rows for which (column op c) holds.
VH_BITS_FN uint32_t vh_bits_rel(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, uint32_t op, uint64_t c, bool neg) {
  if (op == VH_OP_EQ) return vh_bits_eq(x, nb, c, neg);
  if (op == VH_OP_NE) return ~vh_bits_eq(x, nb, c, neg);
  uint32_t lt, eq;
  vh_bits_lt_eq(x, nb, c, neg, &lt, &eq);
  return op == VH_OP_LT ? lt : op == VH_OP_LE ? (lt | eq) : op == VH_OP_GT ? ~(lt | eq) : ~lt;
}
// a set leaf: the rows whose value is a member, from the truth table over the field's nb <= VH_INSET_TRUTH_BITS planes
VH_BITS_FN uint32_t vh_bits_inset(const uint32_t (&x)[VH_BITS_MAX_FIELD], uint32_t nb, const uint32_t* truth) {
  static_assert(VH_INSET_TRUTH_BITS == 10, "one case per field width");
  switch (nb) {
    case 1: return vh_inset_bits<1>(x, truth);
    case 2: return vh_inset_bits<2>(x, truth);
    case 3: return vh_inset_bits<3>(x, truth);
    case 4: return vh_inset_bits<4>(x, truth);
    case 5: return vh_inset_bits<5>(x, truth);
    case 6: return vh_inset_bits<6>(x, truth);
    case 7: return vh_inset_bits<7>(x, truth);
    case 8: return vh_inset_bits<8>(x, truth);
    case 9: return vh_inset_bits<9>(x, truth);
    case 10: return vh_inset_bits<10>(x, truth);
    default: return 0u;        // (the planner gives a set leaf no wider field)
  }
}

// One leaf for the 32 rows of the plane word at byte `woff` of every plane. All of the field's plane loads are issued before the first is
// consumed.
VH_BITS_FN uint32_t vh_bits_leaf(const VhBitsProg& B, VhBitsOp o, const char* planes, uint64_t pitch, uint32_t woff) {
  const uint32_t nb = vh_bits_width(o), kind = vh_bits_kind(o), type = vh_bits_type(o);
  const char* field = planes + (uint64_t)vh_bits_off(o) * pitch;
  uint32_t x[VH_BITS_MAX_FIELD];
  VH_BITS_UNROLL
  for (int b = 0; b < VH_BITS_MAX_FIELD; ++b) {
    x[b] = 0u;
    if ((uint32_t)b < nb) x[b] = VH_BITS_LOAD(field + (uint64_t)b * pitch + woff);
  }
  bool neg;
  if (kind == VH_F_REL) {
    const uint64_t c = vh_bits_literal(type, B.lits[vh_bits_lit(o)], &neg);
    return vh_bits_rel(x, nb, vh_bits_relop(o), c, neg);
  }
  if (kind == VH_F_INSET) {
    const uint32_t m = vh_bits_inset(x, nb, B.set[vh_bits_lit(o)].truth);
    return vh_bits_relop(o) ? m : ~m;
  }
  // IN: OR of ==, NOT IN: AND of != (filter.cc:223-241)
  const uint32_t in = vh_bits_relop(o), n = vh_bits_count(o);
  uint32_t m = in ? 0u : ~0u;
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t c = vh_bits_literal(type, B.lits[vh_bits_lit(o) + k], &neg);
    const uint32_t e = vh_bits_eq(x, nb, c, neg);
    m = in ? (m | e) : (m & ~e);
  }
  return m;
}

// The program for one word position: `planes` = the segment's first plane, `woff` = 4 * the word's index. -> bit i: row 32w + i passes.
// Bits of rows beyond the segment's rows are whatever the planes hold there: the caller masks them.
VH_BITS_FN uint32_t vh_bits_eval(const VhBitsProg& B, const char* planes, uint64_t pitch, uint32_t woff) {
  if (B.flat) {      // leaves + one AND / OR over all of them, or a single leaf: no stack
    uint32_t acc = B.flat == 1 ? ~0u : 0u;
    for (int pc = 0; pc < B.nprog; ++pc) {
      const VhBitsOp o = B.op[pc];
      const uint32_t kind = vh_bits_kind(o);
      if (kind == VH_F_AND || kind == VH_F_OR) continue;
      const uint32_t m = kind == VH_F_TRUE ? ~0u : vh_bits_leaf(B, o, planes, pitch, woff);
      acc = B.flat == 1 ? (acc & m) : (acc | m);
    }
    return acc;
  }
  uint32_t st[VH_MAX_STACK];
  int sp = 0;
  for (int pc = 0; pc < B.nprog; ++pc) {
    const VhBitsOp o = B.op[pc];
    const uint32_t kind = vh_bits_kind(o);
    if (kind == VH_F_AND || kind == VH_F_OR) {
      uint32_t a = st[--sp];
      for (uint32_t i = 1; i < vh_bits_count(o); ++i) { const uint32_t b = st[--sp]; a = kind == VH_F_AND ? (a & b) : (a | b); }
      st[sp++] = a;
    } else {
      st[sp++] = kind == VH_F_TRUE ? ~0u : vh_bits_leaf(B, o, planes, pitch, woff);
    }
  }
  return st[0];
}
