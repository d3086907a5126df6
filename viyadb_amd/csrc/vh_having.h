// vh_having.h — the comparison and the postfix evaluation of a pushed-down HAVING, in one place. Plain C++ for host and device, like
// vh_topk_key.h: the emission kernels include it (vh_small_kernels.h: vh_emit_have, shared by emit_groups_kernel<2>, <16> and
// small_tail_kernel), and a host-compiled check holds it against the typed C++ comparisons (tests/having_host.cc).
//
// The reference evaluates HAVING on the aggregated tuples, one group at a time, with ComparisonBuilder semantics
// (src/codegen/query/post_agg.cc:77-83). Here a group's value of result column c arrives as the 64 bits of its key or of its raw metric
// state, and the comparison happens in the element type the planner chose for the node:
//   - both sides are decoded from their LOW bytes, as db::AnyNum carries a literal. A 64-bit raw state compared in a narrower type is
//     truncated — that is the contract: a `byte` sum that wrapped compares as the wrapped byte;
//   - floats compare as IEEE values: -0.0 equals +0.0, and a NaN on either side is unordered — `ne` holds, every other relation fails;
//   - IN is the OR of `==` over its literals (none: false), NOT IN the AND of `!=` (none: true);
//   - AND / OR fold their `count` operands bitwise, like the scan filter; the program leaves exactly one value (the planner checks it).
#pragma once
#include <stdint.h>
#include "../../include/viya_hip.h"

#if defined(__HIPCC__)
#define VH_HAVING_FN __host__ __device__ __forceinline__
#else
#define VH_HAVING_FN static inline
#endif
#ifndef VH_MAX_STACK
#define VH_MAX_STACK 8           // operand stack of the program (= vh_internal.h)
#endif

template <typename T> VH_HAVING_FN T vh_having_lit(uint64_t bits) {
  T v; __builtin_memcpy(&v, &bits, sizeof(T)); return v;   // low bytes, like db::AnyNum
}

VH_HAVING_FN bool vh_cmp_bits(int type, uint64_t a, uint64_t b, int op) {
  int r;  // -1 / 0 / +1 / 2 (unordered)
#define VH_C(T) { const T x = vh_having_lit<T>(a), y = vh_having_lit<T>(b); r = x < y ? -1 : (x > y ? 1 : (x == y ? 0 : 2)); }
  switch (type) {
    case VH_U8: VH_C(uint8_t) break;   case VH_U16: VH_C(uint16_t) break;
    case VH_U32: VH_C(uint32_t) break; case VH_U64: VH_C(uint64_t) break;
    case VH_I8: VH_C(int8_t) break;    case VH_I16: VH_C(int16_t) break;
    case VH_I32: VH_C(int32_t) break;  case VH_I64: VH_C(int64_t) break;
    case VH_F32: VH_C(float) break;    default: VH_C(double) break;
  }
#undef VH_C
  switch (op) {
    case VH_OP_EQ: return r == 0;
    case VH_OP_NE: return r != 0;
    case VH_OP_LT: return r == -1;
    case VH_OP_LE: return r == -1 || r == 0;
    case VH_OP_GT: return r == 1;
    default: return r == 1 || r == 0;
  }
}

// The program over one group. Op: a node with kind(), op(), count(), slot() and lit() (VhProgOp, vh_internal.h); type[pc]: the element type
// node pc compares in; value_of(c): the 64 bits of the group's result column c. Postfix, bitwise & / | like the filter.
template <class Op, class Type, class ValueOf>
VH_HAVING_FN bool vh_having_eval(const Op* prog, int nprog, const Type* type, const uint64_t* lits, ValueOf value_of) {
  bool st[VH_MAX_STACK];
  int sp = 0;
  for (int pc = 0; pc < nprog; ++pc) {
    const Op o = prog[pc];
    if (o.kind() == VH_F_TRUE) st[sp++] = true;
    else if (o.kind() == VH_F_AND || o.kind() == VH_F_OR) {
      bool a = st[--sp];
      for (int k = 1; k < (int)o.count(); ++k) { const bool b = st[--sp]; a = o.kind() == VH_F_AND ? (a & b) : (a | b); }
      st[sp++] = a;
    } else {
      const uint64_t v = value_of((int)o.slot());
      bool r;
      if (o.kind() == VH_F_REL) r = vh_cmp_bits((int)type[pc], v, lits[o.lit()], (int)o.op());
      else {
        r = !o.op();
        for (int k = 0; k < (int)o.count(); ++k) {
          const bool e = vh_cmp_bits((int)type[pc], v, lits[o.lit() + k], o.op() ? VH_OP_EQ : VH_OP_NE);
          r = o.op() ? (r | e) : (r & e);
        }
      }
      st[sp++] = r;
    }
  }
  return st[0];
}
