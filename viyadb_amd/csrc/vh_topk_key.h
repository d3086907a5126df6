// vh_topk_key.h — the sort key and the slack of the device top-N, in one place. Plain C++: the kernels
// include it (vh_small_kernels.h), the host takes the slack from it (vhh_finalize.h), and a host-compiled check holds
// it against the reference's comparators (tests/test_topk_key.py).
//
// `sort` + `limit` on a numeric column: instead of shipping every group to the host to be formatted and string-
// sorted (src/codegen/query/post_agg.cc:50-147, sort.cc:24-75 — what dominates at ~10 M groups), the device keeps
// a SUPERSET of the rows the reference would return: every group whose primary sort key is at least the K-th
// best (K = skip + limit), ties and a rounding slack included. The host then runs the reference's exact string
// comparators on those few rows. Keys only have to be MONOTONE in the reference's order, not exact:
//   INTEGER columns compare as strings by (length, lexicographic) (src/util/string.h:28-49): ascending order is
//     0..9, -1..-9, 10..99, -10..-99, ...  ->  key = class(digits, sign) : |v|. Equal keys may hide different
//     values (the 18..20-digit classes), never the other way round: no slack.
//   FLOAT columns compare stod() of their "%.15g" (double) / "%g" (float) text: numeric order, except that
//     neighbouring values print the same text and then TIE. The key is the IEEE bit pattern in numeric order (one
//     key unit = one ulp; -0 takes +0's key), and the slack is how many ulps apart two values of one text can be:
//       "%.15g" keeps 15 significant digits: the doubles of one text span less than one unit of the 15th digit,
//         which just above a power of ten x, in the binade whose ulp is at least x / 2^53, is
//         (x / 10^14) / (x / 2^53) = 2 * 2^52 / 10^14 = 90.07 ulps            -> measured widest run: 87 ulps apart
//       "%g" keeps 6: 2 * 2^23 / 10^5 = 167.8 ulps                             -> measured widest run: 163 ulps apart
//     (tests/test_topk_key.py walks the runs and asserts both widths stay below the slack.)
#pragma once
#include <stdint.h>
#ifndef VH_TOPK_FN
#ifdef __HIPCC__
#define VH_TOPK_FN __host__ __device__ __forceinline__
#else
#define VH_TOPK_FN static inline
#endif
#endif
// enum vh_elem (include/viya_hip.h), restated so that this file stands alone
#define VHK_U8 0
#define VHK_U16 1
#define VHK_U32 2
#define VHK_U64 3
#define VHK_I8 4
#define VHK_I16 5
#define VHK_I32 6
#define VHK_I64 7
#define VHK_F32 8
#define VHK_F64 9

enum { VH_TOPK_INT = 0, VH_TOPK_FLOAT = 1 };

// Slack in ulps: each bound above rounded up to the next power of two (a kept row too many costs one host
// comparison; a dropped one is a wrong answer).
#define VH_TOPK_SLACK_F64_ULPS 128ull      // 2 * 2^52 / 10^14 = 90.07, rounded up
#define VH_TOPK_SLACK_F32_ULPS 256ull      // 2 * 2^23 / 10^5 = 167.8, rounded up

// in key units: a float's 32 bits sit in the key's upper half
VH_TOPK_FN uint64_t vh_topk_slack(int cls, int elem) {
  if (cls != VH_TOPK_FLOAT) return 0ull;
  return elem == VHK_F32 ? VH_TOPK_SLACK_F32_ULPS << 32 : VH_TOPK_SLACK_F64_ULPS;
}

VH_TOPK_FN uint64_t vh_topk_key(int cls, int elem, uint64_t bits) {
  if (cls == VH_TOPK_FLOAT) {
    if (elem == VHK_F32) {
      uint32_t b = (uint32_t)bits;
      if (b == 0x80000000u) b = 0;                                  // "-0" and "0" compare equal through stod
      b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      return (uint64_t)b << 32;
    }
    uint64_t b = bits;
    if (b == 0x8000000000000000ull) b = 0;
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
  }
  bool neg = false;
  uint64_t mag = bits;
  switch (elem) {
    case VHK_I8: { const int64_t v = (int8_t)bits; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; } break;
    case VHK_I16: { const int64_t v = (int16_t)bits; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; } break;
    case VHK_I32: { const int64_t v = (int32_t)bits; neg = v < 0; mag = neg ? (uint64_t)(-v) : (uint64_t)v; } break;
    case VHK_I64: { const int64_t v = (int64_t)bits; neg = v < 0; mag = neg ? 0ull - (uint64_t)v : (uint64_t)v; } break;
    case VHK_U8: mag = bits & 0xFFull; break;
    case VHK_U16: mag = bits & 0xFFFFull; break;
    case VHK_U32: mag = bits & 0xFFFFFFFFull; break;
    default: break;
  }
  int nd = 1;                                                        // decimal digits of |v|
  uint64_t base = 1;                                                 // 10^(nd-1)
  while (nd < 20 && mag / 10 >= base) { base *= 10; ++nd; }
  const uint64_t cls_rank = neg ? 2ull * nd + 1 : 2ull * nd;       // string length, '-' sorts before digits
  // 58 bits for the magnitude: exact up to 17 digits; the 18..20-digit classes keep (|v| - 10^(nd-1)) >> 6,
  // still monotone inside the class (the low bits only merge near-ties, which a superset tolerates)
  return (cls_rank << 58) | (nd <= 17 ? mag : (mag - base) >> 6);
}
