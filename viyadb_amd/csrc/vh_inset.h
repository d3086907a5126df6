// vh_inset.h — membership of an integer in a SET, as one lookup per row however long the list (VH_F_INSET, include/viya_hip.h).
// Plain C++: the kernels include it (vh_kernels.h: vh_leaf; vh_jit_body.h: vj_inset), the planner builds the sets with it
// (vhh_plan.h), and a host-compiled check holds both lookup forms against a linear search (tests/inset_host.cc).
//
// The reference — and VH_F_IN here — spends one `==` per value and row (ComparisonBuilder, src/codegen/query/filter.cc:223-241).
// A set leaf spends one lookup:
//   * members are ordered by their ORDER KEY (order_key_of_bits, vhh_result.h): unsigned values as they are, signed values
//     sign-extended and XORed with 2^63 — one unsigned order for every integer element type;
//   * the builder sorts and de-duplicates them and records lo (the smallest key), span (the largest key - lo), n (distinct members);
//   * BITMAP when span < 2^20: span + 1 bits, at most 128 KiB — a small part of an XCD's 4 MiB L2, ~3 us to upload.
//       k = key(v) - lo (64-bit wrap);  member <=> k <= span && (words[k >> 5] >> (k & 31) & 1)
//   * SORTED ARRAY otherwise: key - lo as uint32_t (span < 2^32) or uint64_t; a branchless lower bound of ceil(log2 n) steps — n is
//     uniform over a wave, so its lanes do not diverge.
// Which form a set takes is RUN-TIME data (VhSetDev::form, a scalar branch in the kernels): a compiled scan kernel knows only "a set
// leaf on element type T", so lists of any length and form on one plan shape run the same code object.
// Both forms are read with plain cached loads (the column streams are non-temporal; the table is what should stay in cache).
#pragma once
#include <stdint.h>
#ifndef VH_INSET_FN
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define VH_INSET_FN __host__ __device__ __forceinline__
#else
#define VH_INSET_FN static inline
#endif
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// (the table's address comes out of the kernel arguments: a device allocation, not a generic pointer — global_load, not flat_load)
#define VH_INSET_PTR(T, p) ((const T __attribute__((address_space(1)))*)(p))
#else
#define VH_INSET_PTR(T, p) ((const T*)(p))
#endif

#ifndef VH_MAX_SETS
#define VH_MAX_SETS 4            // set leaves per plan (= include/viya_hip.h)
#endif
#define VH_INSET_BITMAP_SPAN (1ull << 20)      // a set whose span is below this is a bitmap

enum { VH_SET_BITMAP = 0, VH_SET_ARRAY32 = 1, VH_SET_ARRAY64 = 2 };

struct VhSetDev {           // 32 bytes, words only (see VH_PACKED_FIELD in vh_internal.h on sub-dword members of kernel arguments)
  const void* table;        // bitmap words, or the sorted (key - lo) as uint32_t / uint64_t
  uint64_t lo;              // order key of the smallest member
  uint64_t span;            // order key of the largest member - lo
  uint32_t n;               // distinct members, >= 1
  uint32_t form;            // VH_SET_*
};

// the order key of a value of element type T
template <typename T> VH_INSET_FN uint64_t vh_inset_key(T v) {
  if (T(-1) < T(0)) return (uint64_t)(int64_t)v ^ (1ull << 63);
  return (uint64_t)v;
}

// rank of the first element of a[0, n) that is not below k, as long as it is < n - 1; else n - 1 (n >= 1): every index read is < n
template <typename W> VH_INSET_FN uint32_t vh_inset_lower(const W* a, uint32_t n, W k) {
  uint32_t base = 0, len = n;
  while (len > 1) {
    const uint32_t half = len >> 1;
    base += (VH_INSET_PTR(W, a)[base + half - 1] < k) ? half : 0u;
    len -= half;
  }
  return base;
}

VH_INSET_FN bool vh_inset_has_key(const VhSetDev& s, uint64_t key) {
  const uint64_t k = key - s.lo;               // (wraps for keys below lo: then k > span, since span <= UINT64_MAX - lo)
  const bool in = k <= s.span;
  if (s.form == VH_SET_BITMAP) {
    const uint32_t w = in ? VH_INSET_PTR(uint32_t, s.table)[k >> 5] : 0u;
    return ((w >> (k & 31u)) & 1u) != 0u;
  }
  if (s.form == VH_SET_ARRAY32) {
    const uint32_t* a = (const uint32_t*)s.table;
    const uint32_t kk = (uint32_t)k;
    return in & (VH_INSET_PTR(uint32_t, a)[vh_inset_lower<uint32_t>(a, s.n, kk)] == kk);
  }
  const uint64_t* a = (const uint64_t*)s.table;
  return in & (VH_INSET_PTR(uint64_t, a)[vh_inset_lower<uint64_t>(a, s.n, k)] == k);
}
template <typename T> VH_INSET_FN bool vh_inset_has(const VhSetDev& s, T v) { return vh_inset_has_key(s, vh_inset_key<T>(v)); }

// ------------------------------------------------------------------ the builder (host code; the run-time compiler never sees it)
#if !defined(__HIPCC_RTC__)
#include <algorithm>
#include <vector>

// order key of a literal given as raw bits in an integer element type (enum vh_elem: 0..3 unsigned, 4..7 signed, 1 << (elem & 3) bytes)
static inline uint64_t vh_inset_key_of_bits(int elem, uint64_t bits) {
  switch (elem) {
    case 0: return (uint8_t)bits;
    case 1: return (uint16_t)bits;
    case 2: return (uint32_t)bits;
    case 3: return bits;
    case 4: return (uint64_t)(int64_t)(int8_t)bits ^ (1ull << 63);
    case 5: return (uint64_t)(int64_t)(int16_t)bits ^ (1ull << 63);
    case 6: return (uint64_t)(int64_t)(int32_t)bits ^ (1ull << 63);
    default: return bits ^ (1ull << 63);
  }
}

struct VhSetHost {
  std::vector<uint64_t> keys;      // the members' order keys, sorted, distinct (segment skipping searches these)
  std::vector<uint32_t> words;     // the device table, an even number of 32-bit words (so that tables laid end to end stay 8-byte aligned)
  uint64_t lo = 0, span = 0;
  uint32_t n = 0, form = VH_SET_BITMAP;
  VhSetDev dev(const void* table) const { VhSetDev d; d.table = table; d.lo = lo; d.span = span; d.n = n; d.form = form; return d; }
  // some member lies in [kmin, kmax] (order keys)
  bool any_in(uint64_t kmin, uint64_t kmax) const {
    const auto it = std::lower_bound(keys.begin(), keys.end(), kmin);
    return it != keys.end() && *it <= kmax;
  }
};

// `count` >= 1 literals of element type `elem` as raw bits, 8 bytes apart (vh_anynum); search: the sorted-array form whatever the span
static inline void vh_inset_build(int elem, const uint64_t* bits, size_t count, bool search, VhSetHost* out) {
  VhSetHost& s = *out;
  s.keys.resize(count);
  for (size_t i = 0; i < count; ++i) s.keys[i] = vh_inset_key_of_bits(elem, bits[i]);
  std::sort(s.keys.begin(), s.keys.end());
  s.keys.erase(std::unique(s.keys.begin(), s.keys.end()), s.keys.end());
  s.n = (uint32_t)s.keys.size();
  s.lo = s.keys.empty() ? 0 : s.keys.front();
  s.span = s.keys.empty() ? 0 : s.keys.back() - s.lo;
  s.words.clear();
  if (!search && s.span < VH_INSET_BITMAP_SPAN) {
    s.form = VH_SET_BITMAP;
    s.words.assign((size_t)((s.span + 1 + 63) / 64 * 2), 0u);
    for (uint64_t k : s.keys) { const uint64_t d = k - s.lo; s.words[(size_t)(d >> 5)] |= 1u << (d & 31u); }
  } else if (s.span < (1ull << 32)) {
    s.form = VH_SET_ARRAY32;
    s.words.assign(((size_t)s.n + 1) / 2 * 2, 0u);
    for (size_t i = 0; i < s.keys.size(); ++i) s.words[i] = (uint32_t)(s.keys[i] - s.lo);
  } else {
    s.form = VH_SET_ARRAY64;
    s.words.assign((size_t)s.n * 2, 0u);
    for (size_t i = 0; i < s.keys.size(); ++i) { const uint64_t d = s.keys[i] - s.lo; s.words[2 * i] = (uint32_t)d; s.words[2 * i + 1] = (uint32_t)(d >> 32); }
  }
}
#endif
