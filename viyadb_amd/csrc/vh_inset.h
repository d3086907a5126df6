// vh_inset.h — membership of an integer in a SET, as one lookup per row however long the list (VH_F_INSET, include/viya_hip.h).
// Plain C++: the kernels include it (vh_kernels.h: vh_leaf; vh_jit_body.h: vj_inset, vj_bits_inset), the planner builds the sets with it
// (vhh_plan.h), and host-compiled checks hold both lookup forms and the truth-table form against a linear search (tests/inset_host.cc,
// tests/inset_bits_host.cc).
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
//
// A THIRD form serves the scan over the bit-sliced predicate planes, where no lane holds a row's value: a field of NB <= VH_INSET_TRUTH_BITS
// bits holds the column's non-negative value as it is, so the set is a Boolean function of NB bit planes, given as a TRUTH TABLE of 2^NB
// bits (bit v set <=> v is a member; members outside [0, 2^NB) are in no row of the projection and are dropped). vh_inset_bits<NB> evaluates
// it for a lane's 32 rows with bitwise operations only: the table's low five address bits are a 5-input look-up table (31 bit-selects on
// x[0..4]), the high ones pick a 32-bit table word — a wave-uniform value, skipped with a scalar branch when it is zero. The cost goes by
// the non-empty words (at most 2^(NB-5)), never by the list's length. The truth table lies behind the set's ordinary table (VhSetHost::words).
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
// (a truth table is written before the launch and never while a kernel runs: constant address space, so a wave-uniform address is a scalar load)
#define VH_INSET_CPTR(T, p) ((const T __attribute__((address_space(4)))*)(p))
#define VH_INSET_NO_UNROLL _Pragma("unroll 1")
#define VH_INSET_UNROLL _Pragma("unroll")
#else
#define VH_INSET_PTR(T, p) ((const T*)(p))
#define VH_INSET_CPTR(T, p) ((const T*)(p))
#define VH_INSET_NO_UNROLL
#define VH_INSET_UNROLL
#endif

#ifndef VH_MAX_SETS
#define VH_MAX_SETS 4            // set leaves per plan (= include/viya_hip.h)
#endif
#define VH_INSET_BITMAP_SPAN (1ull << 20)      // a set whose span is below this is a bitmap
#define VH_INSET_TRUTH_BITS 10                 // the widest bit-sliced field a set leaf is evaluated on as a truth table (32 table words)

enum { VH_SET_BITMAP = 0, VH_SET_ARRAY32 = 1, VH_SET_ARRAY64 = 2 };

struct VhSetDev {           // 40 bytes, words only (see VH_PACKED_FIELD in vh_internal.h on sub-dword members of kernel arguments)
  const void* table;        // bitmap words, or the sorted (key - lo) as uint32_t / uint64_t
  uint64_t lo;              // order key of the smallest member
  uint64_t span;            // order key of the largest member - lo
  uint32_t n;               // distinct members, >= 1
  uint32_t form;            // VH_SET_*
  const uint32_t* truth;    // the truth table over the leaf's bit-sliced field (max(2, 2^(NB - 5)) words), or null: only a scan on bit planes reads it
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

// ------------------------------------------------------------------ the truth-table form: 32 rows per call, bit planes in, a mask out
// bit k of the result: bit k of a where m has a 1, of b elsewhere (one v_bfi_b32)
VH_INSET_FN uint32_t vh_inset_sel(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }

// W as a look-up table of NB <= 5 inputs: bit k of the result = bit (x[0] | x[1] << 1 | ... of row k) of W. The first level selects between
// all-ones / all-zeros masks made of W's bits (W is uniform over a wave: scalar work), then 2^(NB-1) - 1 selects on x[1 .. NB).
template <int NB> VH_INSET_FN uint32_t vh_inset_lut(uint32_t W, const uint32_t* x) {
  static_assert(NB >= 1 && NB <= 5, "a table word has five address bits");
  uint32_t t[1 << (NB - 1)];
  VH_INSET_UNROLL
  for (int i = 0; i < (1 << (NB - 1)); ++i) t[i] = vh_inset_sel(x[0], 0u - ((W >> (2 * i + 1)) & 1u), 0u - ((W >> (2 * i)) & 1u));
  VH_INSET_UNROLL
  for (int b = 1; b < NB; ++b) {
    VH_INSET_UNROLL
    for (int i = 0; i < (1 << (NB - 1 - b)); ++i) t[i] = vh_inset_sel(x[b], t[2 * i + 1], t[2 * i]);
  }
  return t[0];
}

// One table word over MINTERMS of its five address bits — p[j]: the rows whose bits 0..2 spell j, q[k]: bits 3..4 spell k — which a call
// works out once for all of its table words: a byte of W is then eight and-ors of p[] with all-ones / all-zeros masks of W's bits, the word
// four and-ors of its bytes with q[]: 36 operations where the selects of vh_inset_lut<5> take 63, and none for an empty byte.
VH_INSET_FN uint32_t vh_inset_word(uint32_t W, const uint32_t* p, const uint32_t* q) {
  uint32_t r = 0u;
  VH_INSET_UNROLL
  for (int k = 0; k < 4; ++k) {
    if (((W >> (8 * k)) & 0xFFu) == 0u) continue;      // (uniform over the wave, like W: a sparse set pays for the bytes that hold members)
    uint32_t b = 0u;
    VH_INSET_UNROLL
    for (int j = 0; j < 8; ++j) b |= p[j] & (0u - ((W >> (8 * k + j)) & 1u));
    r |= b & q[k];
  }
  return r;
}

// x[b]: plane b of the lane's 32 rows (what vj_bits_rel takes); truth: 2^NB bits, at least two words; -> the rows whose value is a member.
// NB > 5: the table's words in groups of up to eight, the next group's loaded while this one's are evaluated (so no word is waited for
// where it is used), an empty word or group skipped — the words, hence the branches, are uniform over a wave.
template <int NB> VH_INSET_FN uint32_t vh_inset_bits(const uint32_t* x, const uint32_t* truth) {
  static_assert(NB >= 1 && NB <= 16, "a truth table of 2^NB bits");
  if constexpr (NB <= 5) {
    return vh_inset_lut<NB>(VH_INSET_CPTR(uint32_t, truth)[0], x);
  } else {
    constexpr int NW = 1 << (NB - 5), GS = NW < 8 ? NW : 8, NG = NW / GS;
    uint32_t p[8], q[4], w[GS], nxt[GS];
    VH_INSET_UNROLL
    for (int j = 0; j < 8; ++j) p[j] = (j & 1 ? x[0] : ~x[0]) & (j & 2 ? x[1] : ~x[1]) & (j & 4 ? x[2] : ~x[2]);
    VH_INSET_UNROLL
    for (int k = 0; k < 4; ++k) q[k] = (k & 1 ? x[3] : ~x[3]) & (k & 2 ? x[4] : ~x[4]);
    VH_INSET_UNROLL
    for (int i = 0; i < GS; ++i) { w[i] = VH_INSET_CPTR(uint32_t, truth)[i]; nxt[i] = 0u; }
    uint32_t acc = 0u;
    VH_INSET_NO_UNROLL
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) {
        VH_INSET_UNROLL
        for (int i = 0; i < GS; ++i) nxt[i] = VH_INSET_CPTR(uint32_t, truth)[(g + 1) * GS + i];
      }
      uint32_t any = 0u;
      VH_INSET_UNROLL
      for (int i = 0; i < GS; ++i) any |= w[i];
      if (any) {
        uint32_t eqg = ~0u;        // rows whose address bits above a group's word index are g's (planes from 5 + log2 GS up)
        VH_INSET_UNROLL
        for (int b = 5; b < NB; ++b) if ((1 << (b - 5)) >= GS) eqg &= x[b] ^ (((uint32_t)(g * GS) >> (b - 5)) & 1u ? 0u : ~0u);
        VH_INSET_UNROLL
        for (int i = 0; i < GS; ++i) {
          if (w[i] == 0u) continue;
          uint32_t eq = eqg;
          VH_INSET_UNROLL
          for (int b = 5; b < NB; ++b) if ((1 << (b - 5)) < GS) eq &= (i >> (b - 5)) & 1 ? x[b] : ~x[b];
          acc |= vh_inset_word(w[i], p, q) & eq;
        }
      }
      VH_INSET_UNROLL
      for (int i = 0; i < GS; ++i) w[i] = nxt[i];
    }
    return acc;
  }
}

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
  std::vector<uint32_t> words;     // the device table, an even number of 32-bit words (so that tables laid end to end stay 8-byte aligned) ...
  size_t truth_word = 0;           // ... and behind it, from this word on, the truth table over a bit-sliced field (vh_inset_truth_build) ...
  int truth_bits = 0;              // ... of this many bits; 0: no such table
  uint64_t lo = 0, span = 0;
  uint32_t n = 0, form = VH_SET_BITMAP;
  VhSetDev dev(const void* table) const {
    VhSetDev d; d.table = table; d.lo = lo; d.span = span; d.n = n; d.form = form;
    d.truth = truth_bits ? (const uint32_t*)table + truth_word : nullptr;
    return d;
  }
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
  s.words.clear(); s.truth_word = 0; s.truth_bits = 0;
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

// The truth table of a built set over a field of nb bits (1 .. 16) that holds the column's non-negative value as it is: 2^nb bits, an even
// number of words and at least two, appended to (or rewritten behind) the set's ordinary table. Members that are negative or >= 2^nb are
// in no row of such a field: dropped. `elem`: the element type the set was built for.
static inline void vh_inset_truth_build(int elem, int nb, VhSetHost* out) {
  VhSetHost& s = *out;
  if (s.truth_bits) s.words.resize(s.truth_word);
  s.truth_word = s.words.size();
  s.truth_bits = nb;
  const size_t nw = std::max<size_t>(2, ((size_t)1 << nb) / 32);
  s.words.resize(s.truth_word + nw, 0u);
  const uint64_t zero = elem >= 4 ? 1ull << 63 : 0ull;       // the order key of the value 0
  for (auto it = std::lower_bound(s.keys.begin(), s.keys.end(), zero); it != s.keys.end(); ++it) {
    const uint64_t v = *it - zero;
    if (v >> nb) break;
    s.words[s.truth_word + (size_t)(v >> 5)] |= 1u << (v & 31u);
  }
}
#endif
