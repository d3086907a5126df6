// Host check of viyadb_amd/csrc/vh_inset.h (plain C++, no GPU): for every integer element type, both lookup forms of a set —
// the bitmap and the sorted array — must agree with a linear search over the list as the caller gave it.
// A stand-alone program (tests/test_inset_host.py compiles and runs it, once plain and once with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

#include "vh_inset.h"

static long g_checks = 0, g_lists = 0;
static int g_fail = 0;

template <typename T> struct Elem;
template <> struct Elem<uint8_t> { static constexpr int id = 0; static constexpr const char* name = "u8"; };
template <> struct Elem<uint16_t> { static constexpr int id = 1; static constexpr const char* name = "u16"; };
template <> struct Elem<uint32_t> { static constexpr int id = 2; static constexpr const char* name = "u32"; };
template <> struct Elem<uint64_t> { static constexpr int id = 3; static constexpr const char* name = "u64"; };
template <> struct Elem<int8_t> { static constexpr int id = 4; static constexpr const char* name = "i8"; };
template <> struct Elem<int16_t> { static constexpr int id = 5; static constexpr const char* name = "i16"; };
template <> struct Elem<int32_t> { static constexpr int id = 6; static constexpr const char* name = "i32"; };
template <> struct Elem<int64_t> { static constexpr int id = 7; static constexpr const char* name = "i64"; };

// the literal as the C ABI carries it: the value in the low bytes of an 8-byte word (vh_anynum)
template <typename T> static uint64_t bits_of(T v) { uint64_t b = 0; memcpy(&b, &v, sizeof(T)); return b; }

template <typename T> static bool linear(const std::vector<T>& list, T v) {
  bool hit = false;
  for (T m : list) hit |= m == v;
  return hit;
}

// expect_form: -1 = whatever the builder picks
template <typename T> static void check_list(const std::vector<T>& list, int expect_form, std::mt19937_64& rng, const char* what) {
  typedef std::numeric_limits<T> L;
  typedef typename std::make_unsigned<T>::type U;
  std::vector<uint64_t> bits;
  for (T m : list) bits.push_back(bits_of<T>(m));
  VhSetHost h[2];
  vh_inset_build(Elem<T>::id, bits.data(), bits.size(), false, &h[0]);
  vh_inset_build(Elem<T>::id, bits.data(), bits.size(), true, &h[1]);
  ++g_lists;
  if (expect_form >= 0 && (int)h[0].form != expect_form) { printf("FAIL %s %s: form %u, expected %d (span %llu)\n", Elem<T>::name, what, h[0].form, expect_form, (unsigned long long)h[0].span); ++g_fail; }
  if (h[0].form == VH_SET_BITMAP && h[0].span >= VH_INSET_BITMAP_SPAN) { printf("FAIL %s %s: a bitmap of span %llu\n", Elem<T>::name, what, (unsigned long long)h[0].span); ++g_fail; }
  if (h[0].form == VH_SET_BITMAP && h[0].words.size() * 4 > (128u << 10)) { printf("FAIL %s %s: a bitmap of %zu bytes\n", Elem<T>::name, what, h[0].words.size() * 4); ++g_fail; }
  if (h[1].form == VH_SET_BITMAP) { printf("FAIL %s %s: the forced search form is a bitmap\n", Elem<T>::name, what); ++g_fail; }
  if ((h[1].form == VH_SET_ARRAY32) != (h[1].span < (1ull << 32))) { printf("FAIL %s %s: key width of span %llu\n", Elem<T>::name, what, (unsigned long long)h[1].span); ++g_fail; }
  // exact-size copies of the tables: a read past the end is the sanitizer's to find
  std::vector<uint32_t> tab[2] = {std::vector<uint32_t>(h[0].words), std::vector<uint32_t>(h[1].words)};
  VhSetDev d[2] = {h[0].dev(tab[0].data()), h[1].dev(tab[1].data())};
  std::vector<T> probes;
  for (T m : list) {
    probes.push_back(m);
    probes.push_back((T)((U)m + (U)1));          // (wraps at the type's ends, like the column's own arithmetic)
    probes.push_back((T)((U)m - (U)1));
  }
  probes.push_back(L::min()); probes.push_back(L::max()); probes.push_back((T)0);
  T lo = list[0], hi = list[0];
  for (T m : list) { lo = m < lo ? m : lo; hi = m > hi ? m : hi; }
  for (int i = 0; i < 10000; ++i) {
    const uint64_t r = rng();
    if (i & 1) probes.push_back((T)r);            // anywhere in the type
    else probes.push_back((T)((U)lo - (U)8 + (U)(r % ((uint64_t)(U)((U)hi - (U)lo) + 17ull))));   // in and around [lo, hi]
  }
  for (T v : probes) {
    const bool want = linear<T>(list, v);
    for (int f = 0; f < 2; ++f) {
      ++g_checks;
      if (vh_inset_has<T>(d[f], v) != want) {
        if (g_fail < 20) printf("FAIL %s %s form %u: lookup(%lld) = %d, linear search says %d\n", Elem<T>::name, what, d[f].form, (long long)v, (int)!want, (int)want);
        ++g_fail;
      }
    }
  }
}

template <typename T> static void check_type(std::mt19937_64& rng) {
  typedef std::numeric_limits<T> L;
  typedef typename std::make_unsigned<T>::type U;
  const uint64_t type_span = (uint64_t)(U)((U)L::max() - (U)L::min());
  char what[96];
  // lists of 1 .. 3000 members around zero, with duplicates, with and without the type's extremes
  for (int n : {1, 2, 3, 7, 32, 33, 64, 255, 600, 3000}) {
    for (int ends = 0; ends < 2; ++ends) {
      std::vector<T> list;
      const uint64_t width = type_span < 5000 ? type_span : (uint64_t)(2 * n + 50);
      for (int i = 0; i < n; ++i) list.push_back((T)((U)(T)(L::is_signed ? -(int64_t)(width / 2) : 0) + (U)(rng() % (width + 1))));
      for (int i = 0; i + 1 < n; i += 5) list[(size_t)i + 1] = list[(size_t)i];      // duplicates
      if (ends && n >= 2) { list[0] = L::min(); list[(size_t)n - 1] = L::max(); }
      snprintf(what, sizeof(what), "%d members%s", n, ends ? " with min and max" : "");
      check_list<T>(list, -1, rng, what);
    }
  }
  // spans on both sides of every boundary of the two forms
  struct SpanCase { uint64_t span; int form; };
  const SpanCase spans[] = {{31, VH_SET_BITMAP}, {32, VH_SET_BITMAP}, {33, VH_SET_BITMAP}, {63, VH_SET_BITMAP}, {64, VH_SET_BITMAP}, {65, VH_SET_BITMAP},
                            {(1ull << 20) - 1, VH_SET_BITMAP}, {1ull << 20, VH_SET_ARRAY32}, {(1ull << 32) - 1, VH_SET_ARRAY32}, {1ull << 32, VH_SET_ARRAY64},
                            {(1ull << 32) + 1, VH_SET_ARRAY64}, {1ull << 63, VH_SET_ARRAY64}, {~0ull, VH_SET_ARRAY64}};
  for (const SpanCase& sc : spans) {
    if (sc.span > type_span) continue;            // (the type has no two values that far apart)
    for (int at = 0; at < 3; ++at) {              // the span at the type's bottom, across zero / in the middle, at its top
      const U room = (U)(type_span - sc.span);
      const U base = (U)((U)L::min() + (at == 0 ? (U)0 : at == 1 ? (U)(room / 2) : room));
      std::vector<T> list = {(T)base, (T)(base + (U)sc.span)};
      for (int i = 0; i < 40; ++i) list.push_back((T)(base + (U)(sc.span == ~0ull ? rng() : rng() % (sc.span + 1))));
      list.push_back(list[1]);
      snprintf(what, sizeof(what), "span %llu at %d", (unsigned long long)sc.span, at);
      check_list<T>(list, sc.form, rng, what);
    }
  }
}

int main() {
  std::mt19937_64 rng(20240607);
  check_type<uint8_t>(rng); check_type<uint16_t>(rng); check_type<uint32_t>(rng); check_type<uint64_t>(rng);
  check_type<int8_t>(rng); check_type<int16_t>(rng); check_type<int32_t>(rng); check_type<int64_t>(rng);
  printf("%s: %ld lookups over %ld lists, %d wrong\n", g_fail ? "FAILED" : "ok", g_checks, g_lists, g_fail);
  return g_fail ? 1 : 0;
}
