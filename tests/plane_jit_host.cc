// tests/plane_jit_host.cc — the constant-parameter forms of the aggregates on the bit-sliced planes (viyadb_amd/csrc/vh_bits_agg.h:
// vh_bits_sum_c / vh_bits_min_c / vh_bits_max_c<OFF, NB>, what a kernel compiled for one plan's shape calls: vh_jit_planes.h) held to the
// `_at` forms the pre-built kernels call, for EVERY (off, nb) with off + nb <= 32 — nb = 0 included — over random plane words and
// random, all-zero, all-one and single-bit masks; MIN / MAX on the empty mask too (the value means nothing then: `empty` must say so).
// Stand-alone (its own main), built by tests/test_plane_jit_host.py with g++, plain and under ASan + UBSan. The plane words are an exact-size
// heap block, so a read outside them is an error.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <memory>
#include <random>
#include "vh_bits_agg.h"

typedef uint32_t Planes[VH_BITS_MAX_FIELD];
struct Forms {
  uint64_t (*sum)(const Planes&, uint32_t);
  uint32_t (*min)(const Planes&, uint32_t, bool*);
  uint32_t (*max)(const Planes&, uint32_t, bool*);
  bool valid;
};
static Forms g_forms[33][33];      // [off][nb]

template <int OFF, int NB> static void reg() {
  if constexpr (OFF + NB <= VH_BITS_MAX_FIELD) {
    g_forms[OFF][NB] = Forms{&vh_bits_sum_c<OFF, NB>, &vh_bits_min_c<OFF, NB>, &vh_bits_max_c<OFF, NB>, true};
    reg<OFF, NB + 1>();
  }
}
template <int OFF> static void reg_off() {
  if constexpr (OFF <= VH_BITS_MAX_FIELD) { reg<OFF, 0>(); reg_off<OFF + 1>(); }
}

int main() {
  reg_off<0>();
  std::mt19937_64 rng(20261021);
  std::unique_ptr<uint32_t[]> block(new uint32_t[VH_BITS_MAX_FIELD]);
  Planes& v = *reinterpret_cast<Planes*>(block.get());
  long checked = 0, pairs = 0;
  for (int off = 0; off <= 32; ++off)
    for (int nb = 0; off + nb <= 32; ++nb) {
      const Forms& f = g_forms[off][nb];
      if (!f.valid) { printf("no instantiation for off %d nb %d\n", off, nb); return 1; }
      ++pairs;
      for (int round = 0; round < 6; ++round) {
        for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) v[p] = round == 0 ? 0u : round == 1 ? ~0u : (uint32_t)rng();
        uint32_t masks[4 + 32 + 4];
        int nm = 0;
        masks[nm++] = 0u; masks[nm++] = ~0u;
        for (int b = 0; b < 32; ++b) masks[nm++] = 1u << b;
        for (int k = 0; k < 6; ++k) masks[nm++] = (uint32_t)rng() & (k & 1 ? (uint32_t)rng() : ~0u);
        for (int k = 0; k < nm; ++k) {
          const uint32_t m = masks[k];
          const uint64_t s_at = vh_bits_sum_at(v, (uint32_t)off, (uint32_t)nb, m), s_c = f.sum(v, m);
          bool e_at = false, e_c = true;
          const uint32_t lo_at = vh_bits_min_at(v, (uint32_t)off, (uint32_t)nb, m, &e_at), lo_c = f.min(v, m, &e_c);
          bool E_at = false, E_c = true;
          const uint32_t hi_at = vh_bits_max_at(v, (uint32_t)off, (uint32_t)nb, m, &E_at), hi_c = f.max(v, m, &E_c);
          const bool values = m == 0u || (lo_at == lo_c && hi_at == hi_c);      // (an empty mask's value means nothing)
          if (s_at != s_c || e_at != e_c || E_at != E_c || e_c != (m == 0u) || E_c != (m == 0u) || !values) {
            printf("off %d nb %d mask %08x: sum %llu / %llu, min %u / %u (empty %d / %d), max %u / %u (empty %d / %d)\n", off, nb, m,
                   (unsigned long long)s_at, (unsigned long long)s_c, lo_at, lo_c, (int)e_at, (int)e_c, hi_at, hi_c, (int)E_at, (int)E_c);
            return 1;
          }
          ++checked;
        }
      }
    }
  printf("ok: %ld fields (every off + nb <= 32), %ld (field, planes, mask) cases\n", pairs, checked);
  return 0;
}
