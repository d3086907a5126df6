// tests/plane_jit_info_host.cc — VhWhatRan::plane_jit (viyadb_amd/csrc/vhh_info.h: the plane aggregate in its compiled form) composes to bit
// 27's word plus bit 5, and changes nothing while it is false. This program takes tests/info_bits_host.cc as it is — its numerals, its list
// of the struct's booleans, its main under another name — runs it (every one of its combinations, the new field false: each must still be
// ": ok"), and then repeats its full sweep with the new field TRUE: the word is the numerals' with bit 5 set exactly where plane_agg is.
// Stand-alone, built by tests/test_capi_plane_jit.py with g++ under UBSan.
#define main info_bits_main
#include "info_bits_host.cc"
#undef main

int main() {
  if (info_bits_main() != 0) return 1;
  VhWhatRan w;
  w.packed_rec = 4;
  w.plane_jit = true;
  bool ok = true;
  for (uint32_t c = 0; c < 1u << NBOOL && ok; ++c) {
    for (uint32_t flipped = c ? c ^ (c - 1) : 0; flipped; flipped &= flipped - 1) { const int i = __builtin_ctz(flipped); w.*BOOLS[i] = (c >> i & 1u) != 0; }
    const uint32_t want = legacy_bits(w) | (w.plane_agg ? 32u : 0u), got = vh_info_compose(w);
    if (got != want) { printf("plane_jit with combination %#x: composed %#x, bit 27's word plus bit 5 is %#x\n", c, got, want); ok = false; }
  }
  // the word a compiled plane aggregate reports: bits 27, 5, 4, 11, 13 and nothing of 0, 1, 26 or the projection's
  VhWhatRan j;
  j.plane_agg = j.plane_jit = true; j.fast = j.fastj = j.lanes = j.packed = j.packed_bits = true; j.packed_rec = 4;
  const uint32_t word = vh_info_compose(j);
  if (word != (1u << 27 | 1u << 5 | 1u << 4 | 1u << 11 | 1u << 13)) { printf("a compiled plane aggregate reports %#x\n", word); ok = false; }
  printf("plane_jit over 2^%d combinations: %s\n", NBOOL, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
