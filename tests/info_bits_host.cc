// tests/info_bits_host.cc — vh_result_info.reserved as viyadb_amd/csrc/vhh_info.h composes it from names, against the expression in numerals
// that QueryBuild::launch() and the select's planner carried before the bits had names. The numerals below are the ABI, frozen here: a bit
// that moves, a term that changes its condition or a rule of the pre-built plane readers that is stated differently fails this program.
// Stand-alone (its own main), built by tests/test_info_bits_host.py with g++ under UBSan.
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include "vhh_info.h"

// The expression as it stood in QueryBuild::launch(), its locals read from the struct that names them (`fast` is its `fastj || jk`,
// `lds_hash` its P.lds_hash_slots, `dense_part` its mode == VH_MODE_DENSE_PART, `pp_planes` its jshape.pp_nplanes), and the two rewrites
// that followed it.
static uint32_t legacy_bits(const VhWhatRan& w) {
  const bool hpart = w.hpart, fastj = w.fastj, jk = w.jk, lanes = w.lanes, packed = w.packed, packed_compressed = w.packed_compressed, packed_bits = w.packed_bits;
  const bool narrowed = w.narrowed, hp_pack = w.hp_pack, has_set = w.has_set, set_search = w.set_search, set_truth = w.set_truth, build_pending = w.build_pending;
  const bool grouped = w.grouped, gplanes = w.gplanes, subtrim = w.subtrim, gpspan = w.gpspan, sliced_prebuilt = w.sliced_prebuilt, plane_agg = w.plane_agg;
  const uint32_t packed_rec = w.packed_rec;
  uint32_t reserved = (hpart ? 64 : 0) | (w.fast ? 1 : 0) | (lanes ? 2 : 0) | (w.lds_hash ? 4 : 0) | (packed ? 8 : 0) | (fastj && narrowed ? 16 : 0) | (jk ? 32 : 0) | (packed && packed_compressed ? 128 : 0) | (hpart && hp_pack ? 256 : 0) | (w.dense_part && w.gid_bits ? 1024 : 0) | (jk && (w.pp_planes || w.pp_sliced) ? 2048 : 0) | (jk && w.qpay ? 4096 : 0) | (jk && w.pp_sliced ? 8192 : 0) | (w.dense_part && w.gid_bits && w.tuple4 ? 16384 : 0)
                   | (has_set ? 1u << 22 : 0) | (has_set && set_search ? 1u << 23 : 0) | (jk && has_set && set_truth && w.pp_sliced ? 1u << 25 : 0) | (build_pending ? 1u << 19 : 0) | (jk && grouped ? 1u << 20 : 0) | (jk && grouped && gplanes ? 1u << 21 : 0) | (jk && grouped && gplanes && subtrim ? 1u << 28 : 0) | (jk && grouped && gplanes && gpspan ? 1u << 29 : 0) | (packed && packed_bits ? 32768 : 0) | (packed ? (uint32_t)(31 - __builtin_clz(std::max<uint32_t>(packed_rec, 2)) - 1) << 16 : 0);
  if (sliced_prebuilt) reserved = (reserved & ~(1u | 2u | 32u)) | 1u << 26 | 1u << 4 | 1u << 11 | 1u << 13 | (has_set ? 1u << 22 | 1u << 25 : 0u);
  if (plane_agg) reserved = (reserved & ~(1u | 2u | 32u | 1u << 26 | 8u | 128u | 32768u | 7u << 16)) | 1u << 27 | 1u << 4 | 1u << 11 | 1u << 13 | (has_set ? 1u << 22 | 1u << 25 : 0u);
  return reserved;
}

// The select's, as it stood in QueryBuild::snapshot_segments().
static uint32_t legacy_select(bool sel_sliced, bool has_set, bool set_search) {
  return sel_sliced ? (1u << 4 | 1u << 11 | 1u << 13 | (has_set ? 1u << 22 | 1u << 25 : 0u))
                    : (has_set ? 1u << 22 | (set_search ? 1u << 23 : 0u) : 0u);
}

// Every boolean of the struct, one bit of `c` each.
static bool VhWhatRan::* const BOOLS[] = {
  &VhWhatRan::hpart, &VhWhatRan::fast, &VhWhatRan::fastj, &VhWhatRan::jk, &VhWhatRan::lanes, &VhWhatRan::lds_hash, &VhWhatRan::narrowed,
  &VhWhatRan::hp_pack, &VhWhatRan::dense_part, &VhWhatRan::gid_bits, &VhWhatRan::tuple4, &VhWhatRan::pp_planes, &VhWhatRan::pp_sliced,
  &VhWhatRan::qpay, &VhWhatRan::has_set, &VhWhatRan::set_search, &VhWhatRan::set_truth, &VhWhatRan::build_pending, &VhWhatRan::grouped,
  &VhWhatRan::gplanes, &VhWhatRan::subtrim, &VhWhatRan::gpspan,
  // the five that sweep (b) varies on their own
  &VhWhatRan::packed, &VhWhatRan::packed_compressed, &VhWhatRan::packed_bits, &VhWhatRan::sliced_prebuilt, &VhWhatRan::plane_agg};
constexpr int NBOOL = sizeof(BOOLS) / sizeof(BOOLS[0]), NREST = NBOOL - 5;

static VhWhatRan what(uint32_t c, uint32_t packed_rec) {
  VhWhatRan w;
  for (int i = 0; i < NBOOL; ++i) w.*BOOLS[i] = (c >> i & 1u) != 0;
  w.packed_rec = packed_rec;
  return w;
}
static bool same(const VhWhatRan& w, uint32_t c) {
  const uint32_t got = vh_info_compose(w), want = legacy_bits(w);
  if (got == want) return true;
  printf("inputs %#x, %u-byte records: composed %#x, the numerals give %#x\n", c, w.packed_rec, got, want);
  return false;
}

int main() {
  bool ok = true;
  VhWhatRan w = what(0, 4);
  for (uint32_t c = 0; c < 1u << NBOOL && ok; ++c) {
    for (uint32_t flipped = c ? c ^ (c - 1) : 0; flipped; flipped &= flipped - 1) { const int i = __builtin_ctz(flipped); w.*BOOLS[i] = (c >> i & 1u) != 0; }      // (counting up flips two booleans on average)
    ok = same(w, c);
  }
  if (ok) printf("compose: every combination of the %d booleans at 4-byte records: ok\n", NBOOL);
  bool ok_b = true;
  for (uint32_t rec : {0u, 1u, 2u, 4u, 8u, 16u, 32u, 64u})
    for (uint32_t five = 0; five < 32; ++five)
      for (uint32_t rest : {0u, (1u << NREST) - 1}) ok_b = same(what(five << NREST | rest, rec), five << NREST | rest) && ok_b;
  if (ok_b) printf("compose: records of 0 to 64 bytes with every form of projection and plane reader: ok\n");
  bool ok_s = true;
  for (int c = 0; c < 8; ++c) {
    const bool sliced = c & 1, has_set = c & 2, set_search = c & 4;
    const uint32_t got = vh_info_select(sliced, has_set, set_search), want = legacy_select(sliced, has_set, set_search);
    if (got != want) { printf("select (sliced %d, sets %d, search %d): %#x, the numerals give %#x\n", sliced, has_set, set_search, got, want); ok_s = false; }
  }
  if (ok_s) printf("select: all 8 inputs: ok\n");
  bool ok_r = true;
  for (uint32_t code = 0; code < 8; ++code)
    for (uint32_t bit3 : {0u, 8u})
      for (uint32_t others : {0u, ~(7u << 16 | 8u)}) {
        const uint32_t bits = code << 16 | bit3 | others, want = bit3 ? 2u << code : 0u;
        if (vh_info_rec_bytes(bits) != want) { printf("record bytes of %#x: %u, not %u\n", bits, vh_info_rec_bytes(bits), want); ok_r = false; }
      }
  if (ok_r) printf("record bytes: all 8 codes, bit 3 set and clear: ok\n");
  return ok && ok_b && ok_s && ok_r ? 0 : 1;
}
