// Host check of the ROW SINK of the aggregate on the bit-sliced planes (viyadb_amd/csrc/vh_bits_agg.h: vh_bits_row / vh_bits_row_bit /
// vh_bits_row_field / vh_bits_row_gid, plain C++, no GPU; the device side is vh_plane_agg.h: vh_plane_agg_rows). A stand-alone program
// (tests/test_plane_rows_host.py compiles and runs it, once plain and once with -fsanitize=address,undefined).
//
// 1. Records. Random projections of 1 to 32 planes — fields at plane 0 and fields that end at plane 31 among them, one to three group columns
//    with lo > 0 and an extent that leaves values below lo and at or beyond lo + extent in the rows, up to two metric fields, planes no field
//    covers holding noise — and for every row of a plane word: vh_bits_row equals the row's values at their fields' places, vh_bits_row_gid
//    equals Σ (value - lo) * stride, and its verdict is false exactly for a row with a value outside [lo, lo + extent).
// 2. The two sinks. A wave is 64 lanes of 32 plane words and a pass mask each. A host model of the row sink — the mask in four slices of
//    eight bits, per slice an exclusive prefix of the lanes' popcounts, one queue entry `lane << 5 | bit` per set bit at that position, the
//    queue drained in groups of 64, per entry the record out of the SOURCE lane's words and one update per metric — and a host model of the
//    loop over group ids (vh_plane_agg_groups: vh_bits_match, vh_bits_sum_at / _min_at / _max_at per lane, combined over the wave, one update
//    per id and metric) fill two tables from the same identities. For G <= 64 they must agree bit for bit, presence bytes and range verdict
//    included, across SUM32 (wrapping), SUM64, and MIN / MAX of I32 / U32 / I64 / U64.
// A lane's 32 plane words are an exact-size heap block: a read outside them is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "vh_bits_agg.h"

static long g_checks = 0;
static int g_fail = 0;
static std::mt19937_64 rng(20261021);

typedef uint32_t Planes[VH_BITS_MAX_FIELD];
struct Lane {
  std::unique_ptr<uint32_t[]> mem{new uint32_t[VH_BITS_MAX_FIELD]};
  Planes& v() { return *reinterpret_cast<Planes*>(mem.get()); }
  const Planes& v() const { return *reinterpret_cast<const Planes*>(mem.get()); }
  void noise() { for (int p = 0; p < VH_BITS_MAX_FIELD; ++p) mem[p] = (uint32_t)rng(); }
  void put(uint32_t off, uint32_t nb, const uint64_t* values) {
    for (uint32_t b = 0; b < nb; ++b) {
      uint32_t w = 0;
      for (int i = 0; i < 32; ++i) w |= (uint32_t)((values[i] >> b) & 1u) << i;
      mem[off + b] = w;
    }
  }
};

struct Group { uint64_t lo, extent, stride; };      // what vh_bits_row_gid reads of VhGroupDev
enum Sop { ADD32, ADD64, MIN_I32, MAX_I32, MIN_U32, MAX_U32, MIN_I64, MAX_I64, MIN_U64, MAX_U64, NSOP };
static const char* const kSopName[NSOP] = {"ADD32", "ADD64", "MIN_I32", "MAX_I32", "MIN_U32", "MAX_U32", "MIN_I64", "MAX_I64", "MIN_U64", "MAX_U64"};
static bool sop_is_add(int s) { return s == ADD32 || s == ADD64; }
static bool sop_is_min(int s) { return s == MIN_I32 || s == MIN_U32 || s == MIN_I64 || s == MIN_U64; }
static bool sop_32(int s) { return s == ADD32 || s == MIN_I32 || s == MAX_I32 || s == MIN_U32 || s == MAX_U32; }
static uint64_t sop_ident(int s) {
  switch (s) {
    case MIN_I32: return (uint32_t)INT32_MAX;
    case MAX_I32: return (uint32_t)INT32_MIN;
    case MIN_U32: return UINT32_MAX;
    case MIN_I64: return (uint64_t)INT64_MAX;
    case MAX_I64: return (uint64_t)INT64_MIN;
    case MIN_U64: return UINT64_MAX;
    default: return 0;      // sums, MAX of unsigned
  }
}
// vh_state_update on the host: the state's own width and signedness, a u32 sum wraps
static void state_update(uint64_t* state, int s, uint64_t bits) {
  switch (s) {
    case ADD32: *state = (uint32_t)((uint32_t)*state + (uint32_t)bits); break;
    case ADD64: *state += bits; break;
    case MIN_I32: if ((int32_t)bits < (int32_t)*state) *state = (uint32_t)bits; break;
    case MAX_I32: if ((int32_t)bits > (int32_t)*state) *state = (uint32_t)bits; break;
    case MIN_U32: if ((uint32_t)bits < (uint32_t)*state) *state = (uint32_t)bits; break;
    case MAX_U32: if ((uint32_t)bits > (uint32_t)*state) *state = (uint32_t)bits; break;
    case MIN_I64: if ((int64_t)bits < (int64_t)*state) *state = bits; break;
    case MAX_I64: if ((int64_t)bits > (int64_t)*state) *state = bits; break;
    case MIN_U64: if (bits < *state) *state = bits; break;
    case MAX_U64: if (bits > *state) *state = bits; break;
  }
  if (sop_32(s)) *state &= 0xFFFFFFFFull;
}

struct Field { uint32_t off, nb; };
struct Layout {
  int ngroup = 0, nmetric = 0;
  Field gf[3], mf[2];
  Group g[3];
  uint32_t goff[3], gbits[3], need = 0, care = 0;
  uint64_t G = 1;
};
static uint32_t field_mask(const Field& f) { return (f.nb >= 32u ? ~0u : (1u << f.nb) - 1u) << f.off; }

// A random layout: the fields in random order from plane `first` on, without gaps between them; maxg bounds a group field's width.
static Layout make_layout(int ngroup, int nmetric, uint32_t first, uint32_t planes, uint32_t maxg) {
  Layout L;
  L.ngroup = ngroup; L.nmetric = nmetric;
  const int nf = ngroup + nmetric;
  std::vector<uint32_t> w((size_t)nf, 1u);
  uint32_t left = planes - (uint32_t)nf;
  while (left) {      // a plane more for a random field that may still grow; none may: the projection stays narrower
    std::vector<int> open;
    for (int k = 0; k < nf; ++k) if (w[(size_t)k] < (k < ngroup ? maxg : 32u)) open.push_back(k);
    if (open.empty()) break;
    ++w[(size_t)open[(size_t)(rng() % open.size())]]; --left;
  }
  std::vector<int> order((size_t)nf);
  for (int k = 0; k < nf; ++k) order[(size_t)k] = k;
  for (int k = nf - 1; k > 0; --k) std::swap(order[(size_t)k], order[(size_t)(rng() % (uint64_t)(k + 1))]);
  uint32_t at = first;
  for (int k : order) {
    const Field f{at, w[(size_t)k]};
    at += f.nb;
    if (k < ngroup) L.gf[k] = f; else L.mf[k - ngroup] = f;
  }
  uint64_t stride = 1;
  for (int i = ngroup - 1; i >= 0; --i) {      // the last column is the fastest digit, as the planner lays ids out
    const uint64_t top = 1ull << L.gf[i].nb;
    const uint64_t lo = top == 2 ? 1 : 1 + rng() % (top - 1);                   // 1 .. top - 1: lo > 0, value 0 is always below it
    const uint64_t extent = 1 + rng() % (top - lo);                             // lo + extent <= top; often less: values beyond the range
    L.g[i] = Group{lo, extent, stride};
    stride *= extent;
    L.goff[i] = L.gf[i].off; L.gbits[i] = L.gf[i].nb;
    L.care |= field_mask(L.gf[i]);
  }
  L.G = stride;
  L.need = L.care;
  for (int j = 0; j < nmetric; ++j) L.need |= field_mask(L.mf[j]);
  return L;
}

struct Rows { uint64_t gv[3][32], mv[2][32]; };
static void fill_lane(const Layout& L, Lane& lane, Rows& R, int kind) {
  lane.noise();
  for (int i = 0; i < L.ngroup; ++i) {
    const uint64_t top = 1ull << L.gf[i].nb;
    for (int r = 0; r < 32; ++r) {
      uint64_t x = rng() % top;
      if (kind == 1) x = L.g[i].lo + rng() % L.g[i].extent;      // every row within the range
      if (kind == 2) x = L.g[i].lo;                              // every row in ONE id
      R.gv[i][r] = x;
    }
    lane.put(L.gf[i].off, L.gf[i].nb, R.gv[i]);
  }
  for (int j = 0; j < L.nmetric; ++j) {
    const uint64_t top = L.mf[j].nb >= 32 ? 0xFFFFFFFFull : (1ull << L.mf[j].nb) - 1;
    for (int r = 0; r < 32; ++r) {
      uint64_t x = rng() & top;
      if (kind == 2) x = top;                                    // the largest value everywhere: a 32-bit sum wraps soonest, ties in MIN / MAX
      if (kind == 3) x = 0;
      R.mv[j][r] = x;
    }
    lane.put(L.mf[j].off, L.mf[j].nb, R.mv[j]);
  }
}

static void fail(const char* what, const Layout& L, uint64_t got, uint64_t want) {
  if (++g_fail > 20) return;
  printf("FAIL %s: got %llu (%#llx), want %llu (%#llx); groups", what, (unsigned long long)got, (unsigned long long)got, (unsigned long long)want, (unsigned long long)want);
  for (int i = 0; i < L.ngroup; ++i) printf(" [off %u nb %u lo %llu ext %llu stride %llu]", L.gf[i].off, L.gf[i].nb, (unsigned long long)L.g[i].lo, (unsigned long long)L.g[i].extent, (unsigned long long)L.g[i].stride);
  for (int j = 0; j < L.nmetric; ++j) printf(" metric [off %u nb %u]", L.mf[j].off, L.mf[j].nb);
  printf("\n");
}

// ---- 1. records and ids against the rows they were sliced from
static void check_records(const Layout& L, int kind) {
  Lane lane;
  Rows R;
  fill_lane(L, lane, R, kind);
  for (uint32_t r = 0; r < 32; ++r) {
    uint32_t want = 0;
    uint64_t id = 0;
    bool ok = true;
    for (int i = 0; i < L.ngroup; ++i) {
      want |= (uint32_t)R.gv[i][r] << L.gf[i].off;
      if (R.gv[i][r] < L.g[i].lo || R.gv[i][r] >= L.g[i].lo + L.g[i].extent) ok = false;
      else id += (R.gv[i][r] - L.g[i].lo) * L.g[i].stride;
    }
    for (int j = 0; j < L.nmetric; ++j) want |= (uint32_t)R.mv[j][r] << L.mf[j].off;
    const uint32_t rec = vh_bits_row(lane.v(), L.need, r);
    ++g_checks;
    if (rec != want) fail("vh_bits_row", L, rec, want);
    uint32_t by_bit = 0;
    for (uint32_t p = 0; p < 32; ++p) if ((L.need >> p) & 1u) by_bit |= vh_bits_row_bit(lane.v()[p], r, p);
    if (by_bit != want) fail("vh_bits_row_bit", L, by_bit, want);
    for (int i = 0; i < L.ngroup; ++i) if (vh_bits_row_field(rec, L.goff[i], L.gbits[i]) != R.gv[i][r]) fail("vh_bits_row_field (group)", L, vh_bits_row_field(rec, L.goff[i], L.gbits[i]), R.gv[i][r]);
    for (int j = 0; j < L.nmetric; ++j) if (vh_bits_row_field(rec, L.mf[j].off, L.mf[j].nb) != R.mv[j][r]) fail("vh_bits_row_field (metric)", L, vh_bits_row_field(rec, L.mf[j].off, L.mf[j].nb), R.mv[j][r]);
    uint64_t gid = ~0ull;
    const bool in = vh_bits_row_gid(rec, L.ngroup, L.g, L.goff, L.gbits, &gid);
    if (in != ok) fail("vh_bits_row_gid: the range verdict", L, in, ok);
    if (ok && gid != id) fail("vh_bits_row_gid", L, gid, id);
    if (ok && gid >= L.G) fail("vh_bits_row_gid: an id beyond G", L, gid, L.G);
  }
}

static void records() {
  // the edges by hand: ONE plane; a field at plane 0; a field that ends at plane 31; all 32 planes
  for (int round = 0; round < 50; ++round) {
    check_records(make_layout(1, 0, 0, 1, 1), round % 2);
    check_records(make_layout(1, 0, 31, 1, 1), round % 2);
    check_records(make_layout(1, 1, 0, 32, 8), round % 4);
    check_records(make_layout(3, 2, 0, 32, 8), round % 4);
    check_records(make_layout(2, 1, 0, 17, 6), round % 4);      // from plane 0, noise above
    check_records(make_layout(2, 1, 15, 17, 6), round % 4);     // up to plane 31, noise below
  }
  for (int round = 0; round < 3000; ++round) {
    const int ngroup = 1 + (int)(rng() % 3), nmetric = (int)(rng() % 3);
    const uint32_t planes = (uint32_t)(ngroup + nmetric) + (uint32_t)(rng() % (uint64_t)(33 - ngroup - nmetric));      // nf .. 32
    const uint32_t first = (uint32_t)(rng() % (uint64_t)(33 - planes));
    check_records(make_layout(ngroup, nmetric, first, planes, 1 + (uint32_t)(rng() % 10)), round % 4);
  }
}

// ---- 2. the row sink's model against the loop's
struct Table {
  std::vector<uint64_t> state[2];
  std::vector<uint8_t> present;
  bool range_err = false;
  Table(const Layout& L, const int* sop) : present((size_t)L.G, 0) {
    for (int j = 0; j < L.nmetric; ++j) state[j].assign((size_t)L.G, sop_ident(sop[j]));
  }
};

static void sink_rows(const Layout& L, const int* sop, const std::vector<Lane>& wave, const uint32_t* mask, Table& T) {
  const int SLICE = 8;
  std::unique_ptr<uint16_t[]> q(new uint16_t[64 * SLICE]);      // exact size: an entry beyond it is the sanitizer's to find
  for (int k = 0; k < 32 / SLICE; ++k) {
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {      // the exclusive prefix, lane by lane; a lane's entries by ascending bit
      uint32_t mk = (mask[lane] >> (SLICE * k)) & ((1u << SLICE) - 1u);
      while (mk) {
        const uint32_t bit = (uint32_t)__builtin_ctz(mk);
        mk &= mk - 1u;
        q[total++] = (uint16_t)(lane << 5 | ((uint32_t)(SLICE * k) + bit));
      }
    }
    for (uint32_t i0 = 0; i0 < total; i0 += 64)
      for (uint32_t l = 0; l < 64 && i0 + l < total; ++l) {
        const uint32_t e = q[i0 + l], s = e >> 5, r = e & 31u;
        uint32_t rec = 0;
        for (uint32_t p = 0; p < 32; ++p) if ((L.need >> p) & 1u) rec |= vh_bits_row_bit(wave[s].v()[p], r, p);
        uint64_t gid = 0;
        if (!vh_bits_row_gid(rec, L.ngroup, L.g, L.goff, L.gbits, &gid)) { T.range_err = true; continue; }
        for (int j = 0; j < L.nmetric; ++j) state_update(&T.state[j][(size_t)gid], sop[j], vh_bits_row_field(rec, L.mf[j].off, L.mf[j].nb));
        T.present[(size_t)gid] = 1;
      }
  }
}

static void sink_groups(const Layout& L, const int* sop, const std::vector<Lane>& wave, const uint32_t* mask, Table& T) {
  uint32_t seen[64] = {};
  for (uint64_t g = 0; g < L.G; ++g) {
    uint32_t pat = 0;
    bool fits = true;
    for (int i = 0; i < L.ngroup; ++i) {      // (QueryBuild::choose_plane_agg: id g's digits -> the values its rows hold)
      const uint64_t value = L.g[i].lo + (g / L.g[i].stride) % L.g[i].extent;
      if (value >> L.gbits[i]) fits = false; else pat |= (uint32_t)value << L.goff[i];
    }
    uint32_t mg[64];
    bool any = false;
    for (int lane = 0; lane < 64; ++lane) {
      mg[lane] = fits ? mask[lane] & vh_bits_match(wave[(size_t)lane].v(), L.care, pat) : 0u;
      seen[lane] |= mg[lane];
      any = any || mg[lane];
    }
    if (!any) continue;
    for (int j = 0; j < L.nmetric; ++j) {
      uint64_t total = 0;
      bool empty;
      if (sop_is_add(sop[j])) for (int lane = 0; lane < 64; ++lane) total += vh_bits_sum_at(wave[(size_t)lane].v(), L.mf[j].off, L.mf[j].nb, mg[lane]);
      else if (sop_is_min(sop[j])) {
        uint32_t best = 0;      // the MAX of the complements
        for (int lane = 0; lane < 64; ++lane) { const uint32_t c = mg[lane] ? ~vh_bits_min_at(wave[(size_t)lane].v(), L.mf[j].off, L.mf[j].nb, mg[lane], &empty) : 0u; if (c > best) best = c; }
        total = (uint32_t)~best;
      } else {
        uint32_t best = 0;
        for (int lane = 0; lane < 64; ++lane) { const uint32_t c = mg[lane] ? vh_bits_max_at(wave[(size_t)lane].v(), L.mf[j].off, L.mf[j].nb, mg[lane], &empty) : 0u; if (c > best) best = c; }
        total = best;
      }
      state_update(&T.state[j][(size_t)g], sop[j], total);
    }
    T.present[(size_t)g] = 1;
  }
  for (int lane = 0; lane < 64; ++lane) if (mask[lane] & ~seen[lane]) T.range_err = true;
}

static void sinks() {
  for (int round = 0; round < 1500; ++round) {
    Layout L;
    do {
      const int ngroup = 1 + (int)(rng() % 3), nmetric = 1 + (int)(rng() % 2);
      const uint32_t planes = (uint32_t)(ngroup + nmetric) + (uint32_t)(rng() % (uint64_t)(33 - ngroup - nmetric));
      const uint32_t first = (uint32_t)(rng() % (uint64_t)(33 - planes));
      L = make_layout(ngroup, nmetric, first, planes, 1 + (uint32_t)(rng() % 4));
    } while (L.G > 64);
    const int sop[2] = {round % NSOP, (round / NSOP + 3) % NSOP};
    const int kind = round % 4;                                    // 0: values anywhere (range errors), 1: all within, 2: ONE id and top values, 3: zeros
    std::vector<Lane> wave(64);
    Rows R;
    uint32_t mask[64];
    const int shape = (round / 4) % 6;
    for (int lane = 0; lane < 64; ++lane) {
      fill_lane(L, wave[(size_t)lane], R, kind);
      uint32_t m = (uint32_t)rng();
      if (shape == 1) m = ~0u;                                     // all 2048 rows: every slice fills the queue
      if (shape == 2) m = lane == 0 ? 1u : 0u;                     // ONE survivor: bit 0 of lane 0
      if (shape == 3) m = lane == 63 ? 1u << 31 : 0u;              // ONE survivor: bit 31 of lane 63
      if (shape == 4) m = lane == 7 ? (1u << 9 | 1u << 10) : 1u << 9;      // 65 survivors in one slice: a second drain group of one
      if (shape == 5) m &= (uint32_t)rng() & (uint32_t)rng();      // sparse
      mask[lane] = m;
    }
    Table a(L, sop), b(L, sop);
    sink_rows(L, sop, wave, mask, a);
    sink_groups(L, sop, wave, mask, b);
    ++g_checks;
    if (a.range_err != b.range_err) fail("the sinks' range verdicts differ", L, a.range_err, b.range_err);
    if (a.present != b.present) fail("the sinks' presence bytes differ", L, 0, 0);
    for (int j = 0; j < L.nmetric; ++j)
      for (uint64_t g = 0; g < L.G; ++g)
        if (a.state[j][(size_t)g] != b.state[j][(size_t)g]) { printf("(%s, id %llu) ", kSopName[sop[j]], (unsigned long long)g); fail("the sinks' states differ", L, a.state[j][(size_t)g], b.state[j][(size_t)g]); }
  }
  // a u32 sum that wraps: 64 words of 32 rows of 0xFFFFFFF0 + r in ONE id, many waves over
  Layout L = make_layout(1, 1, 0, 32, 1);
  while (L.mf[0].nb < 31) L = make_layout(1, 1, 0, 32, 1);
  const int sop[2] = {ADD32, ADD32};
  Table a(L, sop), b(L, sop);
  uint64_t exact = 0;
  for (int w = 0; w < 40; ++w) {
    std::vector<Lane> wave(64);
    Rows R;
    uint32_t mask[64];
    for (int lane = 0; lane < 64; ++lane) {
      fill_lane(L, wave[(size_t)lane], R, 2);
      mask[lane] = ~0u;
      for (int r = 0; r < 32; ++r) exact += R.mv[0][r];
    }
    sink_rows(L, sop, wave, mask, a);
    sink_groups(L, sop, wave, mask, b);
  }
  ++g_checks;
  if (exact <= 0xFFFFFFFFull) fail("wrap: the total does not pass 2^32", L, exact, 0);
  if (a.state[0][0] != (uint32_t)exact || b.state[0][0] != (uint32_t)exact) fail("wrap", L, a.state[0][0], (uint32_t)exact);
}

int main() {
  records();
  sinks();
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("ok: %ld checks\n", g_checks);
  return 0;
}
