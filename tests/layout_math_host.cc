// layout_math_host.cc — viyadb_amd/csrc/vhh_layout_math.h as plain C++ (tests/test_layout_math_host.py compiles this with
// -fsanitize=address,undefined and runs it; the library is not loaded).
//
// THE JOB CUTTER against brute force. A model table of 3 segments keeps, per row, the epoch of the last sync that touched it; a layout that
// was current at epoch A is stale in exactly the rows whose epoch is above A. For seeded random journals (with and without a floor, layouts
// that are new, behind the floor, at the floor, ahead of it, and that never held a segment) the jobs must hold every stale row below the
// row limit exactly once, start on multiples of 256, hold at most VH_JOB_ROWS rows, not overlap, end at or below the row limit and carry the
// segment's rows; where the journal reaches back to the layout, every 256 rows a job covers hold a stale row (nothing is re-derived for
// nothing). Widened to tiles, the jobs are exactly the tiles that hold a stale row, each once. Then the edge cases, spelled out.
// THE WIDTH FUNCTIONS against a table recorded from the four functions they replaced (column_stored_width, pack_describe's bit fields,
// predpack_bits_for, narrow_width_for) before those were rewritten on top of this header: every element type at the empty range, [0, 0], the
// largest value of 8, 16, 32 and 63 bits and one more, and — signed types — negative lower bounds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "vhh_layout_math.h"

static const uint32_t NSEG = 3, SEG_ROWS = 40000;

struct Model {
  std::vector<VhChange> journal;             // what the table still holds
  uint64_t floor = 0, epoch = 0;
  std::vector<uint64_t> seg_mod = std::vector<uint64_t>(NSEG, 0), seg_rows = std::vector<uint64_t>(NSEG, 0);
  std::vector<std::vector<uint64_t>> row_epoch = std::vector<std::vector<uint64_t>>(NSEG, std::vector<uint64_t>(SEG_ROWS, 0));
  std::vector<std::vector<uint64_t>> mod_at;  // mod_at[e][s]: seg_mod[s] after epoch e
  Model() { mod_at.push_back(seg_mod); }
  void sync(uint32_t seg, uint32_t first, uint32_t last) {
    ++epoch;
    seg_mod[seg] = epoch;
    seg_rows[seg] = std::max<uint64_t>(seg_rows[seg], last);
    for (uint32_t r = first; r < last; ++r) row_epoch[seg][r] = epoch;
    journal.push_back(VhChange{epoch, seg, first, last});
    mod_at.push_back(seg_mod);
  }
  void trim(size_t drop) { floor = journal[drop - 1].epoch; journal.erase(journal.begin(), journal.begin() + (long)drop); }
  VhCutTable table(uint32_t nseg = NSEG) const { return VhCutTable{journal.data(), journal.size(), floor, seg_mod.data(), seg_rows.data(), nseg}; }
};

// The properties every list of jobs has; `reaches`: the journal reaches back to the layout (ranges, not whole segments).
static bool check_jobs(const Model& m, const std::vector<uint64_t>& lmod, uint64_t applied, uint64_t row_limit, bool tiles, bool reaches, const std::vector<VhJob>& jobs, const char* what) {
  std::vector<std::vector<uint8_t>> cover(NSEG, std::vector<uint8_t>(SEG_ROWS + 4096, 0));
  for (const VhJob& j : jobs) {
    if (j.seg >= NSEG || j.count == 0 || j.seg_rows != m.seg_rows[j.seg]) { printf("%s: job of segment %u, %u rows, seg_rows %u\n", what, j.seg, j.count, j.seg_rows); return false; }
    if (tiles) {
      if (j.first % VH_GROUP_TILE || j.count != VH_GROUP_TILE || j.first >= row_limit) { printf("%s: tile job [%u, +%u)\n", what, j.first, j.count); return false; }
    } else if (j.first % 256u || j.count > VH_JOB_ROWS || (uint64_t)j.first + j.count > row_limit) { printf("%s: job [%u, +%u) against the limit %llu\n", what, j.first, j.count, (unsigned long long)row_limit); return false; }
    for (uint32_t r = j.first; r < j.first + j.count; ++r) if (cover[j.seg][r]++) { printf("%s: row %u of segment %u in two jobs\n", what, r, j.seg); return false; }
  }
  for (uint32_t s = 0; s < NSEG; ++s) {
    // stale: the row changed after the layout was current — or the layout never held the segment's stamp (whole segments are judged by it)
    for (uint32_t r = 0; r < SEG_ROWS && r < row_limit; ++r)
      if (m.row_epoch[s][r] > applied && s < lmod.size() && !cover[s][r]) { printf("%s: stale row %u of segment %u (epoch %llu > %llu) in no job\n", what, r, s, (unsigned long long)m.row_epoch[s][r], (unsigned long long)applied); return false; }
    if (!reaches) continue;
    const uint32_t unit = tiles ? VH_GROUP_TILE : 256u;
    for (uint32_t b = 0; b < SEG_ROWS + 4096; b += unit) {
      if (!cover[s][b]) continue;
      bool any = lmod[s] == 0;          // (a segment the layout never held is derived whole)
      for (uint32_t r = b; r < b + unit && r < SEG_ROWS; ++r) any |= m.row_epoch[s][r] > applied;
      if (!any) { printf("%s: rows [%u, +%u) of segment %u re-derived for nothing\n", what, b, unit, s); return false; }
    }
  }
  return true;
}

static bool random_journals(uint32_t seed) {
  std::mt19937 rng(seed);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  Model m;
  const uint32_t rows[NSEG] = {pick(1, SEG_ROWS), pick(1, SEG_ROWS), SEG_ROWS};
  for (uint32_t s = 0; s < NSEG; ++s) m.sync(s, 0, rows[s]);                 // the load
  const uint32_t nsync = pick(1, 60);
  for (uint32_t i = 0; i < nsync; ++i) {
    const uint32_t s = pick(0, NSEG - 1), kind = pick(0, 9);
    uint32_t first = pick(0, rows[s] - 1), n = kind == 0 ? pick(1, rows[s]) : kind < 4 ? pick(1, 3000) : pick(1, 40);
    if (kind == 1) first = first / 256u * 256u;                                // ranges that start, or end, on a boundary
    uint32_t last = std::min(first + n, rows[s]);
    if (kind == 2 && last / 256u * 256u > first) last = last / 256u * 256u;
    m.sync(s, first, last);
  }
  if (seed % 3 == 1 && m.journal.size() > 4) m.trim(m.journal.size() / 2);
  const uint64_t limits[2] = {(SEG_ROWS + 255ull) / 256 * 256, (SEG_ROWS + 63ull) / 64 * 64};
  for (uint64_t applied = 0; applied <= m.epoch; ++applied) {
    std::vector<uint64_t> lmod = m.mod_at[applied];
    if (applied == 0) lmod.assign(NSEG, 0);
    if (seed % 5 == 2 && applied) lmod[2] = 0;                                 // the table grew after the layout was made: it never held segment 2
    std::vector<uint64_t> short_mod(lmod.begin(), lmod.begin() + (seed % 7 == 3 ? 2 : NSEG));      // ... or has no stamp for it at all
    const bool reaches = applied != 0 && applied >= m.floor;
    for (int tiles = 0; tiles < 2; ++tiles) {
      const uint64_t limit = tiles ? limits[0] : limits[applied & 1];
      std::vector<VhJob> jobs;
      // stale by the model: where a stamp is 0 the whole segment counts, whatever the rows' epochs say
      vh_cut_jobs(m.table(), VhCutLayout{short_mod.data(), short_mod.size(), applied, limit}, tiles != 0, &jobs);
      Model view = m;
      for (uint32_t s = 0; s < NSEG; ++s) if (s < short_mod.size() && short_mod[s] == 0 && m.seg_mod[s] > applied) for (auto& e : view.row_epoch[s]) e = std::max<uint64_t>(e, applied + 1);
      char what[96];
      snprintf(what, sizeof(what), "seed %u applied %llu%s", seed, (unsigned long long)applied, tiles ? " tiles" : "");
      if (!check_jobs(view, short_mod, applied, limit, tiles != 0, reaches, jobs, what)) return false;
    }
  }
  return true;
}

// ---- the edge cases, spelled out
static std::vector<VhJob> cut(const Model& m, const std::vector<uint64_t>& lmod, uint64_t applied, uint64_t limit, bool tiles = false, uint32_t nseg = NSEG) {
  std::vector<VhJob> jobs;
  vh_cut_jobs(m.table(nseg), VhCutLayout{lmod.data(), lmod.size(), applied, limit}, tiles, &jobs);
  return jobs;
}
static bool same(const std::vector<VhJob>& got, const std::vector<VhJob>& want, const char* what) {
  bool ok = got.size() == want.size();
  for (size_t i = 0; ok && i < got.size(); ++i) ok = got[i].seg == want[i].seg && got[i].first == want[i].first && got[i].count == want[i].count && got[i].seg_rows == want[i].seg_rows;
  if (!ok) { printf("%s: got", what); for (const VhJob& j : got) printf(" (%u: %u +%u of %u)", j.seg, j.first, j.count, j.seg_rows); printf("\n"); }
  return ok;
}
static const uint64_t LIMIT = (SEG_ROWS + 255ull) / 256 * 256;      // 40192
static Model loaded() { Model m; for (uint32_t s = 0; s < NSEG; ++s) m.sync(s, 0, SEG_ROWS); return m; }      // epochs 1..3

static bool edge_boundaries() {
  Model m = loaded();
  m.sync(0, 10, 512);       // ends exactly on a boundary
  m.sync(1, 10, 513);       // ... and one past it
  return same(cut(m, m.mod_at[3], 3, LIMIT), {{0, 0, 512, SEG_ROWS}, {1, 0, 768, SEG_ROWS}}, "boundaries");
}
static bool edge_touch_overlap() {
  Model m = loaded();
  m.sync(0, 0, 256); m.sync(0, 256, 300);            // touch
  m.sync(1, 100, 600); m.sync(1, 500, 900);          // overlap
  m.sync(2, 0, 10); m.sync(2, 600, 610);             // neither: two jobs
  return same(cut(m, m.mod_at[3], 3, LIMIT), {{0, 0, 512, SEG_ROWS}, {1, 0, 1024, SEG_ROWS}, {2, 0, 256, SEG_ROWS}, {2, 512, 256, SEG_ROWS}}, "touching and overlapping ranges");
}
static bool edge_long_range() {
  Model m = loaded();
  m.sync(1, 0, SEG_ROWS);
  return same(cut(m, m.mod_at[3], 3, LIMIT), {{1, 0, VH_JOB_ROWS, SEG_ROWS}, {1, VH_JOB_ROWS, VH_JOB_ROWS, SEG_ROWS}, {1, 2 * VH_JOB_ROWS, (uint32_t)(LIMIT - 2 * VH_JOB_ROWS), SEG_ROWS}}, "a range longer than VH_JOB_ROWS") &&
         same(cut(m, m.mod_at[3], 3, SEG_ROWS), {{1, 0, VH_JOB_ROWS, SEG_ROWS}, {1, VH_JOB_ROWS, VH_JOB_ROWS, SEG_ROWS}, {1, 2 * VH_JOB_ROWS, SEG_ROWS - 2 * VH_JOB_ROWS, SEG_ROWS}}, "... under a limit padded to 64");
}
static bool edge_never_held() {
  Model m = loaded();
  m.sync(2, 5, 6);
  std::vector<uint64_t> lmod = m.mod_at[3];
  lmod[2] = 0;
  return same(cut(m, lmod, 3, LIMIT), {{2, 0, VH_JOB_ROWS, SEG_ROWS}, {2, VH_JOB_ROWS, VH_JOB_ROWS, SEG_ROWS}, {2, 2 * VH_JOB_ROWS, (uint32_t)(LIMIT - 2 * VH_JOB_ROWS), SEG_ROWS}}, "a segment the layout never held");
}
static bool edge_new_and_behind_the_floor() {
  Model m = loaded();
  for (int i = 0; i < 6; ++i) m.sync(0, 100u * (uint32_t)i, 100u * (uint32_t)i + 7);      // epochs 4..9, all in segment 0
  const std::vector<VhJob> seg0 = {{0, 0, VH_JOB_ROWS, SEG_ROWS}, {0, VH_JOB_ROWS, VH_JOB_ROWS, SEG_ROWS}, {0, 2 * VH_JOB_ROWS, (uint32_t)(LIMIT - 2 * VH_JOB_ROWS), SEG_ROWS}};
  std::vector<VhJob> all;
  for (uint32_t s = 0; s < NSEG; ++s) for (VhJob j : seg0) { j.seg = s; all.push_back(j); }
  bool ok = same(cut(m, std::vector<uint64_t>(NSEG, 0), 0, LIMIT), all, "applied_epoch 0: every segment");
  ok = ok && same(cut(m, m.mod_at[5], 0, LIMIT), seg0, "applied_epoch 0 with stamps: only the segment whose stamp differs");
  m.trim(6);                                          // the floor is epoch 6
  ok = ok && m.floor == 6 && same(cut(m, m.mod_at[5], 5, LIMIT), seg0, "behind the floor: whole segments, only those whose stamp differs");
  ok = ok && same(cut(m, m.mod_at[6], 6, LIMIT), {{0, 256, 256, SEG_ROWS}}, "exactly at the floor: the journal still reaches it");      // epochs 7..9: rows 300.., 400.., 500.. of 256..511
  ok = ok && same(cut(m, m.mod_at[9], 9, LIMIT), {}, "current: nothing");
  return ok;
}
static bool edge_beyond_nseg() {
  Model m = loaded();
  m.sync(2, 0, 100);
  m.sync(1, 0, 100);
  bool ok = same(cut(m, m.mod_at[3], 3, LIMIT, false, 2), {{1, 0, 256, SEG_ROWS}}, "an entry beyond nseg");
  std::vector<uint64_t> two(m.mod_at[3].begin(), m.mod_at[3].begin() + 2);
  return ok && same(cut(m, two, 3, LIMIT), {{1, 0, 256, SEG_ROWS}}, "an entry beyond the layout's stamps");
}
static bool edge_partial_tile() {
  Model m;
  for (uint32_t s = 0; s < NSEG; ++s) m.sync(s, 0, 5000);
  m.sync(1, 4999, 5000);
  m.sync(2, 2047, 2049);                             // a range across two tiles
  m.sync(2, 100, 101);                               // ... and a second one in the first of them
  const uint64_t limit = (5000 + 255) / 256 * 256;
  return same(cut(m, m.mod_at[3], 3, limit, true), {{1, 4096, VH_GROUP_TILE, 5000}, {2, 0, VH_GROUP_TILE, 5000}, {2, 2048, VH_GROUP_TILE, 5000}}, "the last, partial tile of a 5 000-row segment") &&
         same(cut(m, std::vector<uint64_t>(NSEG, 0), 0, limit, true).size() == 9 ? std::vector<VhJob>{} : std::vector<VhJob>{{9, 9, 9, 9}}, {}, "a new grouped form: three tiles a segment");
}

// ---- the width functions
struct In { int64_t a; uint64_t b; };
static const In INPUTS[] = {{0, 0}, {0, 0}, {0, 255}, {0, 256}, {0, 65535}, {0, 65536}, {0, 0xFFFFFFFFull}, {0, 0x100000000ull}, {0, 0x7FFFFFFFFFFFFFFFull}, {0, 0x8000000000000000ull},
                            {-1, 100}, {-129, 100}, {-40000, 40000}};      // [0]: the empty range; [9]: unsigned and floating-point types only; [10..12]: signed types only
// {element type, input, stored bytes, bits of a record's field (-1: bit fields refused), bits of a predicate field (0: none), narrow width}
static const int WANT[][6] = {
  {0,  0, 1,  1,  0, 0}, {0,  1, 1,  1,  1, 0}, {0,  2, 1,  8,  8, 0}, {0,  3, 1,  9,  9, 0}, {0,  4, 1, 16, 16, 0}, {0,  5, 1, 17, 17, 0},
  {0,  6, 1, 32, 32, 0}, {0,  7, 1, 33, 33, 0}, {0,  8, 1, 63, 63, 0}, {0,  9, 1, 64, 64, 0}, {1,  0, 1,  1,  0, 0}, {1,  1, 1,  1,  1, 0},
  {1,  2, 1,  8,  8, 0}, {1,  3, 2,  9,  9, 0}, {1,  4, 2, 16, 16, 0}, {1,  5, 2, 17, 17, 0}, {1,  6, 2, 32, 32, 0}, {1,  7, 2, 33, 33, 0},
  {1,  8, 2, 63, 63, 0}, {1,  9, 2, 64, 64, 0}, {2,  0, 1,  1,  0, 0}, {2,  1, 1,  1,  1, 1}, {2,  2, 1,  8,  8, 1}, {2,  3, 2,  9,  9, 2},
  {2,  4, 2, 16, 16, 2}, {2,  5, 4, 17, 17, 0}, {2,  6, 4, 32, 32, 0}, {2,  7, 4, 33, 33, 0}, {2,  8, 4, 63, 63, 0}, {2,  9, 4, 64, 64, 0},
  {3,  0, 1,  1,  0, 0}, {3,  1, 1,  1,  1, 0}, {3,  2, 1,  8,  8, 0}, {3,  3, 2,  9,  9, 0}, {3,  4, 2, 16, 16, 0}, {3,  5, 4, 17, 17, 0},
  {3,  6, 4, 32, 32, 0}, {3,  7, 8, 33, 33, 0}, {3,  8, 8, 63, 63, 0}, {3,  9, 8, 64, 64, 0}, {4,  0, 1,  1,  0, 0}, {4,  1, 1,  1,  1, 0},
  {4,  2, 1,  8,  8, 0}, {4,  3, 1,  9,  9, 0}, {4,  4, 1, 16, 16, 0}, {4,  5, 1, 17, 17, 0}, {4,  6, 1, 32, 32, 0}, {4,  7, 1, 33, 33, 0},
  {4,  8, 1, 63, 63, 0}, {4, 10, 1, -1,  0, 0}, {4, 11, 1, -1,  0, 0}, {4, 12, 1, -1,  0, 0}, {5,  0, 1,  1,  0, 0}, {5,  1, 1,  1,  1, 0},
  {5,  2, 2,  8,  8, 0}, {5,  3, 2,  9,  9, 0}, {5,  4, 2, 16, 16, 0}, {5,  5, 2, 17, 17, 0}, {5,  6, 2, 32, 32, 0}, {5,  7, 2, 33, 33, 0},
  {5,  8, 2, 63, 63, 0}, {5, 10, 1, -1,  0, 0}, {5, 11, 2, -1,  0, 0}, {5, 12, 2, -1,  0, 0}, {6,  0, 1,  1,  0, 0}, {6,  1, 1,  1,  1, 0},
  {6,  2, 2,  8,  8, 0}, {6,  3, 2,  9,  9, 0}, {6,  4, 4, 16, 16, 0}, {6,  5, 4, 17, 17, 0}, {6,  6, 4, 32, 32, 0}, {6,  7, 4, 33, 33, 0},
  {6,  8, 4, 63, 63, 0}, {6, 10, 1, -1,  0, 0}, {6, 11, 2, -1,  0, 0}, {6, 12, 4, -1,  0, 0}, {7,  0, 1,  1,  0, 0}, {7,  1, 1,  1,  1, 0},
  {7,  2, 2,  8,  8, 0}, {7,  3, 2,  9,  9, 0}, {7,  4, 4, 16, 16, 0}, {7,  5, 4, 17, 17, 0}, {7,  6, 8, 32, 32, 0}, {7,  7, 8, 33, 33, 0},
  {7,  8, 8, 63, 63, 0}, {7, 10, 1, -1,  0, 0}, {7, 11, 2, -1,  0, 0}, {7, 12, 4, -1,  0, 0}, {8,  0, 4, -1,  0, 0}, {8,  1, 4, -1,  0, 0},
  {8,  2, 4, -1,  0, 0}, {8,  3, 4, -1,  0, 0}, {8,  4, 4, -1,  0, 0}, {8,  5, 4, -1,  0, 0}, {8,  6, 4, -1,  0, 0}, {8,  7, 4, -1,  0, 0},
  {8,  8, 4, -1,  0, 0}, {8,  9, 4, -1,  0, 0}, {9,  0, 8, -1,  0, 0}, {9,  1, 8, -1,  0, 0}, {9,  2, 8, -1,  0, 0}, {9,  3, 8, -1,  0, 0},
  {9,  4, 8, -1,  0, 0}, {9,  5, 8, -1,  0, 0}, {9,  6, 8, -1,  0, 0}, {9,  7, 8, -1,  0, 0}, {9,  8, 8, -1,  0, 0}, {9,  9, 8, -1,  0, 0},
};
static const int ESIZE[10] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8};
static bool widths() {
  size_t n = 0;
  for (const auto& w : WANT) {
    const int e = w[0], i = w[1];
    VhRange r;
    if (i > 0) {
      if (vh_elem_signed(e)) { r.lo = (uint64_t)INPUTS[i].a ^ (1ull << 63); r.hi = INPUTS[i].b ^ (1ull << 63); }
      else if (e == VH_F32) { r.lo = (uint32_t)INPUTS[i].a | 0x80000000u; r.hi = (uint32_t)INPUTS[i].b | 0x80000000u; }
      else if (e == VH_F64) { r.lo = (uint64_t)INPUTS[i].a | (1ull << 63); r.hi = INPUTS[i].b | (1ull << 63); }
      else { r.lo = (uint64_t)INPUTS[i].a; r.hi = INPUTS[i].b; }
    }
    if ((i == 0) != r.empty()) { printf("widths: input %d of type %d: empty() says %d\n", i, e, (int)r.empty()); return false; }
    const int stored = vh_range_stored_bytes(e, ESIZE[e], r);
    const int rec_bits = vh_range_bits(e, r.empty() ? vh_range_of_zero(e) : r);      // (a record projection takes "no rows yet" as the value 0)
    const int pred_bits = vh_range_bits(e, r), narrow = vh_range_narrow_width(e, r);
    if (stored != w[2] || (rec_bits ? rec_bits : -1) != w[3] || pred_bits != w[4] || narrow != w[5]) {
      printf("widths: type %d input %d: stored %d (%d), record bits %d (%d), predicate bits %d (%d), narrow %d (%d)\n", e, i, stored, w[2], rec_bits ? rec_bits : -1, w[3], pred_bits, w[4], narrow, w[5]);
      return false;
    }
    ++n;
  }
  if (n != 108) { printf("widths: %zu rows\n", n); return false; }
  // the fold: empty segments add nothing; bitsets have no bit field
  VhSegStat st[4];
  st[1].lo = 7; st[1].hi = 9; st[3].lo = 2; st[3].hi = 8;
  const VhRange f = vh_range_over(st, 4), none = vh_range_over(st, 1);
  if (f.lo != 2 || f.hi != 9 || !none.empty() || !vh_range_over(st, 0).empty()) { printf("widths: the fold\n"); return false; }
  if (vh_range_bits(VH_BITSET32, f) || vh_range_bits(VH_BITSET64, f)) { printf("widths: a bitset as a bit field\n"); return false; }
  return true;
}

int main() {
  int bad = 0;
  auto say = [&](const char* name, bool ok) { printf("%s: %s\n", name, ok ? "ok" : "FAILED"); bad += !ok; };
  for (uint32_t seed = 0; seed < 24; ++seed) { char name[32]; snprintf(name, sizeof(name), "random journals, seed %u", seed); say(name, random_journals(seed)); }
  say("ranges that end on a boundary and one past it", edge_boundaries());
  say("ranges that touch and overlap", edge_touch_overlap());
  say("a range longer than VH_JOB_ROWS", edge_long_range());
  say("a segment the layout never held", edge_never_held());
  say("new, behind the floor, at the floor", edge_new_and_behind_the_floor());
  say("entries beyond nseg", edge_beyond_nseg());
  say("tiles", edge_partial_tile());
  say("widths", widths());
  return bad ? 1 : 0;
}
