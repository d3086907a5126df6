// vhh_table.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// the table mirror: column arenas, per-segment stats, execution contexts (stream, scratch, staging, events), the derived layouts' types, their
// arenas' ledger (buf_alloc / buf_free) and enumeration (derived_each); vh_table_create / vh_table_destroy.
// -------------------------------------------------------------------- table
struct VhColumn {
  int kind = 0, elem = 0, esize = 0;
  char* base = nullptr;     // arena: cap_seg x stride bytes (+ tail pad)
  uint64_t stride = 0;      // bytes between segments
  // bitset CSR mirrors (one pair per segment)
  std::vector<uint64_t*> bs_offsets;
  std::vector<void*> bs_values;
  std::vector<uint64_t> bs_nvalues;
  std::vector<uint32_t*> bs_offsets32;  // the same offsets as 32-bit words when the segment holds < 2^32 ids (nullptr otherwise): what the compiled
                                        // scan of the hashed partitioning reads — 4 instead of 8 bytes per row of a stream every query of the set takes in full
  std::vector<uint64_t> bs_maxid;      // an upper bound of the segment's ids (what the packed tuples of the hashed partitioning are sized from)
};
// Execution context: everything ONE in-flight query needs besides the table's columns — a stream, device scratch,
// pinned staging, events. A table keeps a pool of them; a vh_result owns one from launch until vh_result_free, so
// queries of different threads on one table overlap on the device (the reference's read_pool runs queries of one table
// concurrently: src/db/database.cc:28-34, src/server/http/service.cc:119) and a handle's device state and host view are
// never reused under it.
struct VhExec {
  hipStream_t own_stream = nullptr;
  char* scratch = nullptr; size_t scratch_bytes = 0;
  uint32_t* h_segrows = nullptr; size_t h_segrows_cap = 0;
  unsigned long long* h_counters = nullptr;     // pinned: 16 words of counters + 64 words for a big result's header
  char* d_sample = nullptr; size_t d_sample_bytes = 0;   // selectivity probe: counters + presence + seg rows
  VhSetDev probe_sets[VH_MAX_SETS] = {};                 // ... and the set descriptors its upload reads (the source of an asynchronous copy outlives any early return)
  char* h_out[2] = {nullptr, nullptr}; size_t h_out_bytes[2] = {0, 0}; int h_out_next = 0;  // pinned result staging (two alternate: a
                                                                                            // zero-copy view outlives vh_result_free until the second-next query)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // streamed delivery of big results (hashed partitioning, VhHpArgs::nchunks): the aggregation's chunk launches alternate between the query's
  // stream and `aux` (the tail of one chunk overlaps the start of the next), finished chunks leave on `copy`; created on first use
  hipStream_t aux = nullptr, copy = nullptr;
  hipEvent_t ev_fork = nullptr, ev_chunk[VH_HP_CHUNKS] = {};
  unsigned long long* h_chunk = nullptr;        // pinned: rows of chunk c, written by publish_count_kernel
  // the LEAD context of a fused group of a batch (vh_query_agg_batch): the members' array as scan_agg_planes_batch_kernel reads it, staged in
  // pinned memory and copied to the device on this context's stream, and the events around the fused launch; created on first use (exec_batch).
  // Not in `scratch`, which ensure_scratch may move, and not per table: two threads may run batches on one table at once, and the kernel
  // runs after the table's lock is released.
  VhBatchMember* h_batch = nullptr; VhBatchMember* d_batch = nullptr;
  hipEvent_t ev_batch[2] = {nullptr, nullptr};
  bool busy = false;
  // an externally owned stream (vh_set_stream) carries all work; otherwise every context has its own
  hipStream_t stream() const { return g_ctx.stream != g_ctx.own_stream ? g_ctx.stream : own_stream; }
};

// A per-segment arena of a derived layout: `stride` bytes per segment for as many segments as it was made for, and a tail pad. The pad lives
// in bytes() alone; `held` is what alloc() took and the table's byte ledger (vh_table::device_bytes) was charged — what free() gives back.
struct VhBuf {
  char* ptr = nullptr; uint64_t stride = 0; size_t held = 0;
  static size_t bytes(uint32_t cap_seg, uint64_t stride) { return (size_t)cap_seg * stride + 256; }
  size_t bytes(uint32_t cap_seg) const { return bytes(cap_seg, stride); }
};
// What every derived layout keeps about itself, and all the refresh path (derived_refresh, vhh_derived.h) needs to know of one.
struct VhLayout {
  uint32_t cap_seg = 0;             // segments its arenas have room for
  std::vector<uint64_t> seg_mod;    // value of vh_table::seg_mod[s] the segment was derived at (0: never)
  uint64_t applied_epoch = 0;       // every change of the table's journal up to this epoch is in the arenas
  uint64_t serial = 0;              // vh_table::layout_serial when it was built: which layout this is (derived_settle; addresses get reused). A grouped form carries its projection's
  bool automatic = false;
  // Lifetime under the table's byte budget (derived_make_room, vhh_derived.h). A grouped form is accounted with its projection: these stay 0 in it.
  bool pinned = false;              // never evicted: built by an explicit call, read by a prepared plan, or pinned through vh_table_layout_pin
  uint64_t uses = 0;                // plans that read the layout
  uint64_t last_use = 0;            // vh_table::use_tick at the last of them (0: never)
  uint64_t held_tick = 0;           // vh_table::use_tick of the last plan that took a pointer into the arenas, counted in `uses` or not (a quiet plan's is not): that plan evicts nothing it holds
};
// The GROUPED form of a 4-byte bit-record projection (vh_grouped.h, group_bits_kernel): a second copy of the records in which every tile of
// 2048 rows is stable-sorted by the field a bit-sliced predicate projection keeps of column `col` (`bits` bits, at most VH_GROUP_MAX_BITS),
// and the tiles' headers. It belongs to its projection (same stride, dropped and grown with it) but follows the journal by itself: its jobs are
// whole tiles. A plan reads it only while it is as current as the planes whose bits give the places (QueryBuild::choose_grouped).
struct VhGrouped : VhLayout {
  int col = -1; uint32_t bits = 0;
  VhBuf rec;                        // records: the projection's stride
  VhBuf hdr;                        // headers: (2 << bits) bytes per tile
  // CLUSTERED predicate planes (vh_grouped.h): the other columns' bits of the bit-sliced predicate projection `pp_serial`, in the tiles' grouped
  // order, word-major, G dwords a word. Written by the launch that writes records and headers (one epoch, one refresh path). The fields the
  // launch reads are copied from the projection when the arena is made; a plan pairs the two by serial, so a projection that was dropped or
  // re-described never meets planes of other fields. planes.ptr == nullptr: none (no room, or no projection yet) — the grouped records alone
  // answer; planes.stride, G and pp_serial are then 0.
  VhBuf planes; uint32_t G = 0;
  uint64_t pp_serial = 0; uint32_t goff = 0;
  std::vector<int> pp_cols; std::vector<uint8_t> pp_bitoff, pp_bitw;
  // The SUB-SORTED form (vh_grouped.h): every tile ordered by (value of `col`, field of `sub_col`, row), 64 boundary keys per tile behind the
  // segment's headers in `hdr` (whose stride grows by them). sub_col == -1: the form in row order inside a run, byte for byte as it ever was.
  // The sub key is taken from the clustered planes' field word (sub_off: the field's bit there), so a sub-sorted form always has its planes:
  // a place follows from no row-order formula any more, and a form that loses its planes is dropped whole (grouped_no_planes).
  int sub_col = -1; uint32_t sub_bits = 0, sub_off = 0;
};
// Payload projection (vh_table_pack): a row-major copy of a few columns, see pack_kernel.
struct VhPack : VhLayout {
  std::vector<int> cols;            // table column indices, in record order (widest first)
  std::vector<uint32_t> off;        // byte offset of each column inside a record
  std::vector<uint8_t> width;       // bytes the column's values take in a record (compressed: fewer than its element size)
  bool compressed = false;          // integer columns stored at the width their values need; only the per-query compiled kernels read these
  // BIT-FIELD records (round 4; compressed projections whose columns are all non-negative integers): every column at the BITS its values
  // need, packed into one 4- or 8-byte word — C3's (d0 10 bits, d1 7, m0 10, count 2) fits 4 bytes: 32 records per 128-byte line instead of 16
  bool bits = false;
  std::vector<uint8_t> bitoff, bitw;
  uint32_t rec_bytes = 0;           // power of two, 8..64 (bit-field records: 4 or 8)
  VhBuf rec;                        // the records: rows padded to 256 per segment
  std::unique_ptr<VhGrouped> grouped;      // its grouped form, if one was built (bit-field records of 4 bytes only)
  int col_index(int col) const { for (size_t i = 0; i < cols.size(); ++i) if (cols[i] == col) return (int)i; return -1; }
};
// Narrow copy of a predicate column (vh_table_narrow): an unsigned 32-bit column whose values fit 8 or 16 bits, kept a second time
// at that width. The register-resident scan kernels stream the copy instead of the arena — a predicate column is read in full by
// every query that filters on it, so its bytes are the floor of the scan (C3: 12 of 18.75 GB per query).
struct VhNarrow : VhLayout {
  int col = -1, width = 0;          // bytes per element: 1 or 2
  VhBuf copy;
};
// Bit-packed predicate projection (vh_table_predpack): the predicate columns of a query shape as bit fields of one word per row (each at
// the bits its recorded min / max need), kept as byte planes — what the per-query compiled scan streams instead of the columns or their
// narrow copies. C3: d2 (2 bits) + d3 (10) + d4 (10) = 22 bits -> a 2-byte and a 1-byte plane: 3 bytes per row instead of 5 (12 from the arenas).
struct VhPredPack : VhLayout {
  std::vector<int> cols;             // table columns, ascending
  std::vector<uint8_t> bitoff, bitw; // each column's field in the row word
  int nplanes = 0;
  int pwidth[4] = {}, ppos[4] = {};  // bytes per row of plane q, first bit of the word it holds
  VhBuf plane[4];
  // BIT-SLICED form: one plane per BIT of the word, one bit per row (32 rows = one 4-byte word of a plane); plane[0] is the whole arena,
  // plane[0].stride the bytes between segments, `pitch` the bytes between planes inside a segment; `bits` planes.
  bool sliced = false; uint32_t bits = 0; uint64_t pitch = 0;
  uint32_t bytes_per_row() const { uint32_t b = 0; for (int q = 0; q < nplanes; ++q) b += (uint32_t)pwidth[q]; return b; }
  uint32_t bits_per_row() const { return sliced ? bits : 8u * bytes_per_row(); }
};
// Pinned staging for the job lists the derived-layout kernels read (16 bytes a job; a list lives until its reader's stream has been waited
// for). The table owns one for the refreshes on the library's stream, the build worker one for its own stream; derived_upload fills both.
struct VhJobStage { char* buf = nullptr; size_t bytes = 0, used = 0; };
struct vh_table {
  std::vector<VhColumn> cols;
  uint64_t segment_rows = 0;
  uint64_t padded_rows = 0;
  uint32_t cap_seg = 0;
  uint32_t nseg = 0;
  std::vector<uint64_t> seg_rows;               // last synced row count
  std::vector<std::vector<VhSegStat>> stats;    // [col][seg]
  // per-query resources live in execution contexts (grow-only pool)
  std::vector<std::unique_ptr<VhExec>> execs;
  std::mutex pool_mu; std::condition_variable pool_cv;
  char* d_stats = nullptr; size_t d_stats_bytes = 0;      // vh_segment_sync*: min/max pass (its own buffer: a sync never touches a query's scratch)
  // vh_table_sync_batch: run descriptors and their result slots in ONE pinned block, a ring for small runs out of unregistered host memory,
  // and what of the last batch still has to be merged into `stats` (sync_resolve: the first planner — or sync — that comes after it waits)
  char* h_sync = nullptr; size_t h_sync_bytes = 0;
  char* h_stage = nullptr; size_t h_stage_bytes = 0;
  hipEvent_t sync_ev = nullptr;
  struct SyncPending { uint32_t col, seg, desc_first, desc_n; };
  std::vector<SyncPending> sync_pending;
  bool sync_inflight = false;
  uint64_t sync_batches = 0, sync_descs = 0, sync_bytes_pulled = 0, sync_bytes_staged = 0, sync_bytes_dma = 0;   // vh_table_sync_stats
  std::vector<uint16_t> ship_all, ship_metrics;          // vh_table_sync_batch: the columns an item ships (every fixed-width one / the metrics alone)
  std::vector<uint64_t> sync_rows_now;                   // ... and its scratch (rows mirrored per named segment while a batch is validated)
  std::map<std::string, uint64_t> groups_seen;           // group-column signature -> groups of the last query (hash sizing)
  std::set<std::string> hpart_hopeless;                  // group-column signatures whose hashed partitioning ended on the plain hash table (a group holding more ids than a range's LDS set takes in any number of passes): later queries of the shape start there
  std::set<std::string> part_clustered;                  // group-column signatures whose survivors came clustered under the piecewise writers: positional extent chunks (VhPlanDev::ext_waves) overflowed although the pool had room — later queries of the shape take their extents off the shared cursor at once
  std::map<std::string, std::pair<uint64_t, uint64_t>> sel_cache;   // filter signature + table state -> (passed, sampled) of the selectivity probe
  std::vector<std::unique_ptr<VhPack>> packs;
  std::vector<std::unique_ptr<VhNarrow>> narrows;
  std::vector<std::unique_ptr<VhPredPack>> predpacks;
  uint64_t layout_serial = 0;                             // the last serial given to a layout built
  std::map<std::string, uint32_t> ppred_seen;             // predicate column set -> compiled-kernel queries that filtered on it (automatic predicate projections)
  std::map<int, uint32_t> pred_seen;                     // column -> queries that filtered on it (automatic narrow copies)
  std::vector<uint64_t> seg_mod;                          // sync_epoch of the last change to a segment's columns
  // Derived layouts follow the arenas by ROW RANGE: every sync appends what it touched; a layout that was current at epoch e re-derives the
  // ranges journalled since — one launch over a list of jobs — instead of every segment whose stamp moved (an upsert batch dirties hundreds
  // of segments by a few rows each). Entries older than `journal_floor` were dropped: a layout behind that re-derives whole segments.
  std::vector<VhChange> journal; uint64_t journal_floor = 0;
  VhJobStage jobs;                                                       // pinned: the job lists of the refreshes enqueued since the stream was last waited for
  hipEvent_t derived_ev = nullptr; bool derived_pending = false;         // a refresh is enqueued on g_ctx.stream: the next query's stream waits for it
  unsigned int* d_packflag = nullptr;                      // pack_kernel's "a value outgrew its stored width" word
  std::map<std::string, uint32_t> gather_seen;            // payload column set -> low-selectivity queries seen (automatic packs)
  uint64_t sync_epoch = 0;   // bumped by every vh_segment_sync / generate: invalidates cached estimates
  std::mutex mu;             // table metadata, column arenas, projections, planner caches: held while a query is PLANNED and
                             // LAUNCHED and by every sync; not while a launched query runs or is read back
  uint64_t device_bytes = 0;
  // where the one-time work runs (vhh_build.h)
  int build_mode = VH_BUILD_INLINE;
  uint64_t inline_builds = 0;      // compiles and layout builds that ran inside a query of this table
  std::map<std::string, uint64_t> build_nothing;   // background layout jobs that found nothing to gain -> the sync epoch they judged at (not queued again before the table changes)
  uint64_t arena_gen = 0;          // bumped whenever table_grow replaces the column arenas: a layout job that enqueued its kernels against the old ones starts over
  // the derived layouts' byte budget (vhh_derived.h, derived_make_room)
  uint64_t use_tick = 0;           // bumped once per planned query: what VhLayout::last_use is stamped with
  uint64_t layout_budget = 0;      // bytes the derived layouts may hold together (0: no budget)
  uint64_t build_reserved = 0;     // arenas of the background job between its step (a) and its publish or drop: real bytes that device_bytes does not hold yet
  uint64_t evictions = 0, evicted_bytes = 0, declined = 0;      // layouts the budget evicted and their bytes; automatic builds it refused
};
static void build_arenas_moving(vh_table* t);              // (vhh_build.h) t->mu held: the arenas are about to be replaced — wait until no background job's kernels read them
static void build_cancel_table(vh_table* t, bool forget);  // (vhh_build.h) t->mu NOT held: drop the table's queued jobs, wait for the running one

static const uint32_t VH_MAX_SEGMENTS = 1u << 24;   // (segment << 32 | row) positions and u32 segment loops stay far from overflow
static bool is_dim(int kind) { return kind <= VH_DIM_BOOLEAN; }
static bool is_bitset_elem(int e) { return e == VH_BITSET32 || e == VH_BITSET64; }

static void trace_alloc(const char* what, const void* p, size_t bytes) {     // VH_TRACE_ALLOC=1: where the big buffers land (placement experiments)
  if (knobs().trace_alloc) fprintf(stderr, "vh alloc %s %p %zu\n", what, p, bytes);
}

// THE LEDGER of the derived layouts: these two are the only code that allocates or frees one of their arenas and the only code that moves
// vh_table::device_bytes for them (t == nullptr: the build worker's buffers before their layout belongs to a table — its publish step adds
// what they hold). soft: no room is the caller's to handle (VH_E_NOMEM, no message, no HIP error left behind).
static int buf_alloc(vh_table* t, VhBuf* b, uint32_t cap_seg, const char* what, bool soft = false) {
  const size_t bytes = b->bytes(cap_seg);
  if (soft) { if (hipMalloc(&b->ptr, bytes) != hipSuccess) { (void)hipGetLastError(); b->ptr = nullptr; return VH_E_NOMEM; } }
  else HIP_TRY(hipMalloc(&b->ptr, bytes));
  trace_alloc(what, b->ptr, bytes);
  b->held = bytes;
  if (t) t->device_bytes += bytes;
  return VH_OK;
}
static void buf_free(vh_table* t, VhBuf* b) {
  if (!b->ptr) return;
  (void)hipFree(b->ptr);
  if (t) t->device_bytes -= b->held;
  b->ptr = nullptr; b->held = 0;
}
// Every arena of every derived layout of the table, kind by kind: f(kind, layout, plane, arena). `which`: bit 0 what belongs to the
// projections (kinds 1, 3, 4), bit 1 the predicate projections' planes (kind 2) — vh_table_relocate's bits —, VL_ALL the rest as well.
enum { VL_PACK = 1, VL_PLANE = 2, VL_GROUPED = 3, VL_GPLANES = 4, VL_GHDR = 5, VL_NARROW = 6, VL_ALL = ~0u };
static const char* const VL_NAME[] = {"", "projection", "predicate plane", "grouped projection", "clustered planes", "grouped headers", "narrow"};
template <class F> static void derived_each(vh_table* t, uint32_t which, F&& f) {
  if (which & 1u) {
    for (auto& pk : t->packs) if (pk->rec.ptr) f(VL_PACK, *pk, 0, pk->rec);
    for (auto& pk : t->packs) if (pk->grouped && pk->grouped->rec.ptr) f(VL_GROUPED, *pk->grouped, 0, pk->grouped->rec);
    for (auto& pk : t->packs) if (pk->grouped && pk->grouped->planes.ptr) f(VL_GPLANES, *pk->grouped, 0, pk->grouped->planes);
  }
  if (which & 2u) for (auto& pp : t->predpacks) for (int q = 0; q < pp->nplanes; ++q) if (pp->plane[q].ptr) f(VL_PLANE, *pp, q, pp->plane[q]);
  if (which == VL_ALL) {
    for (auto& pk : t->packs) if (pk->grouped && pk->grouped->hdr.ptr) f(VL_GHDR, *pk->grouped, 0, pk->grouped->hdr);
    for (auto& nw : t->narrows) if (nw->copy.ptr) f(VL_NARROW, *nw, 0, nw->copy);
  }
}

static int table_grow(vh_table* t, uint32_t need_seg) {
  if (need_seg <= t->cap_seg) return VH_OK;
  uint32_t ncap = std::max<uint32_t>(need_seg, std::max<uint32_t>(4, t->cap_seg * 2));
  if (t->cap_seg) { build_arenas_moving(t); ++t->arena_gen; }
  for (auto& c : t->cols) {
    if (is_bitset_elem(c.elem)) {
      c.bs_offsets.resize(ncap, nullptr); c.bs_offsets32.resize(ncap, nullptr); c.bs_values.resize(ncap, nullptr); c.bs_nvalues.resize(ncap, 0); c.bs_maxid.resize(ncap, 0);
      continue;
    }
    char* nb = nullptr;
    const size_t bytes = VhBuf::bytes(ncap, c.stride);
    HIP_TRY(hipMalloc(&nb, bytes));
    trace_alloc("column", nb, bytes);
    if (c.base && t->nseg) {
      HIP_TRY(hipMemcpyAsync(nb, c.base, (size_t)t->nseg * c.stride, hipMemcpyDeviceToDevice, g_ctx.stream));
      HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    }
    if (c.base) { HIP_TRY(hipFree(c.base)); t->device_bytes -= VhBuf::bytes(t->cap_seg, c.stride); }
    c.base = nb;
    t->device_bytes += bytes;
  }
  t->cap_seg = ncap;
  t->seg_rows.resize(ncap, 0);
  t->seg_mod.resize(ncap, 0);
  for (auto& s : t->stats) s.resize(ncap);
  return VH_OK;
}

extern "C" int vh_table_create(const vh_col_desc* cols, int32_t ncols, uint64_t segment_rows,
                               uint32_t reserve_segments, vh_table** out) {
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  VH_ENTER();
  if (!cols || ncols <= 0 || !out || segment_rows == 0 || segment_rows > 0xFFFF0000ull)
    return vh_fail(VH_E_INVALID, "vh_table_create: bad arguments");
  vh_table* t = new vh_table();
  t->segment_rows = segment_rows;
  t->padded_rows = (segment_rows + 63) / 64 * 64;
  t->build_mode = knobs().build_background ? VH_BUILD_BACKGROUND : VH_BUILD_INLINE;
  t->layout_budget = knobs().layout_budget;
  t->cols.resize(ncols);
  t->stats.resize(ncols);
  for (int i = 0; i < ncols; ++i) {
    VhColumn& c = t->cols[i];
    c.kind = cols[i].kind; c.elem = cols[i].elem;
    const bool dim_kind = c.kind >= VH_DIM_STRING && c.kind <= VH_DIM_BOOLEAN, metric_kind = c.kind >= VH_METRIC_MAX && c.kind <= VH_METRIC_HIDDEN_COUNT;
    if ((!dim_kind && !metric_kind) || (is_bitset_elem(c.elem) != (c.kind == VH_METRIC_BITSET))) {
      delete t;
      return vh_fail(VH_E_INVALID, "column %d: bad kind %d / element type %d", i, cols[i].kind, cols[i].elem);
    }
    if (is_bitset_elem(c.elem)) { c.esize = 0; continue; }
    c.esize = vh_elem_size(c.elem);
    if (!c.esize) { delete t; return vh_fail(VH_E_INVALID, "column %d: bad element type %d", i, c.elem); }
    c.stride = t->padded_rows * c.esize;
  }
  int rc = table_grow(t, std::max<uint32_t>(1, reserve_segments));
  if (rc) { vh_table_destroy(t); return rc; }
  *out = t;
  return VH_OK;
}

// ------------------------------------------------------------------ execution contexts
static void exec_free(VhExec* x) {
  if (x->scratch) (void)hipFree(x->scratch);
  if (x->d_sample) (void)hipFree(x->d_sample);
  for (auto& hp : x->h_out) if (hp) (void)hipHostFree(hp);
  if (x->h_segrows) (void)hipHostFree(x->h_segrows);
  if (x->h_counters) (void)hipHostFree(x->h_counters);
  for (auto& e : x->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : x->ev_chunk) if (e) (void)hipEventDestroy(e);
  if (x->ev_fork) (void)hipEventDestroy(x->ev_fork);
  if (x->h_chunk) (void)hipHostFree(x->h_chunk);
  if (x->aux) (void)hipStreamDestroy(x->aux);
  if (x->copy) (void)hipStreamDestroy(x->copy);
  if (x->h_batch) (void)hipHostFree(x->h_batch);
  if (x->d_batch) (void)hipFree(x->d_batch);
  for (auto& e : x->ev_batch) if (e) (void)hipEventDestroy(e);
  if (x->own_stream) (void)hipStreamDestroy(x->own_stream);
}
// A free context of the table's pool, a new one while the pool may grow, else wait for one to come back.
// (Round 2 timed partitioned plans on three contexts and kept the one whose scratch "landed best": the tuple pool's placement decided
// 10 % of phase 1 when tuples left as partial lines. Whole-line tuple writes removed the sensitivity — eight processes, trials 1 vs 3:
// 2.50-2.54 vs 2.42-2.53 ms, profiles/r03/NOTES.md — and with it the three scratch buffers per table.)
static int exec_acquire(vh_table* t, VhExec** out, bool wait = true) {      // wait = false: a context that is free or can be made now, or VH_E_NOMEM at once (no message)
  const size_t max_exec = (size_t)knobs().max_exec;
  std::unique_lock<std::mutex> lk(t->pool_mu);
  for (;;) {
    for (auto& x : t->execs) if (!x->busy) { x->busy = true; *out = x.get(); return VH_OK; }
    if (t->execs.size() < max_exec) break;
    if (!wait) return VH_E_NOMEM;
    if (t->pool_cv.wait_for(lk, std::chrono::seconds(60)) == std::cv_status::timeout)
      return vh_fail(VH_E_NOMEM, "all %zu execution contexts of this table are held by live vh_result / running queries (vh_result_free them)", max_exec);
  }
  std::unique_ptr<VhExec> x(new VhExec());
  hipError_t he = hipStreamCreateWithFlags(&x->own_stream, hipStreamNonBlocking);
  if (he == hipSuccess) he = hipHostMalloc((void**)&x->h_counters, (16 + 64) * sizeof(unsigned long long), hipHostMallocDefault);
  for (auto& e : x->ev) if (he == hipSuccess) he = hipEventCreate(&e);
  if (he != hipSuccess) { exec_free(x.get()); return vh_fail(VH_E_DEVICE, "execution context: stream / pinned staging / events: %s", hipGetErrorString(he)); }
  x->busy = true;
  *out = x.get();
  t->execs.push_back(std::move(x));
  return VH_OK;
}
static int exec_streaming(VhExec* x) {       // what a streamed result needs on top of a context's stream; once per context
  if (x->copy) return VH_OK;
  HIP_TRY(hipStreamCreateWithFlags(&x->aux, hipStreamNonBlocking));
  { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi); HIP_TRY(hipStreamCreateWithPriority(&x->copy, hipStreamNonBlocking, 0)); }
  HIP_TRY(hipEventCreateWithFlags(&x->ev_fork, hipEventDisableTiming));
  for (auto& e : x->ev_chunk) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipHostMalloc((void**)&x->h_chunk, VH_HP_CHUNKS * sizeof(unsigned long long), hipHostMallocCoherent));
  return VH_OK;
}
static int exec_batch(VhExec* x) {           // what the lead context of a fused group needs on top of a context's stream; once per context
  if (x->ev_batch[1]) return VH_OK;
  if (!x->h_batch) HIP_TRY(hipHostMalloc((void**)&x->h_batch, VH_BATCH_MAX * sizeof(VhBatchMember), hipHostMallocDefault));
  if (!x->d_batch) HIP_TRY(hipMalloc((void**)&x->d_batch, VH_BATCH_MAX * sizeof(VhBatchMember)));
  for (auto& e : x->ev_batch) if (!e) HIP_TRY(hipEventCreate(&e));
  return VH_OK;
}
static void exec_release(vh_table* t, VhExec* x) {
  if (!x) return;
  { std::lock_guard<std::mutex> lk(t->pool_mu); x->busy = false; }
  t->pool_cv.notify_one();
}
// Before column arenas, CSR mirrors or projections are replaced: wait for every launched query that may still read them.
// Called with t->mu held (no new launch can start).
static void table_quiesce(vh_table* t) {
  std::lock_guard<std::mutex> lk(t->pool_mu);
  for (auto& x : t->execs) if (x->busy) (void)hipStreamSynchronize(x->stream());
}

// A sync changed rows [first, last) of a segment's columns: stamp the segment and tell the journal.
static void table_note_change(vh_table* t, uint32_t seg, uint64_t first, uint64_t last, bool new_epoch = true) {
  if (new_epoch) ++t->sync_epoch;
  t->seg_mod[seg] = t->sync_epoch;
  const char* cap_env = test_env("VH_TEST_JOURNAL_CAP");       // (tests: a few hundred small syncs push a layout behind the floor)
  const size_t cap = cap_env && atoi(cap_env) >= 2 ? (size_t)atoi(cap_env) : (1u << 18);
  if (t->journal.size() >= cap) {                 // keep the newer half; layouts older than the floor fall back to whole segments
    const size_t drop = t->journal.size() / 2;
    t->journal_floor = t->journal[drop - 1].epoch;
    t->journal.erase(t->journal.begin(), t->journal.begin() + (long)drop);
  }
  t->journal.push_back(VhChange{t->sync_epoch, seg, (uint32_t)first, (uint32_t)last});
}

extern "C" void vh_table_destroy(vh_table* t) {
  if (!t) return;
  VH_ENTER();
  build_cancel_table(t, true);
  (void)hipStreamSynchronize(g_ctx.stream);
  for (auto& x : t->execs) { (void)hipStreamSynchronize(x->stream()); exec_free(x.get()); }
  for (auto& c : t->cols) {
    if (c.base) (void)hipFree(c.base);
    for (auto p : c.bs_offsets) if (p) (void)hipFree(p);
    for (auto p : c.bs_offsets32) if (p) (void)hipFree(p);
    for (auto p : c.bs_values) if (p) (void)hipFree(p);
  }
  if (t->d_stats) (void)hipFree(t->d_stats);
  if (t->sync_ev) { (void)hipEventSynchronize(t->sync_ev); (void)hipEventDestroy(t->sync_ev); }
  if (t->h_sync) (void)hipHostFree(t->h_sync);
  if (t->h_stage) (void)hipHostFree(t->h_stage);
  if (t->d_packflag) (void)hipFree(t->d_packflag);
  derived_each(t, VL_ALL, [&](int, VhLayout&, int, VhBuf& b) { buf_free(t, &b); });
  if (t->jobs.buf) (void)hipHostFree(t->jobs.buf);
  if (t->derived_ev) (void)hipEventDestroy(t->derived_ev);
  delete t;
}

// What a partitioning query reads while it appends tuples, and where in its scratch the tuple pool will lie: enough to try a scratch
