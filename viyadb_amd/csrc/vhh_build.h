// vhh_build.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// the background build mode (vh_table_set_build_mode, VH_BUILD=background): kernel compiles and automatic layout builds off the query path.
//
// ONE worker thread per process, started by the first job, bound to the library's device, with a stream of its own; joined when the library
// is unloaded (g_build's destructor). No child processes. A query of a background table never compiles and never builds: where the inline
// mode would, it asks for a job here (build_request_*, t->mu held) and goes on with what exists; vh_result_info.reserved bit 19 says so.
// Jobs are keyed — kernel: VhJitShape::key(); layout: kind, form, column set — so a shape asked for a hundred times is built once.
//
// KERNELS. The job is vh_jit_get on the worker (disk cache or hipRTC; the code object is loaded and published under the JIT cache's own
// locks). Queries look the shape up with vh_jit_peek: absent or being compiled = pending (planned for the pre-built kernels exactly like
// "no kernel for this shape", but nothing is remembered or logged and VH_PLAN_FORCE_JIT is no error); a compile that failed is found there
// by the next query and reported as in the inline mode.
//
// LAYOUTS (payload projections, predicate projections, narrow copies) are built beside queries and syncs in three steps:
//   (a) under t->mu: the table's layout budget (derived_make_room: it may evict other layouts; the arenas count as vh_table::build_reserved
//       from here to the publish) and the free-memory guard (both evaluated NOW, not when the job was queued), the layout's description from the recorded stats,
//       its buffers, the journal epoch E and the arena generation it builds against, and the build kernels ENQUEUED on the worker's stream
//       (behind an event on the library's stream: every sync up to E has landed when they start);
//   (b) t->mu released: the kernels run; the worker waits for its stream;
//   (c) under t->mu: publish — applied_epoch = E, per-segment stamps as of (a), linked into t->packs / t->predpacks / t->narrows.
// The journalled refresh every derived layout has (derived_refresh) then re-derives what was synced after E before the first query reads the
// layout; a row a sync rewrote while (b) read it lies in such a range by construction.
//   * What keeps the arenas in place during (b): table_grow — the only code that replaces them — calls build_arenas_moving first, which waits
//     (t->mu held by the sync, not needed by step (b)) until the worker's stream is idle, and bumps vh_table::arena_gen; step (c) sees the
//     generation moved and the job starts over against the new arenas. A layout is never published at another capacity than the table's.
//   * A value that outgrows its field during (b): the projection kernels' own check (their overflow word, a private one of the worker) voids
//     the build at (c) — a compressed projection starts over at the widths the stats say now; what was synced after the rows were read is
//     caught by the first refresh (VH_PACK_STALE) or by the stats check of predpack_usable / narrow_usable, as for any layout. Never silently.
//   * The journal dropped its older half past E (VH_TEST_JOURNAL_CAP): the job starts over.
//   * The GROUPED form of a 4-byte bit-record projection (VhGrouped) is a second form of a layout that exists, not a layout of its own, and it
//     follows its projection's journalled refresh; it is built in one step under t->mu (allocate, enqueue group_bits_kernel on the library's
//     stream like any refresh, no host wait): by the worker's own query (build_warm) right after the projection and the planes it pairs with
//     were published, or by a VB_GROUPED job where a caller's query finds both without it. Counted in jobs_done, not in layouts_built.
// After the last waiting layout job of a table the worker runs the plans that asked for them once more (build_warm: a query whose rows are
// discarded, counted towards nothing), so that the kernel for the shape the NEW layouts give is queued at once and not by the next caller.
//
// LIFETIMES. vh_table_destroy and vh_table_unpack drop the table's queued jobs and wait for the running one (build_cancel_table, before they
// take t->mu); a job only ever creates layouts, it holds no pointer to an existing one. vh_table_prepare waits for the table's jobs, then
// goes on as in the inline mode (g_preparing). vh_query_agg_sharded / vh_query_select_sharded treat every table as inline: the ranks must agree
// on organisation and buffer list, and a rank-local "not ready yet" is out of scope.
//
// The worker's own queries (build_warm) are whole scans through the pre-built kernels, one per distinct asking plan (at most 64 remembered),
// counted in vh_build_info.warm_queries / warm_ms. Planning alone would do if the planner could stop before the launch for an aggregate;
// its plan_only mode stops before the organisation is chosen, which is what the kernel's shape depends on.
//
// SHUTDOWN. The library has no shutdown entry point: the worker is stopped and joined by g_build's destructor, a static of this translation
// unit declared after g_ctx and so destroyed before it. The JIT cache's statics live in another translation unit, whose destruction order
// against this one is not specified: a process that exits in the middle of a background compile is the one case this leaves open. A worker that is
// idle (the normal case at exit) leaves at once; one inside a compile or a kernel wait is waited for. Its stream, event, overflow word and
// pinned job list are left to the process's end on purpose: releasing them from a static destructor would call into a HIP runtime that may
// already be tearing down.
//
// Test hooks (test_env): VH_TEST_BUILD_HOLD=start — the worker accepts jobs but starts none while the variable reads so; =publish — a layout
// job waits between (b) and (c). Both polled (g_build_hold, refreshed from the environment on the calling threads only), ended by a cancel or the library's unloading.
#include <atomic>
#include <deque>
#include <functional>

static thread_local int g_build_quiet = 0;        // this thread's queries count towards no automatic layout and queue none (a pending query's second plan, the worker's own queries)
static thread_local bool g_build_inline = false;  // this thread's queries treat every table as inline (sharded queries)
static thread_local bool g_build_worker = false;  // this thread is the worker (its build_warm queries build a projection's grouped form themselves: choose_grouped)
// The plan being made on this thread reads layout `L` (t->mu held): stamped with the table's query tick, once per query however often the plan
// starts over, and before any automatic build site of the same plan runs — what a plan reads is never its own victim (derived_make_room).
// A quiet plan holds what it reads but counts as no use. vh_table_prepare remembers what its query read: pinned when it ends.
static void layout_use(vh_table* t, VhLayout* L) {
  L->held_tick = t->use_tick;
  if (g_build_quiet || g_plan_unstamped || L->last_use == t->use_tick) return;
  L->last_use = t->use_tick; ++L->uses;
  if (!g_preparing) return;
  g_prepare_reads.push_back(L->serial);
  if (!L->pinned) { L->pinned = true; g_prepare_pinned.push_back(L->serial); }      // (at once, under the lock the stamp is made under: no query between two rounds of the prepare evicts it)
}
static bool build_background(const vh_table* t) { return t->build_mode == VH_BUILD_BACKGROUND && !g_preparing && !g_build_inline; }

struct VhPlanCopy {        // a plan that outlives its caller's arrays (segment snapshot dropped: the rows of the last sync)
  vh_plan p{};
  std::vector<vh_filter_node> filter, having;
  std::vector<vh_anynum> lits;
  std::vector<vh_group_col> groups;
  std::vector<int32_t> metrics;
  std::string sig;
  explicit VhPlanCopy(const vh_plan& s) : p(s) {
    if (s.filter && s.nfilter > 0) filter.assign(s.filter, s.filter + s.nfilter);
    if (s.having && s.nhaving > 0) having.assign(s.having, s.having + s.nhaving);
    if (s.lits && s.nlits > 0) lits.assign(s.lits, s.lits + s.nlits);
    if (s.groups && s.ngroups > 0) groups.assign(s.groups, s.groups + s.ngroups);
    if (s.metrics && s.nmetrics > 0) metrics.assign(s.metrics, s.metrics + s.nmetrics);
    p.filter = filter.empty() ? nullptr : filter.data(); p.having = having.empty() ? nullptr : having.data();
    p.lits = lits.empty() ? nullptr : lits.data(); p.groups = groups.empty() ? nullptr : groups.data(); p.metrics = metrics.empty() ? nullptr : metrics.data();
    p.seg_rows = nullptr; p.nseg = 0;
    auto put = [&](const void* b, size_t n) { sig.append(static_cast<const char*>(b), n); sig.push_back('|'); };
    put(filter.data(), filter.size() * sizeof(vh_filter_node)); put(having.data(), having.size() * sizeof(vh_filter_node));
    put(lits.data(), lits.size() * sizeof(vh_anynum)); put(groups.data(), groups.size() * sizeof(vh_group_col)); put(metrics.data(), metrics.size() * 4);
    put(&p.flags, 4); put(&p.groups_hint, 8); put(&p.top_col, 4); put(&p.top_desc, 4); put(&p.top_k, 8);
  }
};

enum { VB_KERNEL = 0, VB_PACK = 1, VB_PREDPACK = 2, VB_NARROW = 3, VB_GROUPED = 4 };
struct VhBuildJob {
  vh_table* t = nullptr;
  int kind = VB_KERNEL;
  std::string key;
  VhJitShape shape;                    // VB_KERNEL
  std::vector<int> cols;               // layouts: the column set (VB_NARROW: one column; VB_GROUPED: the grouping column)
  uint32_t gbits = 0; uint64_t serial = 0;      // VB_GROUPED: the grouping column's field bits, and VhPack::serial of the projection the form belongs to
  uint64_t pp_serial = 0;              // ... and VhPredPack::serial of the bit-sliced predicate projection whose other columns' bits it keeps clustered (0: none)
  bool form = false, automatic = true; // VB_PACK: compressed records; VB_PREDPACK: bit-sliced planes
  bool pinned = false;                 // the layout it replaces was pinned (a compressed projection a value outgrew): so is this one
  std::string seen;                    // the sightings counter that asked (reset when the job comes to nothing)
  std::atomic<bool> cancel{false};
};
struct VhBuild {
  std::mutex mu;                       // taken AFTER t->mu where both are held; never held while t->mu is taken
  std::condition_variable cv;
  std::deque<std::shared_ptr<VhBuildJob>> queue;
  std::shared_ptr<VhBuildJob> running;
  bool reading = false;                // the running job's kernels may be reading the table's arenas (step (b))
  std::map<vh_table*, vh_build_info> info;
  std::map<vh_table*, std::vector<std::shared_ptr<VhPlanCopy>>> warm;      // plans whose queries asked for the layouts now being built
  std::thread worker;
  bool started = false, stop = false;
  hipStream_t stream = nullptr; hipEvent_t ev = nullptr; unsigned int* d_flag = nullptr;
  VhJobStage jobs;                     // the job list of the running layout job (one at a time: the worker waits for its stream before the next)
  ~VhBuild() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    if (worker.joinable()) worker.join();
  }
};
static VhBuild g_build;
// VH_TEST_BUILD_HOLD as the worker sees it: 0 none, 1 start, 2 publish. The environment is read on the CALLING threads only — whenever a job is
// queued and on entry to vh_table_build_info / vh_table_build_wait / vh_table_set_build_mode — never on the worker, which polls this word: a
// getenv there would race with the setenv of the test's own threads.
static std::atomic<int> g_build_hold{0};
static void build_hold_refresh() {
  const char* e = test_env("VH_TEST_BUILD_HOLD");
  g_build_hold.store(!e ? 0 : !strcmp(e, "start") ? 1 : !strcmp(e, "publish") ? 2 : 0);
}
static void build_worker_main();

// (t->mu held) Queue a job unless one with this key waits or runs for the table. true: there is such a job now.
static bool build_queue(vh_table* t, int kind, const std::string& key, const std::function<void(VhBuildJob&)>& fill, const vh_plan* plan) {
  build_hold_refresh();
  std::lock_guard<std::mutex> lk(g_build.mu);
  if (g_build.stop) return false;
  bool have = g_build.running && g_build.running->t == t && g_build.running->key == key && !g_build.running->cancel;
  for (auto& q : g_build.queue) have |= q->t == t && q->key == key;
  if (!have) {
    auto j = std::make_shared<VhBuildJob>();
    j->t = t; j->kind = kind; j->key = key;
    fill(*j);
    g_build.queue.push_back(j);
    ++g_build.info[t].jobs_queued;
    if (kind != VB_KERNEL && plan) {
      auto pc = std::make_shared<VhPlanCopy>(*plan);
      auto& w = g_build.warm[t];
      bool known = false;
      for (auto& o : w) known |= o->sig == pc->sig;
      if (!known && w.size() < 64) w.push_back(pc);
    }
    if (!g_build.started) { g_build.started = true; g_build.worker = std::thread(build_worker_main); }
    g_build.cv.notify_all();
  }
  return true;
}
static bool build_request_kernel(vh_table* t, const VhJitShape& s) {
  return build_queue(t, VB_KERNEL, "k:" + s.key(), [&](VhBuildJob& j) { j.shape = s; }, nullptr);
}
// `plan`: the aggregate plan that asked (nullptr: none to run again afterwards)
static bool build_request_layout(vh_table* t, int kind, const std::vector<int>& cols, bool form, bool automatic, const std::string& seen, const vh_plan* plan, bool pinned = false) {
  std::string key = kind == VB_PACK ? "p:" : kind == VB_PREDPACK ? "q:" : "n:";
  key += form ? "1:" : "0:";
  std::vector<int> sorted_cols = cols;
  std::sort(sorted_cols.begin(), sorted_cols.end());
  for (int c : sorted_cols) { key += std::to_string(c); key.push_back(','); }
  auto no = t->build_nothing.find(key);
  if (no != t->build_nothing.end()) { if (no->second == t->sync_epoch) return false; t->build_nothing.erase(no); }      // (judged "nothing to gain" at this very state of the table)
  return build_queue(t, kind, key, [&](VhBuildJob& j) { j.cols = cols; j.form = form; j.automatic = automatic; j.seen = seen; j.pinned = pinned; }, plan);
}

// The grouped form (VhGrouped) of projection `serial` by column `col`. It is no layout of its own but a second form of a projection that
// exists, so its job is short: grouped_build under t->mu (build_run_grouped), the kernel enqueued on the library's stream like any refresh.
// `sub_col`: the column a form built by this job is sub-sorted by (-1: none), decided where the job was asked for.
static bool build_request_grouped(vh_table* t, uint64_t serial, uint64_t pp_serial, int col, uint32_t bits, int sub_col, const std::string& seen, const vh_plan* plan) {
  const std::string key = "g:" + std::to_string(serial) + ":" + std::to_string(col) + ":" + std::to_string(bits) + ":" + std::to_string(pp_serial) + (sub_col >= 0 ? ":s" + std::to_string(sub_col) : std::string());
  return build_queue(t, VB_GROUPED, key, [&](VhBuildJob& j) { j.cols.assign(1, col); j.cols.push_back(sub_col); j.gbits = bits; j.serial = serial; j.pp_serial = pp_serial; j.seen = seen; }, plan);
}

static void build_arenas_moving(vh_table* t) {
  std::unique_lock<std::mutex> lk(g_build.mu);
  g_build.cv.wait(lk, [&] { return !(g_build.running && g_build.running->t == t && g_build.reading); });
}
static bool build_busy_locked(const vh_table* t) {
  if (g_build.running && g_build.running->t == t) return true;
  for (auto& q : g_build.queue) if (q->t == t) return true;
  return false;
}
static void build_cancel_table(vh_table* t, bool forget) {
  std::unique_lock<std::mutex> lk(g_build.mu);
  if (!g_build.started) return;
  for (auto it = g_build.queue.begin(); it != g_build.queue.end();) {
    if ((*it)->t != t) { ++it; continue; }
    auto f = g_build.info.find(t);
    if (f != g_build.info.end()) { --f->second.jobs_queued; ++f->second.jobs_cancelled; }
    it = g_build.queue.erase(it);
  }
  g_build.warm.erase(t);
  if (g_build.running && g_build.running->t == t) g_build.running->cancel = true;
  g_build.cv.notify_all();
  g_build.cv.wait(lk, [&] { return !(g_build.running && g_build.running->t == t); });
  if (forget) g_build.info.erase(t);
}
static void build_info_locked(vh_table* t, vh_build_info* out) {      // (g_build.mu held)
  auto f = g_build.info.find(t);
  *out = f != g_build.info.end() ? f->second : vh_build_info{};
}
static int build_wait(vh_table* t, uint32_t timeout_ms, vh_build_info* out) {
  bool idle = true;
  {
    std::unique_lock<std::mutex> lk(g_build.mu);
    auto done = [&] { return !build_busy_locked(t); };
    if (timeout_ms) idle = g_build.cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), done);
    else g_build.cv.wait(lk, done);
    if (out) build_info_locked(t, out);
  }
  if (out) { std::lock_guard<std::mutex> lk(t->mu); out->inline_builds = t->inline_builds; }
  return idle ? VH_OK : vh_fail(VH_E_RANGE, "vh_table_build_wait: jobs of this table still queued or running after %u ms", timeout_ms);
}

extern "C" int vh_table_set_build_mode(vh_table* t, int32_t mode) {
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  if (!t || (mode != VH_BUILD_INLINE && mode != VH_BUILD_BACKGROUND)) return vh_fail(VH_E_INVALID, "vh_table_set_build_mode: bad argument");
  build_hold_refresh();
  std::lock_guard<std::mutex> lk(t->mu);
  t->build_mode = mode;
  return VH_OK;
}
extern "C" int vh_table_build_wait(vh_table* t, uint32_t timeout_ms, vh_build_info* out) {
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  if (!t) return vh_fail(VH_E_INVALID, "null table");
  build_hold_refresh();
  return build_wait(t, timeout_ms, out);
}
extern "C" int vh_table_build_info(vh_table* t, vh_build_info* out) {
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  if (!t || !out) return vh_fail(VH_E_INVALID, "null argument");
  build_hold_refresh();
  { std::lock_guard<std::mutex> lk(g_build.mu); build_info_locked(t, out); }
  std::lock_guard<std::mutex> lk(t->mu);
  out->inline_builds = t->inline_builds;
  return VH_OK;
}

// ------------------------------------------------------------------ the worker
static void build_count(vh_table* t, const std::function<void(vh_build_info&)>& f) {
  std::lock_guard<std::mutex> lk(g_build.mu);
  auto it = g_build.info.find(t);
  if (it != g_build.info.end()) f(it->second);
}
static bool build_hold(const char* at) { return g_build_hold.load() == (!strcmp(at, "start") ? 1 : 2); }
static double build_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// 0: done, 1: failed, 2: cancelled, 3: declined (nothing to gain, no room under the free-memory guard, a build that was void)
static int build_run_kernel(VhBuildJob* j) {
  VhJitKernel* k = nullptr;
  std::string err;
  if (vh_jit_peek(j->shape, &k, &err) != 0) return k ? 0 : 1;      // (somebody — vh_table_prepare, an inline table — was faster)
  const auto t0 = std::chrono::steady_clock::now();
  k = vh_jit_get(j->shape, &err);
  const double ms = build_ms_since(t0);
  build_count(j->t, [&](vh_build_info& i) {
    if (!k) return;
    if (k->compile_ms > 0) ++i.kernels_compiled; else ++i.kernels_cached;
    i.compile_ms += ms;
  });
  if (knobs().times) fprintf(stderr, "vh build: kernel %s in %.1f ms on the worker\n", k ? k->name.c_str() : "(failed)", ms);
  return k ? 0 : 1;
}

// (t->mu held) Room for the grouped form of `pk` under the rule every automatic layout is built by: a quarter of the device stays free.
// 0: none; 1: for the grouped records; 2: for the clustered planes of `pp` (gbits of whose bits are the grouping column's) as well. What a form
// that is about to be replaced holds counts as free.
// Under a layout budget the same two questions are put to it first, planes included and then without (derived_make_room: it may evict other
// layouts, never `pk` or `pp`); a no counts in vh_table::declined unless this is vh_table_prepare, which the budget never refuses.
static int grouped_room(vh_table* t, const VhPack* pk, const VhPredPack* pp = nullptr, uint32_t gbits = 0, bool sub = false) {
  size_t free_b = 0, total_b = 0;
  const size_t need = (size_t)t->cap_seg * pk->rec.stride;
  const bool with_planes = pp && pp->sliced && pp->bits > gbits;
  const size_t planes = with_planes ? (size_t)t->cap_seg * vh_gplanes_seg_bytes(t->segment_rows, vh_gplanes_group(pp->bits - gbits)) : 0;
  int budget = 2;
  if (t->layout_budget && !g_preparing) {
    const VhGrouped* gr = pk->grouped.get();
    const uint64_t credit = gr ? gr->rec.held + gr->hdr.held + gr->planes.held : 0;
    const uint64_t tiles = (t->segment_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE;
    const uint64_t base = VhBuf::bytes(t->cap_seg, pk->rec.stride) + VhBuf::bytes(t->cap_seg, (tiles * vh_grouped_hdr_bytes(gbits) + 63) / 64 * 64);
    const uint64_t keys = sub ? (uint64_t)t->cap_seg * tiles * VH_GSUB_KEYS_BYTES : 0;      // (a sub-sorted form's boundary keys come with its planes)
    if (with_planes && derived_make_room(t, base + keys + VhBuf::bytes(t->cap_seg, vh_gplanes_seg_bytes(t->segment_rows, vh_gplanes_group(pp->bits - gbits))), pk, pp, credit)) budget = 2;
    else if (derived_make_room(t, base, pk, pp, credit)) budget = 1;
    else { ++t->declined; return 0; }
  }
  if (!device_mem(&free_b, &total_b)) return 0;
  if (const VhGrouped* gr = pk->grouped.get()) free_b += gr->rec.held + gr->planes.held;
  if (free_b <= need + total_b / 4) return 0;
  if (!with_planes) return 1;
  return std::min(budget, free_b > need + planes + total_b / 4 ? 2 : 1);
}
static int build_run_grouped(VhBuildJob* j) {
  vh_table* t = j->t;
  const auto t0 = std::chrono::steady_clock::now();
  int outcome = 3;
  {
    std::lock_guard<std::mutex> lk(t->mu);
    if (j->cancel) return 2;
    if (sync_resolve(t)) return 1;
    VhPack* pk = nullptr;
    for (auto& q : t->packs) if (q->serial == j->serial) pk = q.get();
    VhPredPack* pp = nullptr;
    for (auto& q : t->predpacks) if (j->pp_serial && q->serial == j->pp_serial) pp = q.get();
    const int sub_col = j->cols.size() > 1 ? j->cols[1] : -1;
    if (pk && pk->grouped && (!pp || (pk->grouped->planes.ptr && pk->grouped->pp_serial == pp->serial && (sub_col < 0 || pk->grouped->sub_col == sub_col)))) return 0;          // (vh_table_prepare or the worker's own query was faster; one grouped form per projection)
    const int room = pk ? grouped_room(t, pk, pp, j->gbits, sub_col >= 0) : 0;
    if (pk && pk->grouped && room < 2) return 0;          // (no room for the planes it lacks: the records it has stay)
    if (room) {
      if (grouped_build(t, pk, j->cols[0], j->gbits, room == 2 ? pp : nullptr, room == 2 ? sub_col : -1) != VH_OK) { (void)hipGetLastError(); outcome = 1; }
      else if (pk->grouped) outcome = 0;
    }
    if (outcome != 0) t->gather_seen[j->seen] = 0;      // the job came to nothing: the sightings start again
  }
  const double ms = build_ms_since(t0);
  if (outcome == 0) build_count(t, [&](vh_build_info& i) { i.layout_ms += ms; i.lock_ms += ms; });
  return outcome;
}

static int build_run_layout(VhBuildJob* j) {
  vh_table* t = j->t;
  auto nothing = [&](bool judged) {        // (t->mu held) the job comes to nothing: the sightings start again; `judged`: not before the table changes
    if (j->kind == VB_PACK) t->gather_seen[j->seen] = 0;
    else if (j->kind == VB_PREDPACK) t->ppred_seen[j->seen] = 0;
    else t->pred_seen[j->cols[0]] = 0;
    if (judged) t->build_nothing[j->key] = t->sync_epoch;
    return 3;
  };
  std::vector<int> sorted_cols = j->cols;
  std::sort(sorted_cols.begin(), sorted_cols.end());
  auto exists = [&]() -> bool {            // (t->mu held) an explicit call built the same meanwhile
    if (j->kind == VB_PACK) return pack_find(t, sorted_cols, j->form);
    if (j->kind == VB_PREDPACK) return predpack_find(t, sorted_cols, j->form);
    return narrow_find(t, j->cols[0]);
  };
  const auto t_begin = std::chrono::steady_clock::now();
  double lock_ms = 0;
  for (int attempt = 0; attempt < 4; ++attempt) {
    // the ONE layout this job builds: its kind's object, and what every kind shares — the common state `L`, its arenas, its launch
    std::unique_ptr<VhPack> pk; std::unique_ptr<VhPredPack> pp; std::unique_ptr<VhNarrow> nw;
    VhLayout* L = nullptr;
    std::vector<VhBuf*> bufs;
    std::function<void(const VhJob*, size_t)> launch;
    size_t bytes = 0;
    uint64_t E = 0, gen = 0;
    uint32_t nseg_a = 0;
    std::vector<uint64_t> mod_a;
    size_t njobs = 0;
    hipError_t he = hipSuccess;
    auto drop = [&] { for (VhBuf* b : bufs) buf_free(nullptr, b); };
    // ---- (a)
    {
      const auto a0 = std::chrono::steady_clock::now();
      std::lock_guard<std::mutex> lk(t->mu);
      struct Timer { double& acc; std::chrono::steady_clock::time_point t0; ~Timer() { acc += build_ms_since(t0); } } timer{lock_ms, a0};
      if (j->cancel) return 2;
      if (sync_resolve(t)) return 1;
      if (exists()) return 0;
      uint64_t row_limit = t->padded_rows;
      if (j->kind == VB_PACK) {
        if (pack_describe(t, j->cols, j->automatic, j->form, &pk)) return nothing(true);
        L = pk.get(); bufs.push_back(&pk->rec); row_limit = rows_padded_256(t);
        launch = [&](const VhJob* d_jobs, size_t n) { pack_launch(t, pk.get(), d_jobs, n, g_build.d_flag, g_build.stream); };
      } else if (j->kind == VB_PREDPACK) {
        if (predpack_describe(t, sorted_cols, j->automatic, j->form, &pp) || !pp) return nothing(true);
        L = pp.get();
        for (int q = 0; q < pp->nplanes; ++q) bufs.push_back(&pp->plane[q]);
        launch = [&](const VhJob* d_jobs, size_t n) { predpack_launch(t, pp.get(), d_jobs, n, g_build.stream); };
      } else {
        narrow_describe(t, j->cols[0], j->automatic, &nw);
        if (!nw) return nothing(true);
        L = nw.get(); bufs.push_back(&nw->copy);
        launch = [&](const VhJob* d_jobs, size_t n) { narrow_launch(t, nw.get(), d_jobs, n, g_build.stream); };
      }
      L->cap_seg = t->cap_seg; L->seg_mod.assign(t->cap_seg, 0); L->pinned = j->pinned;
      for (VhBuf* b : bufs) bytes += b->bytes(t->cap_seg);
      // the layout budget first (it may evict; a no evicts nothing), then the device's own guard
      if (!j->pinned && !derived_make_room(t, bytes)) { ++t->declined; return nothing(false); }
      // room: a quarter of the device stays free, and a projection does not outgrow the table
      if (!device_room(bytes) || (pk && bytes > t->device_bytes + 256)) return nothing(false);
      for (VhBuf* b : bufs) if (buf_alloc(nullptr, b, t->cap_seg, "background layout", true)) { drop(); return nothing(false); }
      t->build_reserved = bytes;      // real bytes that the ledger takes over at the publish: the budget counts them from now on
      E = t->sync_epoch; gen = t->arena_gen; nseg_a = t->nseg; mod_a = t->seg_mod;
      std::vector<VhJob> jobs;
      derived_jobs(t, *L, row_limit, false, &jobs);
      njobs = jobs.size();
      if (njobs) {
        const VhJob* d_jobs = nullptr;
        bool pending = false;                        // (the worker waited for its stream after the last list: the staging is free)
        g_build.jobs.used = 0;
        if (derived_upload(&g_build.jobs, &pending, jobs, &d_jobs)) { (void)hipGetLastError(); drop(); t->build_reserved = 0; return 1; }
        he = hipEventRecord(g_build.ev, g_ctx.stream);                       // every sync up to E has landed before the build kernels read
        if (he == hipSuccess) he = hipStreamWaitEvent(g_build.stream, g_build.ev, 0);
        if (he == hipSuccess && pk) he = hipMemsetAsync(g_build.d_flag, 0, 256, g_build.stream);
        if (he == hipSuccess) { launch(d_jobs, njobs); he = hipGetLastError(); }
        std::lock_guard<std::mutex> bl(g_build.mu);
        g_build.reading = true;
      }
    }
    // ---- (b): the kernels run beside queries and syncs; nobody waits for this thread
    unsigned int ovf = 0;
    if (njobs) {
      if (he == hipSuccess && pk) he = hipMemcpyAsync(&ovf, g_build.d_flag, sizeof(ovf), hipMemcpyDeviceToHost, g_build.stream);
      const hipError_t se = hipStreamSynchronize(g_build.stream);
      if (he == hipSuccess) he = se;
      { std::lock_guard<std::mutex> bl(g_build.mu); g_build.reading = false; }
      g_build.cv.notify_all();
    }
    while (build_hold("publish") && !j->cancel) {
      { std::lock_guard<std::mutex> bl(g_build.mu); if (g_build.stop) break; }
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    // ---- (c)
    {
      const auto c0 = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(t->mu);
      struct Timer { double& acc; std::chrono::steady_clock::time_point t0; ~Timer() { acc += build_ms_since(t0); } } timer{lock_ms, c0};
      const bool moved = t->arena_gen != gen || t->cap_seg != L->cap_seg || (E && E < t->journal_floor);
      const bool again = !j->cancel && he == hipSuccess && (moved || (ovf && pk && pk->compressed));
      t->build_reserved = 0;      // (published below, or dropped)
      if (j->cancel || he != hipSuccess || moved || ovf || exists()) {
        lk.unlock();
        drop();
        if (j->cancel) return 2;
        if (again) { build_count(t, [](vh_build_info& i) { ++i.layout_restarts; }); continue; }
        if (he != hipSuccess || ovf) { std::lock_guard<std::mutex> l2(t->mu); (void)nothing(false); return he != hipSuccess ? 1 : 3; }
        return 0;
      }
      for (uint32_t s = 0; s < nseg_a && s < L->seg_mod.size(); ++s) L->seg_mod[s] = mod_a[s];      // the stamps as of (a)
      L->applied_epoch = E; L->serial = ++t->layout_serial;
      for (VhBuf* b : bufs) t->device_bytes += b->held;      // (the one place beside buf_alloc: the arenas were made before the layout was the table's)
      if (pk) t->packs.push_back(std::move(pk));
      else if (pp) t->predpacks.push_back(std::move(pp));
      else t->narrows.push_back(std::move(nw));
      if (j->pinned) derived_trim(t, false);      // (the budget never refuses a pinned layout's rebuild; what is unpinned makes room afterwards)
    }
    const double ms = build_ms_since(t_begin);
    build_count(t, [&](vh_build_info& i) { ++i.layouts_built; i.layout_ms += ms; i.lock_ms += lock_ms; });
    if (knobs().times) fprintf(stderr, "vh build: layout %s in %.1f ms on the worker, the table lock held for %.3f ms of them (allocate + enqueue, publish)\n", j->key.c_str(), ms, lock_ms);
    return 0;
  }
  std::lock_guard<std::mutex> lk(t->mu);
  return nothing(false);
}

// The plan of a query that asked for layouts, once more, now that they exist: its kernel's shape has changed with them.
static void build_warm(vh_table* t, const VhPlanCopy* pc) {
  const auto t0 = std::chrono::steady_clock::now();
  ++g_build_quiet;
  vh_result* r = nullptr;
  if (vh_query_agg(t, &pc->p, &r) == VH_OK) vh_result_free(r);
  --g_build_quiet;
  const double ms = build_ms_since(t0);
  build_count(t, [&](vh_build_info& i) { ++i.warm_queries; i.warm_ms += ms; });
}

static void build_worker_main() {
  g_build_worker = true;
  (void)hipSetDevice(g_ctx.device);
  (void)hipStreamCreateWithFlags(&g_build.stream, hipStreamNonBlocking);
  (void)hipEventCreateWithFlags(&g_build.ev, hipEventDisableTiming);
  (void)hipMalloc((void**)&g_build.d_flag, 256);
  for (;;) {
    std::shared_ptr<VhBuildJob> j;
    {
      std::unique_lock<std::mutex> lk(g_build.mu);
      for (;;) {
        if (g_build.stop) return;
        const bool held = build_hold("start");
        if (!held && !g_build.queue.empty()) break;
        if (held) g_build.cv.wait_for(lk, std::chrono::milliseconds(2));
        else g_build.cv.wait(lk);
      }
      auto it = g_build.queue.begin();      // layouts first: the kernel worth compiling is the one for the shape they give
      for (auto q = g_build.queue.begin(); q != g_build.queue.end(); ++q) if ((*q)->kind != VB_KERNEL) { it = q; break; }
      j = *it;
      g_build.queue.erase(it);
      g_build.running = j;
      auto f = g_build.info.find(j->t);
      if (f != g_build.info.end()) { --f->second.jobs_queued; ++f->second.jobs_running; }
    }
    const bool usable = g_build.stream && g_build.ev && g_build.d_flag;
    int outcome = j->kind == VB_KERNEL ? build_run_kernel(j.get()) : j->kind == VB_GROUPED ? build_run_grouped(j.get()) : usable ? build_run_layout(j.get()) : 1;
    if (j->kind != VB_KERNEL && !j->cancel) {
      std::vector<std::shared_ptr<VhPlanCopy>> plans;
      {
        std::lock_guard<std::mutex> lk(g_build.mu);
        bool more = false;
        for (auto& q : g_build.queue) more |= q->t == j->t && q->kind != VB_KERNEL;
        auto w = g_build.warm.find(j->t);
        if (!more && w != g_build.warm.end()) { plans.swap(w->second); g_build.warm.erase(w); }
      }
      for (auto& pc : plans) if (!j->cancel) build_warm(j->t, pc.get());
    }
    if (j->cancel) outcome = 2;
    {
      std::lock_guard<std::mutex> lk(g_build.mu);
      auto f = g_build.info.find(j->t);
      if (f != g_build.info.end()) { --f->second.jobs_running; ++(outcome == 0 ? f->second.jobs_done : outcome == 1 ? f->second.jobs_failed : outcome == 3 ? f->second.jobs_declined : f->second.jobs_cancelled); }
      g_build.running.reset();
      g_build.reading = false;
    }
    g_build.cv.notify_all();
  }
}
