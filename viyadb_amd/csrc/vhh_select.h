// vhh_select.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// select (ordered row emission): vh_query_select, and vh_query_select_sharded over a table sharded across GPUs.
// ----------------------------------------------------------------- select (ordered row emission)
struct vh_rows {
  vh_rows_info info{};
  uint32_t flags = 0;           // which kernels answered, in vh_result_info.reserved's bits (vh_rows_flags)
  std::vector<int> elem;
  std::vector<size_t> off;
  char* d_out = nullptr;
  char* h_out = nullptr;
  ~vh_rows() { if (d_out) (void)hipFree(d_out); if (h_out) (void)hipHostFree(h_out); }
};

extern "C" void vh_rows_free(vh_rows* r) { if (r) { VH_ENTER(); delete r; } }

extern "C" int vh_rows_get_info(vh_rows* r, vh_rows_info* info) {
  if (!r || !info) return vh_fail(VH_E_INVALID, "null argument");
  *info = r->info;
  return VH_OK;
}

extern "C" int vh_rows_flags(vh_rows* r, uint32_t* flags) {
  if (!r || !flags) return vh_fail(VH_E_INVALID, "null argument");
  *flags = r->flags;
  return VH_OK;
}

extern "C" int vh_rows_view(vh_rows* r, const void** cols) {
  if (!r || !cols) return vh_fail(VH_E_INVALID, "null argument");
  for (size_t c = 0; c < r->elem.size(); ++c) cols[c] = r->h_out ? r->h_out + r->off[c] : nullptr;
  return VH_OK;
}

// One table's select up to the number of passing rows of every segment: the plan (filter program, segment snapshot, scan
// geometry), the count and per-segment scan kernels, the totals on the host. What the emission needs is kept here; D lives
// here too, because the emission's copies of it are asynchronous.
struct VhSelectScan {
  std::unique_ptr<vh_result> pr;
  VhPlanDev P{};
  uint32_t nseg = 0, cps = 0;
  unsigned grid = 0;
  char* S = nullptr;
  size_t o_win = 0, o_sel = 0, o_bs[VH_MAX_SELECT] = {};
  const uint32_t* d_counts = nullptr;
  const unsigned long long* d_totals = nullptr;
  bool sliced = false;                        // the filter is read off the bit-sliced predicate planes (QueryBuild::snapshot_segments decides): A, not P
  VhSelectSliced A{};
  std::vector<unsigned long long> totals;     // passing rows per segment
  VhSelectDev D{};
};

static int select_count_locked(vh_table* t, VhExec* x, const vh_select_plan* sp, VhSelectScan* s) {
  const int ncols_t = (int)t->cols.size();
  for (int c = 0; c < sp->ncols; ++c)
    if (sp->cols[c] < 0 || sp->cols[c] >= ncols_t) return vh_fail(VH_E_INVALID, "selected column %d: bad column %d", c, sp->cols[c]);
  vh_plan p{};
  p.filter = sp->filter; p.nfilter = sp->nfilter; p.lits = sp->lits; p.nlits = sp->nlits;
  p.seg_rows = sp->seg_rows; p.nseg = sp->nseg; p.flags = sp->flags;
  vh_result* pr = nullptr;
  VhLaunchOpts o;
  o.plan_only = true;
  int rc = query_launch_locked(t, x, &p, &pr, o);
  if (rc) return rc;
  s->pr.reset(pr);
  VhPlanDev& P = s->P;
  P = pr->plan;
  const uint32_t nseg = s->nseg = P.nseg;
  hipStream_t st = x->stream();
  if (int frc = derived_fence(t, st)) return frc;
  if (nseg == 0) return VH_OK;

  const bool sliced = s->sliced = pr->sel_sliced;
  const uint32_t chunk_rows = sliced ? VH_SLICED_CHUNK_ROWS : VH_WAVE_STEP_ROWS;
  const uint32_t cps = s->cps = (uint32_t)((t->padded_rows + chunk_rows - 1) / chunk_rows);
  const uint64_t nchunks = (uint64_t)nseg * cps;
  ScratchPlan spn;
  const size_t o_ctr = spn.take(256), o_segrows = spn.take(pr->plan_words * 4), o_counts = spn.take(nchunks * 4),
               o_totals = spn.take((size_t)nseg * 8);
  s->o_win = spn.take((size_t)nseg * sizeof(VhSelectWindow));
  s->o_sel = spn.take(sizeof(VhSelectDev));
  size_t o_fbs[VH_MAX_BITSET] = {};
  for (int c = 0; c < sp->ncols; ++c) if (is_bitset_elem(t->cols[sp->cols[c]].elem)) s->o_bs[c] = spn.take((size_t)nseg * 8);
  for (size_t k = 0; k < pr->filter_bitset_cols.size(); ++k) o_fbs[k] = spn.take((size_t)nseg * 8);
  rc = ensure_scratch(x, spn.off);
  if (rc) return rc;
  char* S = s->S = x->scratch;
  HIP_TRY(hipEventRecord(x->ev[0], st));
  HIP_TRY(hipMemsetAsync(S + o_ctr, 0, 256, st));
  P.set = pr->place_sets(x->h_segrows, S + o_segrows);      // (into the pinned staging block, BEFORE the asynchronous upload reads it)
  HIP_TRY(hipMemcpyAsync(S + o_segrows, x->h_segrows, pr->plan_words * 4, hipMemcpyHostToDevice, st));
  P.prog = reinterpret_cast<const VhProgOp*>(S + o_segrows + pr->seg_words * 4);
  P.lits = reinterpret_cast<const uint64_t*>(S + o_segrows + pr->seg_words * 4 + pr->h_prog.size() * sizeof(VhProgOp));
  for (size_t k = 0; k < pr->filter_bitset_cols.size(); ++k) {     // bitset metrics in the filter: per-segment CSR offsets
    const VhColumn& fc = t->cols[pr->filter_bitset_cols[k]];
    for (uint32_t sg = 0; sg < nseg; ++sg)
      if (x->h_segrows[sg] && !fc.bs_offsets[sg]) return vh_fail(VH_E_INVALID, "bitset column %d of segment %u was never synced", pr->filter_bitset_cols[k], sg);
    HIP_TRY(hipMemcpy(S + o_fbs[k], fc.bs_offsets.data(), (size_t)nseg * 8, hipMemcpyHostToDevice));
    P.fbs_offs[k] = reinterpret_cast<const uint64_t* const*>(S + o_fbs[k]);
  }
  P.seg_rows = reinterpret_cast<const uint32_t*>(S + o_segrows);
  P.counters = reinterpret_cast<unsigned long long*>(S + o_ctr);
  uint32_t* d_counts = reinterpret_cast<uint32_t*>(S + o_counts);
  s->d_counts = d_counts;
  unsigned long long* d_totals = reinterpret_cast<unsigned long long*>(S + o_totals);
  s->d_totals = d_totals;
  s->grid = (unsigned)std::min<uint64_t>((nchunks + 3) / 4, (uint64_t)g_ctx.num_cu * 8);
  if (sliced) {
    VhSelectSliced& A = s->A;
    A.B = pr->sel_prog; A.B.set = P.set;
    A.L.planes = pr->sel_planes; A.L.stride = pr->sel_stride; A.L.pitch = pr->sel_pitch;
    A.seg_rows = P.seg_rows; A.counters = P.counters; A.nseg = nseg;
  }
  HIP_TRY(hipEventRecord(x->ev[1], st));
  if (sliced) hipLaunchKernelGGL(select_count_sliced_kernel, dim3(s->grid), dim3(256), 0, st, s->A, cps, d_counts);
  else hipLaunchKernelGGL(select_count_kernel, dim3(s->grid), dim3(256), 0, st, P, cps, d_counts);
  hipLaunchKernelGGL(select_scan_kernel, dim3(nseg), dim3(256), 0, st, d_counts, cps, d_totals);
  HIP_TRY(hipGetLastError());
  s->totals.assign(nseg, 0);
  HIP_TRY(hipMemcpyAsync(s->totals.data(), d_totals, (size_t)nseg * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VH_OK;
}

// The reference's loop (src/codegen/query/scan.cc:103-104,156-160), per segment instead of per row:
//   if (skip > 0 && row_index++ < skip) continue;  ...send...  if (limit > 0 && output_recs >= limit) break;
// `break` leaves the tuple loop only, so once the limit is reached every LATER segment still sends its first
// passing row before it breaks again. Kept: results must be identical to the reference's. Over a sharded table the
// segments are the global sequence (rank, local segment): every rank runs this same loop over all ranks' totals.
// -> rows sent; *passed = rows that passed the filter.
static uint64_t select_windows(const unsigned long long* totals, uint64_t nseg, uint64_t skip, uint64_t limit, VhSelectWindow* win,
                               uint64_t* passed_out) {
  uint64_t remaining_skip = skip, output_recs = 0, passed = 0;
  for (uint64_t s = 0; s < nseg; ++s) {
    const uint64_t n = totals[s];
    passed += n;
    const uint64_t skipped = std::min(n, remaining_skip);
    remaining_skip -= skipped;
    const uint64_t avail = n - skipped;
    uint64_t emit = avail;
    if (limit > 0 && avail > 0) emit = output_recs >= limit ? 1 : std::min(avail, limit - output_recs);
    win[s] = VhSelectWindow{skipped, skipped + emit, output_recs};
    output_recs += emit;
  }
  *passed_out = passed;
  return output_recs;
}

// Output arrays of `nrows` rows: one 256-byte aligned array per column, at off[c] of one allocation. -> its size.
static size_t select_layout(const std::vector<int>& elem, uint64_t nrows, std::vector<size_t>* off) {
  size_t bytes = 0;
  for (size_t c = 0; c < elem.size(); ++c) { (*off)[c] = bytes; bytes += (nrows * vh_elem_size(elem[c]) + 255) / 256 * 256; }
  return bytes;
}

// Emission of the rows inside the windows `win` (one per segment of s) into out[c] + out_base: select_emit_kernel, or its form over the planes.
static int select_emit_locked(vh_table* t, VhExec* x, const vh_select_plan* sp, VhSelectScan* s, const VhSelectWindow* win,
                              const std::vector<int>& elem, char* const* out) {
  hipStream_t st = x->stream();
  char* S = s->S;
  const uint32_t nseg = s->nseg;
  VhSelectDev& D = s->D;
  D = VhSelectDev{};
  D.ncols = sp->ncols;
  for (int c = 0; c < sp->ncols; ++c) {
    const VhColumn& col = t->cols[sp->cols[c]];
    D.esize[c] = (uint32_t)vh_elem_size(elem[c]);
    D.out[c] = out[c];
    if (is_bitset_elem(col.elem)) {
      for (uint32_t sg = 0; sg < nseg; ++sg)
        if (x->h_segrows[sg] && !col.bs_offsets[sg]) return vh_fail(VH_E_INVALID, "bitset column %d of segment %u was never synced", sp->cols[c], sg);
      HIP_TRY(hipMemcpyAsync(S + s->o_bs[c], col.bs_offsets.data(), (size_t)nseg * 8, hipMemcpyHostToDevice, st));
      D.base[c] = nullptr; D.bs_offs[c] = reinterpret_cast<const uint64_t* const*>(S + s->o_bs[c]);
    } else { D.base[c] = col.base; D.stride[c] = col.stride; }
  }
  HIP_TRY(hipMemcpyAsync(S + s->o_sel, &D, sizeof(D), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(S + s->o_win, win, (size_t)nseg * sizeof(VhSelectWindow), hipMemcpyHostToDevice, st));
  if (s->sliced)
    hipLaunchKernelGGL(select_emit_sliced_kernel, dim3(s->grid), dim3(256), 0, st, s->A, s->cps, s->d_counts, s->d_totals,
                       reinterpret_cast<const VhSelectWindow*>(S + s->o_win), reinterpret_cast<const VhSelectDev*>(S + s->o_sel));
  else
    hipLaunchKernelGGL(select_emit_kernel, dim3(s->grid), dim3(256), 0, st, s->P, s->cps, s->d_counts,
                       reinterpret_cast<const VhSelectWindow*>(S + s->o_win), reinterpret_cast<const VhSelectDev*>(S + s->o_sel));
  HIP_TRY(hipGetLastError());
  return VH_OK;
}

extern "C" int vh_query_select(vh_table* t, const vh_select_plan* sp, vh_rows** out) {
  if (!t || !sp || !out) return vh_fail(VH_E_INVALID, "null argument");
  if (sp->ncols < 0 || sp->ncols > VH_MAX_SELECT) return vh_fail(VH_E_UNSUPPORTED, "%d selected columns (max %d)", sp->ncols, VH_MAX_SELECT);
  VH_ENTER();
  VhExec* x = nullptr;
  if (int rc = exec_acquire(t, &x)) return rc;
  struct Release { vh_table* t; VhExec* x; ~Release() { (void)hipStreamSynchronize(x->stream()); exec_release(t, x); } } release{t, x};
  // select launches twice with a host decision in between: it keeps the table lock throughout (not the hot path)
  std::lock_guard<std::mutex> lk(t->mu);
  VhSelectScan s;
  if (int rc = select_count_locked(t, x, sp, &s)) return rc;
  const uint32_t nseg = s.nseg;
  hipStream_t st = x->stream();
  std::unique_ptr<vh_rows> rows(new vh_rows());
  rows->info.scanned_recs = s.pr->info.scanned_recs;
  rows->info.scanned_segments = s.pr->info.scanned_segments;
  rows->flags = s.pr->info.reserved;
  for (int c = 0; c < sp->ncols; ++c) rows->elem.push_back(is_bitset_elem(t->cols[sp->cols[c]].elem) ? VH_U64 : t->cols[sp->cols[c]].elem);
  rows->off.assign(sp->ncols, 0);
  if (nseg == 0) { *out = rows.release(); return VH_OK; }

  std::vector<VhSelectWindow> win(nseg);
  uint64_t passed = 0;
  const uint64_t output_recs = select_windows(s.totals.data(), nseg, sp->skip, sp->limit, win.data(), &passed);
  rows->info.nrows = output_recs;
  rows->info.passed_recs = passed;
  if (output_recs) {
    const size_t bytes = select_layout(rows->elem, output_recs, &rows->off);
    if (bytes > ((size_t)64 << 30)) return vh_fail(VH_E_NOMEM, "select would return %llu rows (%zu bytes): add a limit", (unsigned long long)output_recs, bytes);
    if (bytes) {
      HIP_TRY(hipMalloc((void**)&rows->d_out, bytes));
      HIP_TRY(host_alloc_near_device((void**)&rows->h_out, bytes, hipHostMallocDefault));
    }
    std::vector<char*> cols(sp->ncols);
    for (int c = 0; c < sp->ncols; ++c) cols[c] = rows->d_out + rows->off[c];
    if (int rc = select_emit_locked(t, x, sp, &s, win.data(), rows->elem, cols.data())) return rc;
    HIP_TRY(hipEventRecord(x->ev[2], st));
    if (bytes) HIP_TRY(hipMemcpyAsync(rows->h_out, rows->d_out, bytes, hipMemcpyDeviceToHost, st));
  } else {
    HIP_TRY(hipEventRecord(x->ev[2], st));
  }
  HIP_TRY(hipEventRecord(x->ev[3], st));
  HIP_TRY(hipStreamSynchronize(st));   // D and win live on this frame
  float ms = 0;
  (void)hipEventElapsedTime(&ms, x->ev[1], x->ev[2]); rows->info.kernel_ms = ms;
  (void)hipEventElapsedTime(&ms, x->ev[0], x->ev[3]); rows->info.total_ms = ms;
  *out = rows.release();
  return VH_OK;
}

// ----------------------------------------------------------------- select over a table sharded across GPUs
// The communicator is defined with the sharded aggregate (vh_sharded.h, later in this translation unit).
static int agree_status(vh_comm* comm, int lrc, const char* what);
static void comm_shape(const vh_comm* c, int* rank, int* world);
static std::mutex& comm_mutex(vh_comm* c);
static int comm_alltoallv(vh_comm* c, int32_t ncols, const void* const* send, void* const* recv, const uint32_t* esize,
                          const uint64_t* send_off, const uint64_t* recv_off, hipStream_t st);

// Every rank counts its shard's passing rows per segment; the counts are all-gathered, every rank runs select_windows over the
// global segment sequence and emits only its own slice of the answer, and one all-to-all-v carries the slices into root's output
// arrays, each at its offset. Root emits its own slice in place (its send to itself is that same range); the others emit into a
// buffer of their slice's size. Local failures are carried to the next status point (agree_status), as in vh_query_agg_sharded.
extern "C" int vh_query_select_sharded(vh_table* t, const vh_select_plan* sp, vh_comm* comm, int32_t root, vh_rows** out) {
  if (!t || !sp || !comm || !out) return vh_fail(VH_E_INVALID, "null argument");
  struct InlineBuilds { bool was = g_build_inline; InlineBuilds() { g_build_inline = true; } ~InlineBuilds() { g_build_inline = was; } } inline_builds;      // (sharded queries treat every table as inline: vhh_build.h)
  int R = 0, W = 1;
  comm_shape(comm, &R, &W);
  if (root < 0 || root >= W) return vh_fail(VH_E_INVALID, "root %d of %d ranks", root, W);
  if (sp->ncols < 0 || sp->ncols > VH_MAX_SELECT) return vh_fail(VH_E_UNSUPPORTED, "%d selected columns (max %d)", sp->ncols, VH_MAX_SELECT);
  if (W == 1 && !test_env("VH_TEST_SHARDED_WORLD1")) return vh_query_select(t, sp, out);   // (the test knob sends one rank through the whole protocol)
  VH_ENTER();
  std::lock_guard<std::mutex> comm_lk(comm_mutex(comm));
  int lrc = VH_OK;
  char lerr[sizeof(g_err)] = "";
  auto keep = [&](int rc) { if (rc && !lrc) { lrc = rc; snprintf(lerr, sizeof(lerr), "%s", g_err); } return rc; };
  VhExec* x = nullptr;
  keep(exec_acquire(t, &x));
  struct Release { vh_table* t; VhExec* x; ~Release() { if (x) { (void)hipStreamSynchronize(x->stream()); exec_release(t, x); } } } release{t, x};
  hipStream_t st = x ? x->stream() : nullptr;
  std::lock_guard<std::mutex> lk(t->mu);      // (as in vh_query_select: count and emission see one snapshot; held until the rows have left)
  VhSelectScan s;
  if (!lrc) keep(select_count_locked(t, x, sp, &s));

  // ---- 1. status, segment count and scan counters of every rank
  uint64_t mine[4] = {lrc ? 1ull : 0ull, lrc ? 0ull : s.nseg, s.pr && !lrc ? s.pr->info.scanned_recs : 0ull, s.pr && !lrc ? s.pr->info.scanned_segments : 0ull};
  std::vector<uint64_t> all((size_t)W * 4);
  if (int rc = vh_comm_allgather_host(comm, mine, all.data(), sizeof(mine))) return rc;
  if (lrc) return vh_fail(lrc, "%s", lerr);
  std::vector<uint64_t> nseg(W), base(W + 1, 0);
  uint64_t maxn = 0, scanned = 0, scanned_segs = 0;
  for (int p = 0; p < W; ++p) {
    if (all[(size_t)p * 4]) return vh_fail(VH_E_DEVICE, "select: failed on rank %d", p);
    nseg[p] = all[(size_t)p * 4 + 1]; base[p + 1] = base[p] + nseg[p]; maxn = std::max(maxn, nseg[p]);
    scanned += all[(size_t)p * 4 + 2]; scanned_segs += all[(size_t)p * 4 + 3];
  }
  // ---- 2. passing rows per segment, padded to the largest shard
  std::vector<unsigned long long> totals(base[W], 0);
  if (maxn) {
    std::vector<unsigned long long> pad(maxn, 0), allt((size_t)W * maxn);
    std::copy(s.totals.begin(), s.totals.end(), pad.begin());
    if (int rc = vh_comm_allgather_host(comm, pad.data(), allt.data(), maxn * 8)) return rc;
    for (int p = 0; p < W; ++p) std::copy(allt.begin() + (size_t)p * maxn, allt.begin() + (size_t)p * maxn + nseg[p], totals.begin() + base[p]);
  }
  // ---- 3. the global window, and every rank's slice of it
  std::vector<VhSelectWindow> win(base[W]);
  uint64_t passed = 0;
  const uint64_t output_recs = select_windows(totals.data(), base[W], sp->skip, sp->limit, win.data(), &passed);
  std::vector<uint64_t> first(W + 1, output_recs);            // rank p's rows are [first[p], first[p + 1]) of the answer
  for (int p = W - 1; p >= 0; --p) first[p] = nseg[p] ? win[base[p]].out_base : first[p + 1];
  std::unique_ptr<vh_rows> rows(new vh_rows());
  rows->info.scanned_recs = scanned; rows->info.scanned_segments = scanned_segs; rows->info.passed_recs = passed;
  rows->info.nrows = R == root ? output_recs : 0;
  rows->flags = s.pr ? s.pr->info.reserved : 0u;        // (this rank's: the ranks need not agree on the path)
  for (int c = 0; c < sp->ncols; ++c) rows->elem.push_back(is_bitset_elem(t->cols[sp->cols[c]].elem) ? VH_U64 : t->cols[sp->cols[c]].elem);
  rows->off.assign(sp->ncols, 0);
  if (output_recs == 0 || sp->ncols == 0) {                   // (the same on every rank: nothing to move)
    *out = rows.release();
    return VH_OK;
  }
  {
    std::vector<size_t> off(sp->ncols);
    const size_t bytes = select_layout(rows->elem, output_recs, &off);
    if (bytes > ((size_t)64 << 30)) return vh_fail(VH_E_NOMEM, "select would return %llu rows (%zu bytes): add a limit", (unsigned long long)output_recs, bytes);   // (every rank)
  }
  const uint64_t mine_rows = first[R + 1] - first[R];
  char* d_send = nullptr;                                     // a non-root rank's slice
  struct SendGuard { char*& p; ~SendGuard() { if (p) (void)hipFree(p); } } send_guard{d_send};
  std::vector<size_t> soff(sp->ncols, 0);
  std::vector<char*> cols(sp->ncols, nullptr);
  std::vector<VhSelectWindow> mywin(win.begin() + base[R], win.begin() + base[R + 1]);
  size_t out_bytes = 0;
  if (R == root) {
    out_bytes = select_layout(rows->elem, output_recs, &rows->off);
    if (hipMalloc((void**)&rows->d_out, out_bytes) != hipSuccess || host_alloc_near_device((void**)&rows->h_out, out_bytes, hipHostMallocDefault) != hipSuccess)
      keep(vh_fail(VH_E_NOMEM, "no memory for %llu selected rows", (unsigned long long)output_recs));
    for (int c = 0; c < sp->ncols && !lrc; ++c) cols[c] = rows->d_out + rows->off[c];
  } else if (mine_rows) {
    const size_t bytes = select_layout(rows->elem, mine_rows, &soff);
    if (hipMalloc((void**)&d_send, bytes) != hipSuccess) keep(vh_fail(VH_E_NOMEM, "no memory for %llu selected rows", (unsigned long long)mine_rows));
    for (int c = 0; c < sp->ncols && !lrc; ++c) cols[c] = d_send + soff[c];
    for (VhSelectWindow& w : mywin) w.out_base -= first[R];
  }
  if (!lrc && mine_rows) keep(select_emit_locked(t, x, sp, &s, mywin.data(), rows->elem, cols.data()));
  (void)hipEventRecord(x->ev[2], st);
  if (int rc = agree_status(comm, lrc, "sending the selected rows")) return rc;   // every slice and root's output arrays exist

  // ---- 4. every slice to root, straight into its output arrays
  std::vector<const void*> send(sp->ncols);
  std::vector<void*> recv(sp->ncols, nullptr);
  std::vector<uint32_t> es(sp->ncols);
  for (int c = 0; c < sp->ncols; ++c) {
    es[c] = (uint32_t)vh_elem_size(rows->elem[c]);
    send[c] = R == root ? rows->d_out + rows->off[c] + first[R] * es[c] : cols[c];
    if (R == root) recv[c] = rows->d_out + rows->off[c];
  }
  std::vector<uint64_t> so(W + 1, 0), ro(W + 1, 0);
  for (int p = 0; p <= W; ++p) so[p] = p > root ? mine_rows : 0;          // everything goes to root
  if (R == root) for (int p = 0; p <= W; ++p) ro[p] = first[p];           // rank p's slice lands at its offset of the answer
  if (int rc = comm_alltoallv(comm, sp->ncols, send.data(), recv.data(), es.data(), so.data(), ro.data(), st))
    return rc < 0 ? rc : vh_fail(VH_E_DEVICE, "gather of the selected rows failed (%d)", rc);
  if (R == root) HIP_TRY(hipMemcpyAsync(rows->h_out, rows->d_out, out_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(x->ev[3], st));
  HIP_TRY(hipStreamSynchronize(st));   // D and the windows live on this frame
  float ms = 0;
  if (s.nseg) { (void)hipEventElapsedTime(&ms, x->ev[1], x->ev[2]); rows->info.kernel_ms = ms; }
  ms = 0;
  if (s.nseg) { (void)hipEventElapsedTime(&ms, x->ev[0], x->ev[3]); rows->info.total_ms = ms; }
  *out = rows.release();
  return VH_OK;
}
