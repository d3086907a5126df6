// vhh_derived.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// the derived layouts — second forms of the column arenas that the scan kernels read instead of them:
//   * payload projections (vh_table_pack, VhPack): a few columns row-major in one record per row, plain, compressed or as bit fields;
//   * their grouped form (VhGrouped): the 4-byte bit records of every 2048-row tile sorted by an equality column, the tiles' headers, and
//     beside them the clustered planes — the other predicate columns' bits in the tiles' grouped order;
//   * narrow copies (vh_table_narrow, VhNarrow): an unsigned 32-bit predicate column at 8 or 16 bits;
//   * predicate projections (vh_table_predpack, VhPredPack): the predicate columns as bit fields of one word per row, as byte planes or bit-sliced.
// They have ONE shape. Every layout is a VhLayout (capacity, per-segment stamps, the journal epoch it is current at, serial) that owns
// VhBuf arenas (vhh_table.h); arenas come and go through buf_alloc / buf_free alone, which keep the table's byte ledger; derived_each
// visits every arena of a table (bytes, move, settle, unpack, destroy). What is specific to a kind is its description (*_describe: fields
// and strides from the recorded stats, on top of vhh_layout_math.h), its build kernel (*_launch) and how it is found (*_find); the
// rest is written once:
//   * derived_refresh — grow with the table, cut what the journal says changed into jobs (vh_cut_jobs, vhh_layout_math.h), upload, launch,
//     order queries behind the launch, stamp. The background build (vhh_build.h) uses the same describe / launch / upload pieces off the lock;
//   * derived_drop — quiesce the table, wait for the library's stream, free through the ledger, erase;
//   * derived_move / derived_settle — try other places for the arenas (vh_table_prepare, vh_table_relocate).
//   * derived_make_room / derived_trim — how long a layout lives: the table's byte budget, use stamps, LRU eviction through the drop
//     functions, pins, and the listing (vh_table_layouts) — see "lifetimes" below.
#define VH_PACK_STALE 9001      // (internal) pack_refresh: a value no longer fits its stored width, the projection must go
#define VH_NO_ROOM 9002         // (internal) derived_refresh of a layout that starts over when the table grew: no room for an arena it cannot do without
// Over the byte budget (vh_table::layout_budget): unpinned layouts leave, least recently used first (defined below, after the drop functions).
static void derived_trim(vh_table* t, bool in_plan);
static uint64_t rows_padded_256(const vh_table* t) { return (t->segment_rows + 255) / 256 * 256; }      // rows a projection's stride has room for
// What layout `L` has to re-derive, as jobs for its kernel (vh_cut_jobs): the journal's ranges since it was current, or whole segments.
static void derived_jobs(const vh_table* t, const VhLayout& L, uint64_t row_limit, bool whole_tiles, std::vector<VhJob>* jobs) {
  const VhCutTable T{t->journal.data(), t->journal.size(), t->journal_floor, t->seg_mod.data(), t->seg_rows.data(), t->nseg};
  vh_cut_jobs(T, VhCutLayout{L.seg_mod.data(), L.seg_mod.size(), L.applied_epoch, row_limit}, whole_tiles, jobs);
}
// The jobs in pinned memory the kernels read them from. Lists are appended while earlier ones may still be read; when the staging is full
// and *pending says so, the library's stream — the reader — is waited for first.
static int derived_upload(VhJobStage* S, bool* pending, const std::vector<VhJob>& jobs, const VhJob** out) {
  const size_t bytes = jobs.size() * sizeof(VhJob);
  if (S->used + bytes > S->bytes) {
    if (*pending) { HIP_TRY(hipStreamSynchronize(g_ctx.stream)); *pending = false; }      // (earlier lists are still being read)
    S->used = 0;
    if (bytes > S->bytes) {
      if (S->buf) { HIP_TRY(hipHostFree(S->buf)); S->buf = nullptr; S->bytes = 0; }
      const size_t nb = std::max<size_t>(bytes * 2, 1u << 16);
      HIP_TRY(hipHostMalloc((void**)&S->buf, nb, hipHostMallocCoherent));
      S->bytes = nb;
    }
  }
  memcpy(S->buf + S->used, jobs.data(), bytes);
  *out = reinterpret_cast<const VhJob*>(S->buf + S->used);
  S->used += (bytes + 255) / 256 * 256;
  return VH_OK;
}
static int derived_enqueued(vh_table* t) {       // a refresh kernel went onto g_ctx.stream: queries launched from now on wait for it (QueryBuild::launch)
  if (!t->derived_ev) HIP_TRY(hipEventCreateWithFlags(&t->derived_ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(t->derived_ev, g_ctx.stream));
  t->derived_pending = true;
  return VH_OK;
}
static int derived_waited(vh_table* t) {         // the host waited for g_ctx.stream: nothing pending, the job lists are free
  t->derived_pending = false; t->jobs.used = 0;
  return VH_OK;
}
// Work about to go onto a query's own stream reads derived layouts (and arenas): it is ordered behind the refreshes enqueued on g_ctx.stream.
static int derived_fence(vh_table* t, hipStream_t st) {
  if (!t->derived_pending) return VH_OK;
  if (hipEventQuery(t->derived_ev) == hipSuccess) return derived_waited(t);
  HIP_TRY(hipStreamWaitEvent(st, t->derived_ev, 0));
  return VH_OK;
}
// Before an arena of a layout is freed or replaced (t->mu held): no launched query reads it, no refresh writes it, the job lists are free.
static int derived_idle(vh_table* t) {
  table_quiesce(t);
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  return derived_waited(t);
}

// ------------------------------------------------------- the build kernels' launches: over a list of jobs (pinned memory), on `st`
template <class Args> static void args_sources(const vh_table* t, const std::vector<int>& cols, Args* A) {      // the source columns' arenas
  for (size_t c = 0; c < cols.size(); ++c) {
    const VhColumn& col = t->cols[cols[c]];
    A->src[c] = col.base; A->src_stride[c] = col.stride; A->esize[c] = (uint32_t)col.esize;
  }
}
static void pack_bits_args(const vh_table* t, const VhPack* pk, char* dst, const VhJob* d_jobs, unsigned int* flag, VhPackBitsArgs* B) {
  B->ncols = (int32_t)pk->cols.size(); B->rec_bytes = pk->rec_bytes;
  args_sources(t, pk->cols, B);
  for (size_t c = 0; c < pk->cols.size(); ++c) { B->bitoff[c] = pk->bitoff[c]; B->bitw[c] = pk->bitw[c]; }
  B->overflow = flag; B->dst = dst; B->dst_stride = pk->rec.stride; B->jobs = d_jobs;
}
// `flag`: the "a value outgrew its stored width" word.
static void pack_launch(const vh_table* t, const VhPack* pk, const VhJob* d_jobs, size_t njobs, unsigned int* flag, hipStream_t st) {
  if (pk->bits) {
    VhPackBitsArgs B{};
    pack_bits_args(t, pk, pk->rec.ptr, d_jobs, flag, &B);
    hipLaunchKernelGGL(pack_bits_kernel, dim3((unsigned)njobs), dim3(256), 0, st, B);
  } else {
    VhPackArgs A{};
    A.ncols = (int32_t)pk->cols.size(); A.rec_bytes = pk->rec_bytes;
    args_sources(t, pk->cols, &A);
    for (size_t c = 0; c < pk->cols.size(); ++c) {
      A.off[c] = pk->off[c]; A.wbytes[c] = pk->width[c];
      if (vh_elem_signed(t->cols[pk->cols[c]].elem)) A.sgn_mask |= 1u << c;
    }
    A.overflow = flag; A.dst = pk->rec.ptr; A.dst_stride = pk->rec.stride; A.jobs = d_jobs;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)njobs), dim3(256), 256 * pk->rec_bytes, st, A);
  }
}
// The grouped form of `pk`: records, headers and — where it has them — the clustered planes out of one launch, one block per tile.
static void grouped_launch(const vh_table* t, const VhPack* pk, const VhJob* d_jobs, size_t njobs, unsigned int* flag, hipStream_t st) {
  const VhGrouped* gr = pk->grouped.get();
  VhGroupArgs A{};
  pack_bits_args(t, pk, gr->rec.ptr, d_jobs, flag, &A.B);
  const VhColumn& gc = t->cols[gr->col];
  A.gsrc = gc.base; A.gsrc_stride = gc.stride; A.gesize = (uint32_t)gc.esize; A.gbits = gr->bits;
  A.hdr = gr->hdr.ptr; A.hdr_stride = gr->hdr.stride;
  if (gr->planes.ptr) {
    A.pncols = (int32_t)gr->pp_cols.size(); A.goff = gr->goff; A.G = gr->G;
    for (size_t c = 0; c < gr->pp_cols.size(); ++c) {
      const VhColumn& col = t->cols[gr->pp_cols[c]];
      A.psrc[c] = col.base; A.psrc_stride[c] = col.stride; A.pesize[c] = (uint32_t)col.esize; A.pbitoff[c] = gr->pp_bitoff[c];
    }
    A.planes = gr->planes.ptr; A.planes_stride = gr->planes.stride;
    if (gr->sub_col >= 0) { A.sub_off = gr->sub_off; A.sub_bits = gr->sub_bits; A.keys_off = vh_gsub_keys_off((t->segment_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE, gr->bits); }
  }
  hipLaunchKernelGGL(group_bits_kernel, dim3((unsigned)njobs), dim3(256), 0, st, A);
}
static void narrow_launch(const vh_table* t, const VhNarrow* nw, const VhJob* d_jobs, size_t njobs, hipStream_t st) {
  const VhColumn& c = t->cols[nw->col];
  if (nw->width == 1)
    hipLaunchKernelGGL((narrow_kernel<uint8_t>), dim3((unsigned)njobs), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(c.base), c.stride / 4,
                       reinterpret_cast<uint8_t*>(nw->copy.ptr), nw->copy.stride, d_jobs);
  else
    hipLaunchKernelGGL((narrow_kernel<uint16_t>), dim3((unsigned)njobs), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(c.base), c.stride / 4,
                       reinterpret_cast<uint16_t*>(nw->copy.ptr), nw->copy.stride / 2, d_jobs);
}
static void predpack_launch(const vh_table* t, const VhPredPack* pp, const VhJob* d_jobs, size_t njobs, hipStream_t st) {
  VhPredPackArgs A{};
  A.ncols = (int32_t)pp->cols.size(); A.nplanes = pp->nplanes;
  args_sources(t, pp->cols, &A);
  for (size_t c = 0; c < pp->cols.size(); ++c) A.bitoff[c] = pp->bitoff[c];
  for (int q = 0; q < pp->nplanes; ++q) { A.plane[q] = pp->plane[q].ptr; A.plane_stride[q] = pp->plane[q].stride; A.plane_width[q] = (uint32_t)pp->pwidth[q]; A.plane_pos[q] = (uint32_t)pp->ppos[q]; }
  A.jobs = d_jobs;
  if (pp->sliced) hipLaunchKernelGGL(predslice_kernel, dim3((unsigned)njobs), dim3(256), 0, st, A, pp->bits, pp->pitch);
  else hipLaunchKernelGGL(predpack_kernel, dim3((unsigned)njobs), dim3(256), 0, st, A);
}
static int packflag_ready(vh_table* t) {       // the projection kernels' overflow word
  if (!t->d_packflag) { HIP_TRY(hipMalloc((void**)&t->d_packflag, 256)); HIP_TRY(hipMemsetAsync(t->d_packflag, 0, 256, g_ctx.stream)); }
  return VH_OK;
}

// ------------------------------------------------------- the refresh path
// What differs between the layouts when they follow the table.
struct VhRefresh {
  VhBuf* bufs[4] = {}; const char* what[4] = {}; int nbufs = 0;
  uint64_t row_limit = 0;        // rows a segment of the layout has room for: padded to 256 (projections, the grouped form) or vh_table::padded_rows
  bool whole_tiles = false;      // the ranges widened to whole 2048-row tiles
  bool restart = false;          // when the table grew: true — the arenas are made anew and everything is derived again (arenas of stride 0 are not
  int required = 0;              //   made; no room for one of the first `required`: VH_NO_ROOM, for a later one: it stays away); false — contents copied
  bool overflow_wait = false;    // wait for the kernel's overflow word: VH_PACK_STALE when a value outgrew its stored width
};
// Nothing to do — the test every query of a packed plan makes before anything else of a refresh exists.
static inline bool derived_current(const vh_table* t, const VhLayout& L) { return L.cap_seg >= t->cap_seg && L.applied_epoch == t->sync_epoch; }
// Bring a layout up to date with the arenas: re-derive what changed since it was last current in ONE launch on the library's stream, no
// host wait (but the overflow word's). launch(d_jobs, njobs) enqueues the layout's kernel.
template <class Launch> static int derived_refresh(vh_table* t, VhLayout* L, const VhRefresh& R, Launch&& launch) {
  if (!t->nseg) return VH_OK;
  if (L->cap_seg < t->cap_seg) {                        // the table grew
    if (int rc = derived_idle(t)) return rc;
    if (R.restart) for (int i = 0; i < R.nbufs; ++i) buf_free(t, R.bufs[i]);
    for (int i = 0; i < R.nbufs; ++i) {
      VhBuf old = *R.bufs[i], *b = R.bufs[i];
      if (R.restart) {
        if (b->stride && buf_alloc(t, b, t->cap_seg, R.what[i], true) != VH_OK && i < R.required) return VH_NO_ROOM;
        continue;
      }
      if (int rc = buf_alloc(t, b, t->cap_seg, R.what[i])) { *b = old; return rc; }
      if (old.ptr) {
        HIP_TRY(hipMemcpyAsync(b->ptr, old.ptr, (size_t)L->cap_seg * old.stride, hipMemcpyDeviceToDevice, g_ctx.stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
        buf_free(t, &old);
      }
    }
    L->cap_seg = t->cap_seg;
    if (R.restart) { L->seg_mod.assign(t->cap_seg, 0); L->applied_epoch = 0; }
    else L->seg_mod.resize(t->cap_seg, 0);
  }
  if (L->applied_epoch == t->sync_epoch) return VH_OK;
  std::vector<VhJob> jobs;
  derived_jobs(t, *L, R.row_limit, R.whole_tiles, &jobs);
  if (!jobs.empty()) {
    const VhJob* d_jobs = nullptr;
    if (int rc = derived_upload(&t->jobs, &t->derived_pending, jobs, &d_jobs)) return rc;
    if (int rc = launch(d_jobs, jobs.size())) return rc;
    HIP_TRY(hipGetLastError());
    if (R.overflow_wait) {                              // did every value survive its stored width? (the one host wait of a refresh)
      unsigned int ovf = 0;
      HIP_TRY(hipMemcpyAsync(&ovf, t->d_packflag, sizeof(ovf), hipMemcpyDeviceToHost, g_ctx.stream));
      HIP_TRY(hipStreamSynchronize(g_ctx.stream));
      derived_waited(t);
      if (ovf) {                                        // a synced value outgrew its stored width: the projection is void (the caller drops it)
        HIP_TRY(hipMemsetAsync(t->d_packflag, 0, 256, g_ctx.stream));
        return VH_PACK_STALE;
      }
    } else if (int rc = derived_enqueued(t)) return rc;
  }
  for (uint32_t s = 0; s < t->nseg; ++s) L->seg_mod[s] = t->seg_mod[s];
  L->applied_epoch = t->sync_epoch;
  return VH_OK;
}
// ------------------------------------------------------- the drop path
// `x` leaves `list`: nobody reads or writes its arenas any more, free_arenas() gives them back through the ledger, the layout is erased.
template <class T, class Free> static void derived_drop(vh_table* t, std::vector<std::unique_ptr<T>>* list, T* x, Free&& free_arenas) {
  (void)derived_idle(t);
  for (size_t k = 0; k < list->size(); ++k) {
    if ((*list)[k].get() != x) continue;
    free_arenas();
    list->erase(list->begin() + (long)k);
    return;
  }
}

// ------------------------------------------------------- value ranges of the columns (the recorded stats; arithmetic: vhh_layout_math.h)
// The range of a column's values over every mirrored segment; false: no stats for it.
static bool column_range(const vh_table* t, int col, VhRange* r) {
  if ((size_t)col >= t->stats.size() || t->stats[col].size() < t->nseg) return false;
  *r = vh_range_over(t->stats[col].data(), t->nseg);
  return true;
}
// Bytes the values of an integer column need over every mirrored segment (1, 2, 4 or 8; the element size for floating point): from the
// recorded stats, or from a min / max pass of its own where there are none.
static int column_stored_width(vh_table* t, int col, int* width_out) {
  const VhColumn& c = t->cols[col];
  *width_out = (int)c.esize;
  if (vh_elem_float(c.elem) || c.esize == 1 || !t->nseg) return VH_OK;
  VhRange r;
  if (!column_range(t, col, &r)) {      // (refresh_stats keeps min / max of every fixed-width column, metrics included)
    const uint32_t n = t->nseg;
    char* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)n * 16 + (size_t)n * 4 + 256));
    unsigned long long* d_st = reinterpret_cast<unsigned long long*>(tmp);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(tmp + (size_t)n * 16);
    std::vector<unsigned long long> init((size_t)n * 2);
    for (size_t i = 0; i < init.size(); i += 2) { init[i] = ~0ull; init[i + 1] = 0; }
    std::vector<uint32_t> hrows(n);
    for (uint32_t s = 0; s < n; ++s) hrows[s] = (uint32_t)t->seg_rows[s];
    hipError_t he = hipMemcpyAsync(d_st, init.data(), init.size() * 8, hipMemcpyHostToDevice, g_ctx.stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_rows, hrows.data(), hrows.size() * 4, hipMemcpyHostToDevice, g_ctx.stream);
    if (he == hipSuccess) {
      for (uint32_t first = 0; first < n; first += 32768) {       // (grid.y)
        const uint32_t cnt = std::min<uint32_t>(32768, n - first);
        dim3 grid((unsigned)std::min<uint64_t>(64, (t->segment_rows + 4095) / 4096), cnt);
        VH_ELEM_SWITCH(c.elem, (seg_minmax_kernel<T><<<grid, dim3(256), 0, g_ctx.stream>>>(reinterpret_cast<const T*>(c.base), c.stride / c.esize, d_rows + first, first, d_st + 2ull * first)));
      }
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(init.data(), d_st, init.size() * 8, hipMemcpyDeviceToHost, g_ctx.stream);
    if (he == hipSuccess) he = hipStreamSynchronize(g_ctx.stream);
    (void)hipFree(tmp);
    if (he != hipSuccess) return vh_fail(VH_E_DEVICE, "min / max pass over column %d: %s", col, hipGetErrorString(he));
    for (uint32_t s = 0; s < n; ++s) if (init[2 * s] <= init[2 * s + 1]) r.add(init[2 * s], init[2 * s + 1]);
  }
  *width_out = vh_range_stored_bytes(c.elem, (int)c.esize, r);
  return VH_OK;
}
// Width of a narrow copy of the column: 1, 2, or 0 (not an unsigned 32-bit column, no rows, or its values need more than 16 bits).
static int narrow_width_for(const vh_table* t, int col) {
  VhRange r;
  return column_range(t, col, &r) ? vh_range_narrow_width(t->cols[col].elem, r) : 0;
}
// Bits the values of a column need in a predicate projection (0: not an integer column, negative values, no rows, or no stats).
static int predpack_bits_for(const vh_table* t, int col) {
  VhRange r;
  return column_range(t, col, &r) ? vh_range_bits(t->cols[col].elem, r) : 0;
}

// ------------------------------------------------------- the grouped form of a bit-record projection (VhGrouped): built and refreshed with its projection, tile by tile
static void grouped_drop(vh_table* t, VhPack* pk) {      // (the caller made the table idle: derived_idle)
  VhGrouped* gr = pk->grouped.get();
  if (!gr) return;
  buf_free(t, &gr->rec); buf_free(t, &gr->hdr); buf_free(t, &gr->planes);
  pk->grouped.reset();
}
// The grouped records alone answer from now on — unless the form is sub-sorted: its places follow from no row-order formula, nothing can
// read it without the planes, so the whole form goes (the caller made the table idle: derived_idle).
static void grouped_no_planes(vh_table* t, VhPack* pk) {
  VhGrouped* gr = pk->grouped.get();
  if (!gr) return;
  if (gr->sub_col >= 0) { grouped_drop(t, pk); return; }
  buf_free(t, &gr->planes);
  gr->planes.stride = 0; gr->G = 0; gr->pp_serial = 0;
}
// The clustered planes' fields: those of bit-sliced predicate projection `pp` without the grouping column's. false: `pp` has nothing to cluster
// (it lacks the grouping column, or holds no other).
static bool grouped_planes_describe(const vh_table* t, VhGrouped* gr, const VhPredPack* pp) {
  if (!pp || !pp->sliced) return false;
  const size_t at = (size_t)(std::find(pp->cols.begin(), pp->cols.end(), gr->col) - pp->cols.begin());
  if (at >= pp->cols.size() || pp->bitw[at] != gr->bits || pp->bits <= gr->bits || pp->bits > 32) return false;
  gr->G = vh_gplanes_group(pp->bits - gr->bits); gr->goff = pp->bitoff[at];
  gr->planes.stride = vh_gplanes_seg_bytes(t->segment_rows, gr->G);
  gr->pp_serial = pp->serial; gr->pp_cols = pp->cols; gr->pp_bitoff = pp->bitoff; gr->pp_bitw = pp->bitw;
  return true;
}
// The sub-sort of a form whose planes were just described: `sub_col`'s field in the squeezed field word. false: the planes have no such field
// (or it is the grouping column's, or wider than a boundary key) — the form stays in row order inside its runs.
static bool grouped_sub_describe(VhGrouped* gr, const VhPredPack* pp, int sub_col) {
  gr->sub_col = -1; gr->sub_bits = 0; gr->sub_off = 0;
  if (!pp || sub_col < 0 || sub_col == gr->col || !gr->G) return false;
  const size_t at = (size_t)(std::find(pp->cols.begin(), pp->cols.end(), sub_col) - pp->cols.begin());
  if (at >= pp->cols.size() || pp->bitw[at] == 0 || pp->bitw[at] > VH_GSUB_MAX_BITS) return false;
  gr->sub_col = sub_col; gr->sub_bits = pp->bitw[at]; gr->sub_off = vh_gplanes_plane(pp->bitoff[at], gr->goff, gr->bits);
  return true;
}
// Re-derive the tiles that hold a row journalled since the grouped form was last current: whole tiles (one changed row moves the places of
// its tile's rows behind it), one block per tile. When the table grew it starts over in new arenas; no room for records and headers: the
// form is dropped and the ungrouped records answer; no room for the planes: the grouped records alone.
static int grouped_refresh(vh_table* t, VhPack* pk) {
  VhGrouped* gr = pk->grouped.get();
  if (!gr || derived_current(t, *gr)) return VH_OK;
  VhRefresh R;
  R.bufs[0] = &gr->rec; R.bufs[1] = &gr->hdr; R.bufs[2] = &gr->planes; R.nbufs = 3; R.required = 2;
  R.what[0] = VL_NAME[VL_GROUPED]; R.what[1] = VL_NAME[VL_GHDR]; R.what[2] = VL_NAME[VL_GPLANES];
  R.row_limit = rows_padded_256(t); R.whole_tiles = true; R.restart = true;
  const int rc = derived_refresh(t, gr, R, [&](const VhJob* d_jobs, size_t njobs) {
    if (int frc = packflag_ready(t)) return frc;
    grouped_launch(t, pk, d_jobs, njobs, t->d_packflag, g_ctx.stream);
    return (int)VH_OK;
  });
  if (rc == VH_NO_ROOM) { grouped_drop(t, pk); return VH_OK; }
  if (gr->G && !gr->planes.ptr) grouped_no_planes(t, pk);      // (there was no room for the planes; a sub-sorted form goes whole: the launch wrote it in row order)
  return rc;
}
// The grouped form of `pk` by column `col`, whose field in the bit-sliced planes has `bits` bits: built (or built again for another column or
// width) and brought up to date. Bit-field records of 4 bytes only; nullptr and VH_OK where there is no room for it.
// `pp`: the bit-sliced predicate projection whose other columns' bits are kept clustered beside the records (nullptr: records alone — no such
// projection, or no room). A form whose planes belong to another projection than `pp` starts over: records, headers and planes are one launch.
// `sub_col`: the column whose field sub-sorts the runs (-1: none; taken only together with the planes); a form of another sub column starts over.
static int grouped_build(vh_table* t, VhPack* pk, int col, uint32_t bits, const VhPredPack* pp = nullptr, int sub_col = -1) {
  if (!pk->bits || pk->rec_bytes != 4 || bits == 0 || bits > VH_GROUP_MAX_BITS || col < 0 || (size_t)col >= t->cols.size()) return VH_OK;
  if (pk->grouped && (pk->grouped->col != col || pk->grouped->bits != bits || (pp && (!pk->grouped->planes.ptr || pk->grouped->pp_serial != pp->serial)) || pk->grouped->sub_col != (pp ? sub_col : -1))) {
    if (int rc = derived_idle(t)) return rc;
    grouped_drop(t, pk);
  }
  if (!pk->grouped) {
    VhGrouped* gr = new VhGrouped();
    pk->grouped.reset(gr);
    gr->col = col; gr->bits = bits; gr->serial = pk->serial; gr->automatic = pk->automatic;
    const uint64_t tiles = (t->segment_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE;
    gr->rec.stride = pk->rec.stride;
    gr->hdr.stride = (tiles * vh_grouped_hdr_bytes(bits) + 63) / 64 * 64;
    if (grouped_planes_describe(t, gr, pp) && grouped_sub_describe(gr, pp, sub_col)) gr->hdr.stride = vh_gsub_hdr_stride(tiles, bits);
  }
  return grouped_refresh(t, pk);
}

// ------------------------------------------------------- payload projections (vh_table_pack)
static int pack_refresh_records(vh_table* t, VhPack* pk) {
  if (derived_current(t, *pk)) return VH_OK;
  VhRefresh R;
  R.bufs[0] = &pk->rec; R.what[0] = VL_NAME[VL_PACK]; R.nbufs = 1;
  R.row_limit = rows_padded_256(t); R.overflow_wait = pk->compressed;
  return derived_refresh(t, pk, R, [&](const VhJob* d_jobs, size_t njobs) {
    if (int frc = packflag_ready(t)) return frc;
    pack_launch(t, pk, d_jobs, njobs, t->d_packflag, g_ctx.stream);
    return (int)VH_OK;
  });
}
// Bring the projection up to date with the arenas; its grouped form follows in the same call: a plan finds both, and the planes, at one epoch.
static int pack_refresh(vh_table* t, VhPack* pk) {
  if (int rc = pack_refresh_records(t, pk)) return rc;
  return grouped_refresh(t, pk);
}
static void pack_drop(vh_table* t, VhPack* pk) {
  derived_drop(t, &t->packs, pk, [&] { buf_free(t, &pk->rec); grouped_drop(t, pk); });
}
// The projection of exactly these columns (ascending) in this form, or nullptr.
static VhPack* pack_find(const vh_table* t, const std::vector<int>& sorted_cols, bool compressed) {
  for (auto& pk : t->packs) {
    std::vector<int> have = pk->cols;
    std::sort(have.begin(), have.end());
    if (have == sorted_cols && pk->compressed == compressed) return pk.get();
  }
  return nullptr;
}

// The record layout of a projection of `order` (distinct columns): widths (compressed: what the recorded values need), offsets, bit fields.
static int pack_describe(vh_table* t, const std::vector<int>& order, bool automatic, bool compress, std::unique_ptr<VhPack>* out) {
  std::map<int, int> wof;
  for (int c : order) {
    int w = (int)t->cols[c].esize;
    if (compress) if (int rc = column_stored_width(t, c, &w)) return rc;
    wof[c] = w;
  }
  std::vector<int> ord = order;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return wof[a] > wof[b]; });   // widest first: every field naturally aligned
  uint32_t bytes = 0;
  std::vector<uint32_t> off;
  std::vector<uint8_t> width;
  for (int c : ord) { off.push_back(bytes); width.push_back((uint8_t)wof[c]); bytes += (uint32_t)wof[c]; }
  if (bytes > 64) return vh_fail(VH_E_UNSUPPORTED, "vh_table_pack: %u payload bytes per row (max 64)", bytes);
  uint32_t rec = 8;
  while (rec < bytes) rec <<= 1;
  // bit fields instead of bytes when every column is a non-negative integer (by its recorded min / max) and the word comes out smaller
  std::vector<uint8_t> bitoff, bitw;
  bool bits = compress && !test_env("VH_NO_PACK_BITS") && t->nseg > 0;
  uint32_t used = 0;
  for (int c : ord) {
    if (!bits) break;
    VhRange r;
    if (!column_range(t, c, &r)) { bits = false; break; }
    if (r.empty()) r = vh_range_of_zero(t->cols[c].elem);      // no rows yet: as if they held 0 (a later value that needs more voids the projection)
    const int b = vh_range_bits(t->cols[c].elem, r);
    if (!b) { bits = false; break; }
    bitoff.push_back((uint8_t)used); bitw.push_back((uint8_t)b); used += (uint32_t)b;
    if (used > 64) { bits = false; break; }
  }
  const uint32_t rec_bits = used <= 32 ? 4u : 8u;
  if (bits && rec_bits >= rec) bits = false;
  std::unique_ptr<VhPack>& pk = *out;
  pk.reset(new VhPack());
  pk->cols = ord; pk->off = off; pk->width = width; pk->rec_bytes = rec; pk->automatic = automatic; pk->compressed = compress;
  if (bits) { pk->bits = true; pk->bitoff = bitoff; pk->bitw = bitw; pk->rec_bytes = rec = rec_bits; for (auto& o : pk->off) o = 0; }
  pk->rec.stride = rows_padded_256(t) * (uint64_t)rec;
  return VH_OK;
}

static int table_pack_locked(vh_table* t, const int32_t* cols, int32_t ncols, bool automatic, VhPack** out, bool compress) {
  if (!cols || ncols <= 0 || ncols > VH_PACK_MAX_COLS) return vh_fail(VH_E_INVALID, "vh_table_pack: 1..%d columns", VH_PACK_MAX_COLS);
  std::vector<int> order;
  for (int i = 0; i < ncols; ++i) {
    const int c = cols[i];
    if (c < 0 || (size_t)c >= t->cols.size() || is_bitset_elem(t->cols[c].elem)) return vh_fail(VH_E_INVALID, "vh_table_pack: column %d cannot be packed", c);
    if (std::find(order.begin(), order.end(), c) == order.end()) order.push_back(c);
  }
  std::vector<int> sorted_cols = order;
  std::sort(sorted_cols.begin(), sorted_cols.end());
  bool was_pinned = false;
  if (VhPack* pk = pack_find(t, sorted_cols, compress)) {
    const int rc = pack_refresh(t, pk);
    if (rc != VH_PACK_STALE) { if (out) *out = pk; return rc; }
    was_pinned = pk->pinned;
    pack_drop(t, pk);      // built again below, at the widths the values need now (a pin is carried over)
  }
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::unique_ptr<VhPack> pk;
    if (int drc = pack_describe(t, order, automatic, compress, &pk)) return drc;
    pk->serial = ++t->layout_serial; pk->pinned = was_pinned;
    VhPack* raw = pk.get();
    t->packs.push_back(std::move(pk));
    const int rc = pack_refresh(t, raw);
    if (rc == VH_PACK_STALE && attempt == 0) { pack_drop(t, raw); continue; }      // (a metric changed between the min / max pass and the copy)
    if (rc) { pack_drop(t, raw); return rc == VH_PACK_STALE ? vh_fail(VH_E_DEVICE, "vh_table_pack: values keep outgrowing their stored widths") : rc; }
    if (out) *out = raw;
    return VH_OK;
  }
  return VH_OK;
}

// ------------------------------------------------------- narrow predicate copies (vh_table_narrow)
static VhNarrow* narrow_find(const vh_table* t, int col) {
  for (auto& nw : t->narrows) if (nw->col == col) return nw.get();
  return nullptr;
}
// The narrow copy `col` would get; *out stays empty when there is nothing to gain (narrow_width_for).
static void narrow_describe(const vh_table* t, int col, bool automatic, std::unique_ptr<VhNarrow>* out) {
  out->reset();
  const int w = narrow_width_for(t, col);
  if (!w) return;
  out->reset(new VhNarrow());
  (*out)->col = col; (*out)->width = w; (*out)->automatic = automatic;
  (*out)->copy.stride = t->padded_rows * (uint64_t)w;
}
static int narrow_refresh(vh_table* t, VhNarrow* nw) {
  if (derived_current(t, *nw)) return VH_OK;
  VhRefresh R;
  R.bufs[0] = &nw->copy; R.what[0] = VL_NAME[VL_NARROW]; R.nbufs = 1; R.row_limit = t->padded_rows;
  return derived_refresh(t, nw, R, [&](const VhJob* d_jobs, size_t njobs) { narrow_launch(t, nw, d_jobs, njobs, g_ctx.stream); return (int)VH_OK; });
}
static void narrow_drop(vh_table* t, VhNarrow* nw) {
  derived_drop(t, &t->narrows, nw, [&] { buf_free(t, &nw->copy); });
}
// The narrow copy of `col`, fresh, or nullptr (none, or the values no longer fit: the copy is dropped).
static VhNarrow* narrow_usable(vh_table* t, int col) {
  VhNarrow* nw = narrow_find(t, col);
  if (!nw) return nullptr;
  const int w = narrow_width_for(t, col);
  if (w == 0 || w > nw->width) { narrow_drop(t, nw); return nullptr; }
  return narrow_refresh(t, nw) == VH_OK ? nw : nullptr;
}
static int table_narrow_locked(vh_table* t, int col, bool automatic) {
  if (col < 0 || (size_t)col >= t->cols.size()) return vh_fail(VH_E_INVALID, "vh_table_narrow: column %d", col);
  if (narrow_find(t, col)) { (void)narrow_usable(t, col); return VH_OK; }
  std::unique_ptr<VhNarrow> nw;
  narrow_describe(t, col, automatic, &nw);
  if (!nw) return VH_OK;                         // nothing to gain: not an unsigned 32-bit column, or it uses its bits
  nw->serial = ++t->layout_serial;
  VhNarrow* raw = nw.get();
  t->narrows.push_back(std::move(nw));
  const int rc = narrow_refresh(t, raw);
  if (rc) narrow_drop(t, raw);
  return rc;
}

// ------------------------------------------------------- bit-packed predicate projections (vh_table_predpack)
static void predpack_drop(vh_table* t, VhPredPack* pp) {
  derived_drop(t, &t->predpacks, pp, [&] {
    for (int q = 0; q < pp->nplanes; ++q) buf_free(t, &pp->plane[q]);
    for (auto& pk : t->packs)        // clustered planes derived from it go with it (the grouped records stay)
      if (pk->grouped && pk->grouped->pp_serial == pp->serial) grouped_no_planes(t, pk.get());
  });
}
static int predpack_refresh(vh_table* t, VhPredPack* pp) {
  if (derived_current(t, *pp)) return VH_OK;
  VhRefresh R;
  for (int q = 0; q < pp->nplanes; ++q) { R.bufs[q] = &pp->plane[q]; R.what[q] = VL_NAME[VL_PLANE]; }
  R.nbufs = pp->nplanes; R.row_limit = t->padded_rows;
  return derived_refresh(t, pp, R, [&](const VhJob* d_jobs, size_t njobs) { predpack_launch(t, pp, d_jobs, njobs, g_ctx.stream); return (int)VH_OK; });
}
// The projection of exactly `cols` (ascending) in this form, or nullptr.
static VhPredPack* predpack_find(const vh_table* t, const std::vector<int>& cols, bool sliced) {
  for (auto& pp : t->predpacks) if (pp->cols == cols && pp->sliced == sliced) return pp.get();
  return nullptr;
}
// The projection that holds every column of `cols` (ascending), fresh, or nullptr. One whose fields no longer hold the recorded values is dropped.
static VhPredPack* predpack_usable(vh_table* t, const std::vector<int>& cols, int want_sliced = -1) {
  for (auto& q : t->predpacks) {
    VhPredPack* pp = q.get();
    if (!std::includes(pp->cols.begin(), pp->cols.end(), cols.begin(), cols.end())) continue;
    if (want_sliced >= 0 && (int)pp->sliced != want_sliced) continue;
    bool fits = true;
    for (size_t c = 0; c < pp->cols.size(); ++c) { const int b = predpack_bits_for(t, pp->cols[c]); fits &= b > 0 && b <= (int)pp->bitw[c]; }
    if (!fits) { predpack_drop(t, pp); return nullptr; }
    return predpack_refresh(t, pp) == VH_OK ? pp : nullptr;
  }
  return nullptr;
}
// The fields and planes of a predicate projection of `cols`; *out stays empty when there is nothing to gain.
static int predpack_describe(vh_table* t, const std::vector<int>& cols, bool automatic, bool sliced, std::unique_ptr<VhPredPack>* out) {
  std::unique_ptr<VhPredPack> pp(new VhPredPack());
  out->reset();
  uint32_t used = 0, plain = 0;
  for (int c : cols) {
    if (c < 0 || (size_t)c >= t->cols.size()) return vh_fail(VH_E_INVALID, "vh_table_predpack: column %d", c);
    const int b = predpack_bits_for(t, c);
    if (!b) return VH_OK;
    pp->cols.push_back(c); pp->bitoff.push_back((uint8_t)used); pp->bitw.push_back((uint8_t)b);
    used += (uint32_t)b;
    const int nwid = narrow_width_for(t, c);
    plain += nwid ? (uint32_t)nwid : (uint32_t)t->cols[c].esize;
  }
  if (used > 32) return VH_OK;
  if (sliced) {          // `used` planes of one bit per row; a plane's share of a segment padded to whole 256-byte blocks
    pp->sliced = true; pp->bits = used;
    pp->pitch = (t->padded_rows / 8 + 255) / 256 * 256;
    pp->nplanes = 1; pp->pwidth[0] = 0; pp->ppos[0] = 0; pp->plane[0].stride = pp->pitch * used;
    if (used >= plain * 8u) return VH_OK;
  } else {
    for (uint32_t left = used, pos = 0; left > 0;) {
      const int w = left > 8 ? 2 : 1;
      pp->pwidth[pp->nplanes] = w; pp->ppos[pp->nplanes] = (int)pos; pp->plane[pp->nplanes].stride = t->padded_rows * (uint64_t)w;
      ++pp->nplanes;
      pos += 8u * w; left = left > 8u * w ? left - 8u * w : 0;
    }
    if (pp->bytes_per_row() >= plain) return VH_OK;
  }
  pp->automatic = automatic;
  *out = std::move(pp);
  return VH_OK;
}
// Build one for `cols` (ascending, distinct). *built = nullptr when there is nothing to gain: a column that is no non-negative integer,
// more than 32 bits in all, or no fewer bytes per row than the columns' narrowest copies would take.
static int table_predpack_locked(vh_table* t, const std::vector<int>& cols, bool automatic, VhPredPack** built, bool sliced) {
  if (built) *built = nullptr;
  if (cols.empty() || cols.size() > VH_PACK_MAX_COLS || cols.size() > VJ_MAX_PRED) return VH_OK;
  if (predpack_find(t, cols, sliced)) { if (built) *built = predpack_usable(t, cols, sliced ? 1 : 0); return VH_OK; }
  std::unique_ptr<VhPredPack> pp;
  if (int drc = predpack_describe(t, cols, automatic, sliced, &pp)) return drc;
  if (!pp) return VH_OK;
  pp->serial = ++t->layout_serial;
  VhPredPack* raw = pp.get();
  t->predpacks.push_back(std::move(pp));
  const int rc = predpack_refresh(t, raw);
  if (rc) { predpack_drop(t, raw); return rc; }
  if (built) *built = raw;
  return VH_OK;
}

extern "C" int vh_table_predpack(vh_table* t, const int32_t* cols, int32_t ncols) { return vh_table_predpack_ex(t, cols, ncols, VH_PREDPACK_AUTO); }
extern "C" int vh_table_predpack_ex(vh_table* t, const int32_t* cols, int32_t ncols, uint32_t form) {
  if (!t || !cols || ncols <= 0) return vh_fail(VH_E_INVALID, "vh_table_predpack: null argument");
  if (form > VH_PREDPACK_SLICED) return vh_fail(VH_E_INVALID, "vh_table_predpack_ex: form %u", form);
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  if (int src = sync_resolve(t)) return src;
  std::vector<int> set(cols, cols + ncols);
  std::sort(set.begin(), set.end());
  set.erase(std::unique(set.begin(), set.end()), set.end());
  const bool sliced = form == VH_PREDPACK_AUTO ? !knobs().predpack_bytes : form == VH_PREDPACK_SLICED;
  const int rc = table_predpack_locked(t, set, false, nullptr, sliced);
  if (VhPredPack* pp = rc ? nullptr : predpack_find(t, set, sliced)) pp->pinned = true;      // asked for by name: the budget never evicts it
  derived_trim(t, false);
  return rc;
}

extern "C" int vh_table_narrow(vh_table* t, const int32_t* cols, int32_t ncols) {
  if (!t || (!cols && ncols)) return vh_fail(VH_E_INVALID, "null argument");
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  if (int src = sync_resolve(t)) return src;
  int rc = VH_OK;
  for (int i = 0; i < ncols && !rc; ++i) {
    rc = table_narrow_locked(t, cols[i], false);
    if (VhNarrow* nw = rc ? nullptr : narrow_find(t, cols[i])) nw->pinned = true;
  }
  derived_trim(t, false);
  return rc;
}

extern "C" int vh_table_pack_ex(vh_table* t, const int32_t* cols, int32_t ncols, uint32_t form) {
  if (!t) return vh_fail(VH_E_INVALID, "null table");
  if (form > VH_PACK_COMPRESSED) return vh_fail(VH_E_INVALID, "vh_table_pack_ex: form %u", form);
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  if (int src = sync_resolve(t)) return src;
  // VH_PACK_AUTO: compressed where the per-query compiled kernels — the only readers of compressed records — would run a scan of the
  // whole table (VH_JIT=force, or auto and the table holds VH_JIT_MIN_ROWS rows); plain where the pre-built kernels answer
  bool compress = form == VH_PACK_COMPRESSED;
  if (form == VH_PACK_AUTO) {
    uint64_t rows = 0;
    for (uint32_t s = 0; s < t->nseg; ++s) rows += t->seg_rows[s];
    compress = !knobs().pack_plain && (vh_jit_policy() == VH_JIT_FORCE || (vh_jit_policy() == VH_JIT_AUTO && rows >= vh_jit_min_rows()));
  }
  VhPack* built = nullptr;
  const int rc = table_pack_locked(t, cols, ncols, false, &built, compress);
  if (!rc && built) built->pinned = true;
  derived_trim(t, false);
  return rc;
}
extern "C" int vh_table_pack(vh_table* t, const int32_t* cols, int32_t ncols) { return vh_table_pack_ex(t, cols, ncols, VH_PACK_AUTO); }

// Room for `need` more bytes under the rule every automatic layout is built by: a quarter of the device stays free. device_mem: the two
// figures, for the sites that weigh something else against them (false: the device does not say).
static bool device_mem(size_t* free_b, size_t* total_b) {
  if (hipMemGetInfo(free_b, total_b) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}
static bool device_room(size_t need) {
  size_t free_b = 0, total_b = 0;
  return device_mem(&free_b, &total_b) && free_b > need + total_b / 4;
}

// ------------------------------------------------------- lifetimes: a byte budget, LRU eviction, pins, the listing
// The layouts above are built unasked and nothing but staleness ever dropped them: a workload of many query shapes filled the device to the
// 3/4 mark of device_room and every later shape stayed on the arenas. vh_table::layout_budget bounds what they hold together —
// "layout bytes": every arena derived_each(VL_ALL) visits plus the background job's arenas in flight (build_reserved); the column arenas
// are not part of it. Every plan stamps what it reads (layout_use, vhh_build.h); an automatic build that would pass the budget first evicts
// unpinned layouts, least recently used first (derived_make_room), or is declined when even all of them would not make room. Pinned
// layouts — built by an explicit call or read by a prepared plan — never leave this way and may exceed the budget by themselves. An eviction
// is the kind's own drop function: derived_drop waits until nobody reads the arenas. With no budget none of this does anything.
static thread_local int g_plan_depth = 0;                       // query_launch_locked calls on this thread's stack (a plan that starts over is the same query)
static thread_local bool g_plan_evicted = false;                // this thread's query evicted a layout while it was planned (vh_result_info.reserved bit 24)
static thread_local bool g_plan_carry = false;                  // ... in a pass that belongs to a query whose result comes later (a sharded query's summary pass): carried to that result
static thread_local bool g_plan_unstamped = false;              // the plan being made is a further pass of a query already counted (summary pass, heavy second pass): it holds what it reads, `uses` do not move
static thread_local std::vector<uint64_t> g_prepare_reads;      // vh_table_prepare: serials of the layouts its last query read
static thread_local std::vector<uint64_t> g_prepare_pinned;     // ... and of the layouts it pinned itself, as its queries stamped them (unpinned again where it fails, or where its last query no longer reads them)
struct VhLayoutRef {         // one layout as the policy and the listing see it: a projection with its grouped form, a predicate projection with all planes, a narrow copy
  int kind; VhLayout* L; VhPack* pk; VhPredPack* pp; VhNarrow* nw; uint64_t bytes, grouped_bytes;
};
static void layout_refs(vh_table* t, std::vector<VhLayoutRef>* out) {
  for (auto& q : t->packs) {
    const VhGrouped* gr = q->grouped.get();
    const uint64_t g = gr ? gr->rec.held + gr->hdr.held + gr->planes.held : 0;
    out->push_back(VhLayoutRef{VH_LAYOUT_PROJECTION, q.get(), q.get(), nullptr, nullptr, q->rec.held + g, g});
  }
  for (auto& q : t->predpacks) {
    uint64_t b = 0;
    for (int k = 0; k < q->nplanes; ++k) b += q->plane[k].held;
    out->push_back(VhLayoutRef{q->sliced ? VH_LAYOUT_PRED_SLICED : VH_LAYOUT_PRED_BYTES, q.get(), nullptr, q.get(), nullptr, b, 0});
  }
  for (auto& q : t->narrows) out->push_back(VhLayoutRef{VH_LAYOUT_NARROW, q.get(), nullptr, nullptr, q.get(), q->copy.held, 0});
  std::sort(out->begin(), out->end(), [](const VhLayoutRef& a, const VhLayoutRef& b) { return a.L->serial < b.L->serial; });
}
// Bytes the arenas `which` names hold (derived_each's sets: 1 projections, 2 predicate planes — vh_table_relocate's bits —, VL_ALL every arena:
// the figure the layout budget bounds, with vh_table::build_reserved).
static size_t derived_bytes(vh_table* t, uint32_t which) {
  size_t b = 0;
  derived_each(t, which == VL_ALL ? (uint32_t)VL_ALL : which & 3u, [&](int, VhLayout&, int, VhBuf& buf) { b += buf.held; });
  return b;
}
static std::string cols_key(std::vector<int> cols) {
  std::sort(cols.begin(), cols.end());
  std::string k;
  for (int c : cols) { k += std::to_string(c); k.push_back(','); }
  return k;
}
// `v` leaves through its kind's drop function. `evicted`: by the budget — the shape's sightings start again (VH_AUTO_* fresh ones before it is
// built once more: no thrashing), the counters move, VH_TIMES says what the wait for its readers and the frees took.
static void layout_drop(vh_table* t, const VhLayoutRef& v, bool evicted) {
  const bool timed = evicted && knobs().times;
  const auto t0 = timed ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
  const uint64_t serial = v.L->serial, bytes = v.bytes;
  if (v.pk) {
    const std::string k = cols_key(v.pk->cols), g = "g:" + std::to_string(serial) + ":";
    t->gather_seen.erase("c:" + k); t->gather_seen.erase("p:" + k);
    for (auto it = t->gather_seen.lower_bound(g); it != t->gather_seen.end() && it->first.compare(0, g.size(), g) == 0;) it = t->gather_seen.erase(it);
    t->build_nothing.erase("p:0:" + k); t->build_nothing.erase("p:1:" + k);
    pack_drop(t, v.pk);
  } else if (v.pp) {
    const std::string k = cols_key(v.pp->cols);
    t->ppred_seen.erase((v.pp->sliced ? "s:" : "b:") + k);
    t->build_nothing.erase((v.pp->sliced ? "q:1:" : "q:0:") + k);
    predpack_drop(t, v.pp);
  } else {
    t->pred_seen.erase(v.nw->col);
    t->build_nothing.erase("n:0:" + std::to_string(v.nw->col) + ",");
    narrow_drop(t, v.nw);
  }
  if (!evicted) return;
  ++t->evictions; t->evicted_bytes += bytes;
  g_plan_evicted = true;
  if (timed) fprintf(stderr, "vh evict: %s %llu, %llu bytes, in %.3f ms (the wait for its readers and the frees)\n", v.kind == VH_LAYOUT_PROJECTION ? "projection" : v.kind == VH_LAYOUT_NARROW ? "narrow copy" : "predicate projection",
                     (unsigned long long)serial, (unsigned long long)bytes, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}
// Evict until `deficit` bytes are free. in_plan: what the plan of the current tick holds stays. all_or_nothing: where even every candidate
// would not cover the deficit, nothing leaves and the answer is false; otherwise every candidate leaves then.
static bool layout_evict(vh_table* t, uint64_t deficit, bool in_plan, bool all_or_nothing, const VhLayout* keep1 = nullptr, const VhLayout* keep2 = nullptr) {
  std::vector<VhLayoutRef> refs;
  layout_refs(t, &refs);
  std::vector<VhEvictEntry> e;
  uint64_t can = 0;
  for (const VhLayoutRef& v : refs) {
    const bool ok = !v.L->pinned && !(in_plan && v.L->held_tick == t->use_tick) && v.L != keep1 && v.L != keep2;
    e.push_back(VhEvictEntry{v.bytes, v.L->last_use, v.L->serial, ok});
    if (ok) can += v.bytes;
  }
  std::vector<size_t> victims;
  bool fits = vh_evict_pick(e.data(), e.size(), deficit, &victims);
  if (!fits && all_or_nothing) return false;
  if (!fits) (void)vh_evict_pick(e.data(), e.size(), can, &victims);
  for (size_t i : victims) layout_drop(t, refs[i], true);
  return fits;
}
// (t->mu held) An automatic build is about to take `need` more bytes: true — they fit the budget, after evictions where it took some; false —
// they do not, and nothing was evicted. keep1 / keep2: layouts the build is made for (a grouped form's projection and planes), whatever
// their stamps; credit: bytes the build itself gives back first (the grouped form it replaces).
static bool derived_make_room(vh_table* t, uint64_t need, const VhLayout* keep1 = nullptr, const VhLayout* keep2 = nullptr, uint64_t credit = 0) {
  if (!t->layout_budget) return true;
  const uint64_t have = derived_bytes(t, VL_ALL) + t->build_reserved;
  const uint64_t after = have - std::min(have, credit) + need;
  if (after <= t->layout_budget) return true;
  return layout_evict(t, after - t->layout_budget, true, true, keep1, keep2);
}
static void derived_trim(vh_table* t, bool in_plan) {
  if (!t->layout_budget) return;
  const uint64_t have = derived_bytes(t, VL_ALL) + t->build_reserved;
  if (have > t->layout_budget) (void)layout_evict(t, have - t->layout_budget, in_plan, false);
}

extern "C" int vh_table_set_layout_budget(vh_table* t, uint64_t bytes) {
  if (!t) return vh_fail(VH_E_INVALID, "vh_table_set_layout_budget: null table");
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  t->layout_budget = bytes;
  derived_trim(t, false);
  return VH_OK;
}
extern "C" int vh_table_layouts(vh_table* t, vh_layout_info* out, uint32_t cap, uint32_t* n, vh_layout_summary* sum) {
  if (!t) return vh_fail(VH_E_INVALID, "vh_table_layouts: null table");
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  if (!n || (cap && !out)) return vh_fail(VH_E_INVALID, "vh_table_layouts: null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  std::vector<VhLayoutRef> refs;
  layout_refs(t, &refs);
  *n = (uint32_t)refs.size();
  uint64_t pinned_bytes = 0;
  for (size_t i = 0; i < refs.size(); ++i) {
    const VhLayoutRef& v = refs[i];
    if (v.L->pinned) pinned_bytes += v.bytes;
    if (!out || i >= cap) continue;
    vh_layout_info& o = out[i];
    o = vh_layout_info{};
    o.serial = v.L->serial; o.kind = v.kind;
    const std::vector<int> one = v.nw ? std::vector<int>{v.nw->col} : std::vector<int>();
    const std::vector<int>& cols = v.pk ? v.pk->cols : v.pp ? v.pp->cols : one;
    o.ncols = (int32_t)cols.size();
    for (size_t c = 0; c < cols.size() && c < VH_LAYOUT_COLS; ++c) o.cols[c] = cols[c];
    o.bytes = v.bytes; o.grouped_bytes = v.grouped_bytes;
    const VhGrouped* gr = v.pk ? v.pk->grouped.get() : nullptr;
    o.flags = (v.L->automatic ? 1u : 0) | (v.L->pinned ? 2u : 0) | (v.L->applied_epoch == t->sync_epoch ? 4u : 0) | (v.pk && v.pk->compressed ? 8u : 0) |
              (v.pk && v.pk->bits ? 16u : 0) | (gr && gr->rec.ptr ? 32u : 0) | (gr && gr->planes.ptr ? 64u : 0);
    o.uses = v.L->uses; o.last_use = v.L->last_use;
  }
  if (sum) {
    *sum = vh_layout_summary{};
    sum->budget = t->layout_budget; sum->bytes = derived_bytes(t, VL_ALL); sum->pinned_bytes = pinned_bytes; sum->reserved_bytes = t->build_reserved;
    sum->tick = t->use_tick; sum->evictions = t->evictions; sum->evicted_bytes = t->evicted_bytes; sum->declined = t->declined;
  }
  return VH_OK;
}
static bool layout_by_serial(vh_table* t, uint64_t serial, VhLayoutRef* out) {
  std::vector<VhLayoutRef> refs;
  layout_refs(t, &refs);
  for (const VhLayoutRef& v : refs) if (v.L->serial == serial) { *out = v; return true; }
  return false;
}
extern "C" int vh_table_layout_pin(vh_table* t, uint64_t serial, int32_t pinned) {
  if (!t) return vh_fail(VH_E_INVALID, "vh_table_layout_pin: null table");
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  VhLayoutRef v;
  if (!layout_by_serial(t, serial, &v)) return vh_fail(VH_E_INVALID, "vh_table_layout_pin: no layout %llu", (unsigned long long)serial);
  v.L->pinned = pinned != 0;      // (unpinned over the budget, it is the next query's to evict: nothing leaves inside this call)
  return VH_OK;
}
extern "C" int vh_table_layout_drop(vh_table* t, uint64_t serial) {
  if (!t) return vh_fail(VH_E_INVALID, "vh_table_layout_drop: null table");
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  VH_ENTER();
  std::lock_guard<std::mutex> lk(t->mu);
  VhLayoutRef v;
  if (!layout_by_serial(t, serial, &v)) return vh_fail(VH_E_INVALID, "vh_table_layout_drop: no layout %llu", (unsigned long long)serial);
  layout_drop(t, v, false);
  return VH_OK;
}

// WHERE the derived layouts lie. The same records and planes read by the same kernel take 1.07 or 1.23 ms per 1 B rows depending on the physical
// pages they were given (profiles/r06/NOTES.md, "Placement": six execution contexts with six scratch allocations agree within 0.5 %, the
// projection alone moved twenty-three times changes nothing, projection AND planes re-built behind 3 GB spacers spread over 15 % — all at
// 2 MB-aligned virtual addresses, so it is nothing a process can compute). What a process can do is try: derived_move copies every layout `which`
// names (1: projections, 2: predicate planes) to FRESH allocations while the old ones are still held — so that the new ones are other pages —
// and swaps the pointers (kernels take addresses as arguments); the caller measures and keeps or gives back (vh_table_prepare, vh_table_relocate).
struct VhMoved {       // an arena of derived_each's `kind` (the grouped headers stay: 32 bytes a tile), `plane` of its layout; `serial` and `applied_epoch` of the layout at the move
  int kind; uint64_t serial, applied_epoch; int plane; char* old_ptr; char* new_ptr; size_t bytes;
};
static int derived_move(vh_table* t, uint32_t which, std::vector<VhMoved>* moved) {      // (t->mu held)
  if (int irc = derived_idle(t)) return irc;
  int rc = VH_OK;
  derived_each(t, which & 3u, [&](int kind, VhLayout& L, int plane, VhBuf& buf) {
    if (rc) return;
    char* nb = nullptr;
    if (hipMalloc(&nb, buf.held) != hipSuccess) { (void)hipGetLastError(); rc = VH_E_NOMEM; return; }
    trace_alloc(VL_NAME[kind], nb, buf.held);
    if (hipMemcpyAsync(nb, buf.ptr, buf.held, hipMemcpyDeviceToDevice, g_ctx.stream) != hipSuccess) { (void)hipFree(nb); rc = vh_fail(VH_E_DEVICE, "moving a derived layout"); return; }
    moved->push_back(VhMoved{kind, L.serial, L.applied_epoch, plane, buf.ptr, nb, buf.held});
    buf.ptr = nb;
  });
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  return rc == VH_E_NOMEM ? VH_OK : rc;          // (out of memory: what could be moved was moved)
}
// The buffers a move left behind (keep = true), or the ones it made after the layouts were pointed back at the old ones (keep = false), into
// `out` — still allocated: whoever tries several places frees them all at the end, so that no candidate lands on a place already tried.
// The caller dropped t->mu between the move and this call (vh_table_prepare measures with queries of its own), so the layout may have changed:
// - it is found by its serial, not by its address: a projection dropped and rebuilt meanwhile (a synced value outgrew it) can come back at the
//   same host address AND be given the device address just freed — its new widths would then be paired with the old buffer;
// - it must still hold new_ptr: another prepare or relocate may have moved it on (then new_ptr is that one's old buffer, settled by that one);
// - it goes back to old_ptr only if nothing was refreshed since the move: a sync that landed meanwhile was re-derived into new_ptr alone, and
//   the old buffer would be stale under an applied_epoch that says current. Then the new buffer stays, whatever the verdict.
// Exactly one of the two buffers is ours to free: new_ptr where the layout goes back, old_ptr otherwise — where the layout was dropped, grew
// or moved on, whoever replaced new_ptr owns it (and freed it, or will settle it).
static void derived_settle(vh_table* t, std::vector<VhMoved>& moved, bool keep, std::vector<char*>* out) {      // (t->mu held)
  (void)derived_idle(t);
  for (const VhMoved& m : moved) {
    char** slot = nullptr;
    uint64_t applied = 0;
    derived_each(t, 3u, [&](int kind, VhLayout& L, int plane, VhBuf& buf) {
      if (kind == m.kind && L.serial == m.serial && plane == m.plane && buf.ptr == m.new_ptr) { slot = &buf.ptr; applied = L.applied_epoch; }
    });
    if (slot && !keep && applied == m.applied_epoch) { *slot = m.old_ptr; out->push_back(m.new_ptr); }
    else out->push_back(m.old_ptr);
  }
  moved.clear();
}
extern "C" int vh_table_relocate(vh_table* t, uint32_t which) {
  if (!t) return vh_fail(VH_E_INVALID, "null table");
  VH_ENTER();
  std::vector<char*> drop;
  {
    std::lock_guard<std::mutex> lk(t->mu);
    if (int src = sync_resolve(t)) return src;
    std::vector<VhMoved> moved;
    if (int rc = derived_move(t, which ? which : 3u, &moved)) { derived_settle(t, moved, false, &drop); for (char* p : drop) (void)hipFree(p); return rc; }
    derived_settle(t, moved, true, &drop);
  }
  for (char* p : drop) (void)hipFree(p);
  return VH_OK;
}

extern "C" int vh_table_unpack(vh_table* t) {
  if (!t) return vh_fail(VH_E_INVALID, "null table");
  VH_ENTER();
  build_cancel_table(t, false);      // (before the lock: the running job needs it to finish; what it publishes meanwhile is dropped below)
  std::lock_guard<std::mutex> lk(t->mu);
  if (int src = sync_resolve(t)) return src;
  if (int rc = derived_idle(t)) return rc;
  derived_each(t, VL_ALL, [&](int, VhLayout&, int, VhBuf& b) { buf_free(t, &b); });
  t->packs.clear(); t->gather_seen.clear();
  t->narrows.clear(); t->pred_seen.clear();
  t->predpacks.clear(); t->ppred_seen.clear();
  return VH_OK;
}
