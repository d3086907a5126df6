// vhh_launch.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// QueryBuild continued: kernel compile, scan dispatch, work decomposition, scratch layout, launch; query_launch_locked.
// Adds a dense result's private copies (one per XCD, or one per block of a partition's range) into copy 0.
static void merge_args_of(const vh_result* r, VhMergeArgs* A) {
  const VhPlanDev& P = r->plan;
  *A = VhMergeArgs{};
  A->nmetric = P.nmetric; A->nxcd = r->nxcd; A->G = P.G; A->xcd_stride = P.xcd_stride; A->present = P.present;
  A->present_carrier = P.present_carrier;
  for (int j = 0; j < P.nmetric; ++j) { A->state[j] = P.m[j].state; A->sop[j] = P.m[j].sop(); }
  if (P.part_count && P.nlevel == 1) { A->part_count = P.part_count; A->npart = P.npart; A->agg_shift = P.agg_shift; A->blocks = r->part_blocks; }
}
static int merge_copies_now(vh_result* r, hipStream_t st) {
  if (!r->unmerged) return VH_OK;
  VhMergeArgs A;
  merge_args_of(r, &A);
  hipLaunchKernelGGL(dense_merge_kernel, dim3((unsigned)((r->plan.G + 255) / 256)), dim3(256), 0, st, A);
  HIP_TRY(hipGetLastError());
  r->unmerged = false;
  r->tail.merged = VH_MERGE_KERNEL;
  return VH_OK;
}

// A compiled scan ran (or will run) without the predicate projection that serves its form: count the query; at the VH_AUTO_NARROW-th one
// (the first, inside vh_table_prepare) build it for the queries to come, memory permitting. Only where kernels get compiled at all.
void QueryBuild::predpack_auto(bool want_sliced) {
  const int auto_after = g_preparing ? 1 : knobs().auto_narrow;
  if (pp_cols.empty() || auto_after <= 0 || g_build_quiet) return;
  uint64_t rows = 0;
  for (uint32_t sgi = 0; sgi < t->nseg; ++sgi) rows += t->seg_rows[sgi];
  if (!(vh_jit_policy() == VH_JIT_FORCE || (p->flags & VH_PLAN_FORCE_JIT) || rows >= vh_jit_min_rows())) return;
  const bool sliced = want_sliced && !knobs().predpack_bytes;
  if (predpack_find(t, pp_cols, sliced)) return;
  std::string key = sliced ? "s:" : "b:";
  for (int c : pp_cols) { key += std::to_string(c); key.push_back(','); }
  if (++t->ppred_seen[key] < (uint32_t)auto_after) return;
  if (build_background(t)) { build_pending |= build_request_layout(t, VB_PREDPACK, pp_cols, sliced, true, key, p); return; }      // (the worker builds it and evaluates the guard)
  const size_t need = (size_t)t->cap_seg * t->padded_rows * 4;
  const size_t had = t->predpacks.size();
  uint64_t exact = 0;
  if (t->layout_budget) {      // the budget is asked for the bytes the planes will really take (nothing to gain: nothing is built, nothing asked)
    std::unique_ptr<VhPredPack> d;
    if (predpack_describe(t, pp_cols, true, sliced, &d) == VH_OK && d) for (int q = 0; q < d->nplanes; ++q) exact += VhBuf::bytes(t->cap_seg, d->plane[q].stride);
  }
  if ((!exact || budget_room(exact)) && device_room(need)) { (void)table_predpack_locked(t, pp_cols, true, nullptr, sliced); t->inline_builds += t->predpacks.size() > had; }
  else t->ppred_seen[key] = 0;
}

// Grouped payload records (vh_grouped.h). A plan takes them when
//   * it runs the compiled bit-sliced compacting scan (no lanes form, no streamed payload),
//   * every group and metric value is a field of ONE 4-byte bit record of a projection (nothing else is gathered: no row id, no bitset),
//   * the filter's top-level AND has exactly one `==` leaf on some column whose field in the planes has at most VH_GROUP_MAX_BITS bits — the
//     first such column in program order is the grouping column —
// and the projection's grouped form by that column exists at the planes' epoch. Where the automatic layouts are built (vh_table_prepare, or the
// VH_AUTO_PACK-th query of the shape; on a background-build table by the worker, see vhh_build.h) it is built under the same
// "leaves a quarter of the device free" rule — on a table of VH_SUBSORT_MIN_ROWS rows SUB-SORTED by the column of the filter's first range
// leaf, whose runs the scan then trims (see below). VH_PLAN_NO_GROUPED keeps the ungrouped records: an A/B inside one process.
#define VH_SUBSORT_MIN_ROWS (4ull << 20)      // rows a table must hold before a grouped form built for it is sub-sorted
void QueryBuild::choose_grouped() {
  VhJitShape& js = jshape;
  if ((p->flags & VH_PLAN_NO_GROUPED) || !js.pp_sliced || lanes || js.qpay || !packed || !packed_use || !sliced_use || !packed_bits || packed_rec != 4 || P.nbitset) return;
  for (int i = 0; i < P.ngroup; ++i) if (slot_rec[P.g[i].slot()] != 0 || slot_bits[P.g[i].slot()] != 4) return;
  for (int j = 0; j < P.nmetric; ++j) if (metric_col[j] < 0 || P.m[j].slot() == VH_SLOT_ROWID || slot_rec[P.m[j].slot()] != 0 || slot_bits[P.m[j].slot()] != 4) return;
  // the leaves of the top-level conjunction (a wide AND was folded pairwise: nested ANDs are the same conjunction)
  const std::vector<VhProgOp>& g = js.prog;
  if (g.empty() || g.back().kind() != VH_F_AND) return;
  std::vector<int> leaves;
  {
    std::vector<int> sub(g.size(), 1);         // size of the subtree that ends at node k
    for (size_t k = 0; k < g.size(); ++k)
      if (g[k].kind() == VH_F_AND || g[k].kind() == VH_F_OR) { int at = (int)k - 1; for (int c = 0; c < (int)g[k].count() && at >= 0; ++c) { sub[k] += sub[at]; at -= sub[at]; } }
    std::vector<int> todo{(int)g.size() - 1};
    while (!todo.empty()) {
      const int k = todo.back(); todo.pop_back();
      if (g[k].kind() != VH_F_AND) { leaves.push_back(k); continue; }
      int at = k - 1;
      for (int c = 0; c < (int)g[k].count() && at >= 0; ++c) { todo.push_back(at); at -= sub[at]; }
    }
    std::sort(leaves.begin(), leaves.end());
  }
  int eq_leaves[VJ_MAX_PRED] = {}, leaf_of[VJ_MAX_PRED];
  for (int k : leaves) if (g[k].kind() == VH_F_REL && g[k].op() == VH_OP_EQ && (int)g[k].pslot() < js.npred) { if (!eq_leaves[g[k].pslot()]++) leaf_of[g[k].pslot()] = k; }
  int gp = -1;
  for (int k : leaves) {
    if (g[k].kind() != VH_F_REL || g[k].op() != VH_OP_EQ) continue;
    const int ps = (int)g[k].pslot();
    if (ps < js.npred && eq_leaves[ps] == 1 && js.pp_bits[ps] >= 1 && js.pp_bits[ps] <= VH_GROUP_MAX_BITS && jit_pred_col[ps] >= 0) { gp = ps; break; }
  }
  if (gp < 0 || P.nslots >= VH_MAX_SLOTS) return;
  const int gcol = jit_pred_col[gp];
  const uint32_t gbits = (uint32_t)js.pp_bits[gp];
  VhGrouped* gr = packed_use->grouped.get();
  // The SUB column (vh_grouped.h): the column of the first leaf of the conjunction, in program order, that is a relation a run can be trimmed
  // by (LT, LE, GT, GE, EQ) on a field of the planes other than the grouping column's, of at most VH_GSUB_MAX_BITS bits. A form built now is
  // sub-sorted by it where the table holds VH_SUBSORT_MIN_ROWS rows (below that both paths are launch-bound, and the sub-sorted form gives up
  // the records-only readers) — VH_TEST_SUBSORT=1 / 0 forces it on / off — and only together with its planes.
  int sp = -1, sp_leaf = -1;
  for (int k : leaves) {
    if (g[k].kind() != VH_F_REL || !vh_gsub_op_ok((int)g[k].op())) continue;
    const int ps = (int)g[k].pslot();
    if (ps < js.npred && ps != gp && jit_pred_col[ps] >= 0 && js.pp_bits[ps] >= 1 && js.pp_bits[ps] <= (int)VH_GSUB_MAX_BITS) { sp = ps; sp_leaf = k; break; }
  }
  const int scol = sp >= 0 ? jit_pred_col[sp] : -1;
  const char* const sub_hook = test_env("VH_TEST_SUBSORT");
  int sub_want = -1;
  if (scol >= 0 && sliced_use->bits > gbits) {
    uint64_t rows = 0;
    for (uint32_t s = 0; s < t->nseg; ++s) rows += t->seg_rows[s];
    if (sub_hook ? atoi(sub_hook) != 0 : rows >= VH_SUBSORT_MIN_ROWS) sub_want = scol;
  }
  // the form is built where it is missing, is another column's, or lacks the clustered planes of the bit-sliced projection this plan reads
  // (that projection was dropped and described again since): records, headers and planes come out of one launch, so it starts over
  const bool other = gr && (gr->col != gcol || gr->bits != gbits);
  const bool bare = gr && !other && sliced_use->bits > gbits && (!gr->planes.ptr || gr->pp_serial != sliced_use->serial);
  // (one form per projection: a form sub-sorted by another column, or by none, serves this plan without trimming; only a prepared plan has it
  // built again for its own sub column — or, under the hook that forces the sub-sort off, without one)
  const bool resub = gr && !other && !bare && g_preparing && gr->sub_col != sub_want && (sub_want >= 0 || (sub_hook && !atoi(sub_hook)));
  auto build = [&]() {
    const int auto_after = g_preparing ? 1 : knobs().auto_pack;
    if (auto_after <= 0) return;
    if (other && !g_preparing) return;         // (one grouped form per projection: only a prepared plan replaces another column's)
    const std::string sig = "g:" + std::to_string(packed_use->serial) + ":" + std::to_string(gcol) + (bare ? ":" + std::to_string(sliced_use->serial) : std::string()) + (resub ? ":s" + std::to_string(sub_want) : std::string());
    // background build mode: the worker's own query (build_warm), run because the layouts this plan's sightings asked for now exist, builds the
    // form here, off every caller's path; a caller's query that finds projection and planes without it asks for a job after its own sightings
    const bool bg = build_background(t), own = bg && g_build_worker;
    if (!own) {
      if (g_build_quiet) return;
      if (++t->gather_seen[sig] < (uint32_t)auto_after) return;
      if (bg) { build_pending |= build_request_grouped(t, packed_use->serial, sliced_use->serial, gcol, gbits, sub_want, sig, p); return; }
    }
    const int room = grouped_room(t, packed_use, sliced_use, gbits, sub_want >= 0);
    if (!room || ((bare || resub) && room < 2)) { t->gather_seen[sig] = 0; return; }      // (a form that lacks only its planes, or its sub-sort, is kept where there is no room for them)
    if (grouped_build(t, packed_use, gcol, gbits, room == 2 ? sliced_use : nullptr, room == 2 ? sub_want : -1) != VH_OK) { (void)hipGetLastError(); return; }
    if (!bg) ++t->inline_builds;
  };
  if (!gr || other || bare || resub) {
    build();
    gr = packed_use->grouped.get();
    if (!gr || gr->col != gcol || gr->bits != gbits) return;
  }
  // as current as the planes whose bits give the places, and as the table: anything else is a stale layout
  if (!gr->rec.ptr || !gr->hdr.ptr || gr->applied_epoch != t->sync_epoch || sliced_use->applied_epoch != t->sync_epoch || packed_use->applied_epoch != t->sync_epoch) return;
  // Whether the plan reads the CLUSTERED planes is settled first: a sub-sorted form can be read through them alone (a place follows from no
  // row-order formula there), so a plan that may not — VH_PLAN_NO_GPLANES, a second leaf on the grouping column, a snapshot that cuts into a
  // built tile — leaves the form alone and gathers the ungrouped records of the projection, which always exist.
  bool planes_ok = !(p->flags & VH_PLAN_NO_GPLANES) && gr->planes.ptr && gr->G && gr->pp_serial == sliced_use->serial && P.nslots + 1 < VH_MAX_SLOTS;
  if (planes_ok) {
    int reads = 0;
    for (const VhProgOp& o : g) if (o.kind() != VH_F_AND && o.kind() != VH_F_OR && o.kind() != VH_F_TRUE && (int)o.pslot() == gp) ++reads;
    planes_ok = reads == 1;
  }
  for (uint32_t s = 0; s < nseg && planes_ok; ++s) if (x->h_segrows[s] != (uint32_t)t->seg_rows[s] && x->h_segrows[s] % VH_GROUP_TILE != 0) planes_ok = false;
  if (gr->sub_col >= 0 && !planes_ok) return;
  for (int s = 0; s < P.nslots; ++s) if (slot_rec[s] == 0 && slot_bits[s] == 4) P.colbase[s] = gr->rec.ptr;      // (a bit record's members all start at the record)
  P.colbase[P.nslots] = gr->hdr.ptr; P.colstride[P.nslots] = gr->hdr.stride; P.colpitch[P.nslots] = vh_grouped_hdr_bytes(gbits);
  js.pp_group = gp; js.pp_group_hdr = P.nslots++; js.pp_group_lit = (int)g[leaf_of[gp]].lit();
  grouped = true;
  // The CLUSTERED planes beside the grouped records (vh_grouped.h): the scan reads only the words that cover the run [start[literal], end) of
  // every tile, and no plane of the grouping column at all. A plan takes them when
  //   * they exist, derived from the bit-sliced projection this plan reads (same serial), at the same epoch as records and headers (one launch),
  //   * no filter leaf other than the one `==` leaf reads the grouping column (the planes hold no bit of it),
  //   * every segment's snapshot is the rows the form was built with or a multiple of the tile (0 included): places have lost their row
  //     numbers, so a snapshot that cuts into a built tile cannot be honoured — such a plan keeps the row-order planes, as before.
  // VH_PLAN_NO_GPLANES keeps the row-order planes: an A/B inside one process.
  if (!planes_ok) return;
  P.colbase[P.nslots] = gr->planes.ptr; P.colstride[P.nslots] = gr->planes.stride; P.colpitch[P.nslots] = 4u * gr->G;
  js.gp_slot = P.nslots++; js.gp_G = (int)gr->G; js.gp_goff = (int)gr->goff;
  gplanes = true;
  choose_gpspan();
  // The scan TRIMS its runs (vh_gsub_trim) when the form is sub-sorted, exactly one leaf of the whole program reads its sub column (the rule
  // the grouping column has), that leaf is a relation of the top-level AND a run can be trimmed by, and its literal is a value of the field —
  // otherwise the runs are read whole, which is right for any order inside them. VH_TEST_NO_SUBTRIM=1 reads a sub-sorted form without
  // trimming: an A/B inside one process.
  if (gr->sub_col < 0 || P.nslots >= VH_MAX_SLOTS) return;
  if (const char* e = test_env("VH_TEST_NO_SUBTRIM")) if (atoi(e)) return;
  sp = -1; sp_leaf = -1;
  for (int k : leaves) {
    const int ps = (int)g[k].pslot();
    if (g[k].kind() == VH_F_REL && vh_gsub_op_ok((int)g[k].op()) && ps < js.npred && ps != gp && jit_pred_col[ps] == gr->sub_col) { sp = ps; sp_leaf = k; break; }
  }
  if (sp < 0 || (uint32_t)js.pp_bits[sp] != gr->sub_bits) return;
  int sreads = 0;
  for (const VhProgOp& o : g) if (o.kind() != VH_F_AND && o.kind() != VH_F_OR && o.kind() != VH_F_TRUE && (int)o.pslot() == sp) ++sreads;
  if (sreads != 1) return;
  {   // the literal in field space: a non-negative integer below 2^bits
    const VhProgOp& lf = g[sp_leaf];
    const int ty = (int)lf.type(), es = vh_elem_size(ty);
    if (vh_elem_float(ty) || (int)lf.lit() >= VH_INLINE_LITS) return;
    uint64_t v = P.ilits[lf.lit()];
    if (es < 8) v &= (1ull << (8 * es)) - 1ull;
    if (vh_elem_signed(ty) && es < 8) v = (uint64_t)((int64_t)(v << (64 - 8 * es)) >> (64 - 8 * es));
    if ((vh_elem_signed(ty) && (int64_t)v < 0) || (v >> gr->sub_bits) != 0ull) return;
  }
  const uint64_t tiles = (t->segment_rows + VH_GROUP_TILE - 1) / VH_GROUP_TILE;
  P.colbase[P.nslots] = gr->hdr.ptr + vh_gsub_keys_off(tiles, gbits); P.colstride[P.nslots] = gr->hdr.stride; P.colpitch[P.nslots] = VH_GSUB_KEYS_BYTES;
  js.sub_slot = P.nslots++; js.sub_pred = sp; js.sub_op = (int)g[sp_leaf].op(); js.sub_lit = (int)g[sp_leaf].lit();
  subtrim = true;
}

// Tile groups that SPAN segments (vh_grouped.h, vh_gspan_*; vj_scan's clustered branch): a wave's group of up to 64 tiles no longer ends at a
// segment change — with units of 32 768 rows every unit of a block lies in another segment, which made a group four tiles — a queued survivor
// is its record's table-wide index and the drain pipeline is flushed once per wave. The scan takes the form when the records' and the
// planes' segment strides divide by 4 and 16 and every index of the scanned segments fits 32 bits (VH_TEST_GPSPAN_BOUND lowers the bound:
// tests); compile_kernel takes it back for a plan whose survivors read anything but the one 4-byte record the queue indexes (vh_jit_span_ok;
// choose_grouped's first lines rule that out already), so no reader needs the segment. VH_TEST_NO_GPSPAN=1 keeps the groups inside a segment: an A/B
// inside one process.
void QueryBuild::choose_gpspan() {
  if (const char* e = test_env("VH_TEST_NO_GPSPAN")) if (atoi(e)) return;
  uint64_t bound = VH_GSPAN_BOUND;
  if (const char* e = test_env("VH_TEST_GPSPAN_BOUND")) bound = std::min<uint64_t>(bound, strtoull(e, nullptr, 10));
  uint64_t rec_stride = 0;
  bool one = true;
  auto rec_slot = [&](int s) { if (!rec_stride) rec_stride = P.colstride[s]; one &= P.colstride[s] == rec_stride && P.colpitch[s] == 4; };
  for (int i = 0; i < P.ngroup; ++i) rec_slot((int)P.g[i].slot());
  for (int j = 0; j < P.nmetric; ++j) rec_slot((int)P.m[j].slot());
  if (!rec_stride || !one || !vh_gspan_ok(nseg, rec_stride, P.colstride[jshape.gp_slot], bound)) return;
  jshape.gp_span = 1;
  gpspan = true;
}

int vh_jit_drain_depth(const VhJitShape& s) {
  if (!vh_jit_rec_bytes(s)) return 0;
  int depth = VH_DRAIN_DEPTH_DEFAULT;
  if (const char* e = test_env("VH_TEST_DRAIN_DEPTH")) depth = std::min(std::max(atoi(e), 0), VH_DRAIN_DEPTH_MAX);      // (A/B: depth 0 is the drain as it was)
  return depth;
}

// No compiled kernel for this plan (yet): hand the query to a second plan for the pre-built kernels, with the options of this one. keep_part:
// an organisation chosen as DENSE_PART stays DENSE_PART; no_hashed_part: the hashed partitioning, which only a compiled scan feeds, is off.
int QueryBuild::plan_again(bool keep_part, bool no_hashed_part) {
  vh_plan p2 = *p;
  p2.flags |= VH_PLAN_NO_JIT;
  if (keep_part && mode == VH_MODE_DENSE_PART) p2.flags |= VH_PLAN_FORCE_PART;
  VhLaunchOpts o2 = o;
  o2.rp.no_hpart |= no_hashed_part;
  holder.reset();
  done = true;
  return query_launch_locked(t, x, &p2, out, o2);
}

// No compiled kernel for a plan that asked for the COMPILED aggregate on the planes and met the rest of its rule: the same plan with
// VH_PLAN2_PLANE_AGG in the flag's place, for the pre-built kernels — choose_plane_agg then takes it (bit 27 without bit 5). A member of a
// batch is then answered as the single query it is; one with its kernel at hand is a compiled candidate of the batch (launch() below).
int QueryBuild::plan_again_prebuilt_planes() {
  vh_plan p2 = *p;
  p2.flags |= VH_PLAN_NO_JIT;
  p2.flags2 = (p2.flags2 & ~(uint32_t)VH_PLAN2_PLANE_JIT) | VH_PLAN2_PLANE_AGG;
  VhLaunchOpts o2 = o;
  o2.fuse = nullptr;
  holder.reset();
  done = true;
  return query_launch_locked(t, x, &p2, out, o2);
}

// The aggregate ON the bit-sliced planes by a kernel compiled for this plan's shape (include/viya_hip.h, "Aggregates on the bit-sliced planes,
// compiled"; the frame is vh_jit_planes.h): asked for (pagg_jit), a compiled kernel may run the query at all (jit_try: the JIT policy, the
// plan's flags, VH_JIT_MIN_ROWS), and the rest of the rule holds (plane_agg_rule, the pre-built choice's own). The shape handed to the
// generator is then the plane aggregate's, not the scan's the plan would otherwise get: the filter's fields in F (slot pp_slot, as the
// bit-sliced compacting scan finds them), V in a slot of its own unless it is F, every group column's and every metric's field in V, the
// metrics' kinds and the sink — nothing that is data: the ids' patterns, which rest on lo / extent / stride, stay in the descriptor.
// *settled: this function has answered (kernel at hand, or the query handed to a second plan); false: the flag changes nothing.
int QueryBuild::compile_plane_agg(bool* settled) {
  *settled = false;
  VhPredPack *f = nullptr, *v = nullptr;
  if (!pagg_jit || !jit_try || !plane_agg_rule(&f, &v)) return VH_OK;
  *settled = true;
  // F and V in the plan's LAST two slots, whatever the plan's own slots hold: which narrow copies and projections exist — they come and go
  // with the automatic layouts — must not make another shape, and another compile, of the same query. V's slot is F's when V is F.
  const int fslot = VH_MAX_SLOTS - 2, vslot = f && v == f ? fslot : VH_MAX_SLOTS - 1;
  // No shape for this plan — its last two slots taken, more columns than a shape names, or more filter planes than the 64 registers the
  // compiled scan allows itself for them (compile_kernel below: beyond that the array would spill) —: the pre-built plane kernel, quietly, even
  // under VH_PLAN_FORCE_JIT (include/viya_hip.h lists these beside the other "no compiled kernel can be had" cases).
  int filter_planes = 0;
  for (int k = 0; pagg_filter && k < jshape.npred; ++k) filter_planes += pp_sbits[k];
  if (P.nslots > fslot || P.ngroup > VJ_MAX_COLS || P.nmetric > VJ_MAX_COLS || (pagg_filter && !jshape.pp_sliced) || filter_planes > 64) return plan_again_prebuilt_planes();
  if (f) { P.colbase[fslot] = f->plane[0].ptr; P.colstride[fslot] = f->plane[0].stride; P.colpitch[fslot] = (uint32_t)f->pitch; }
  P.colbase[vslot] = v->plane[0].ptr; P.colstride[vslot] = v->plane[0].stride; P.colpitch[vslot] = (uint32_t)v->pitch;
  VhJitShape js;
  js.mode = mode; js.block = 256;
  js.xcd = nxcd > 1 ? 1 : 0;
  js.scope = nxcd > 1 ? (int)__HIP_MEMORY_SCOPE_WORKGROUP : (int)__HIP_MEMORY_SCOPE_AGENT;      // (vh_launch_scan_planes: vh_with_scope)
  if (pagg_filter) {
    js.prog = jshape.prog; js.nlits = jshape.nlits; js.npred = jshape.npred;
    js.pp_sliced = 1; js.pp_slot = fslot;
    for (int k = 0; k < js.npred; ++k) { js.pred[k] = VhJitPred{-1, jshape.pred[k].type, 0}; js.pp_off[k] = pp_soff[k]; js.pp_bits[k] = pp_sbits[k]; }      // (the planes' fields; no column is streamed)
  } else {
    VhProgOp all{};
    all.set_kind(VH_F_TRUE);
    js.prog = {all};
  }
  js.pa_sink = pagg_desc.rows ? 2 : 1; js.pa_filter = pagg_filter ? 1 : 0; js.pa_vslot = vslot;
  js.ng = P.ngroup; js.nm = P.nmetric;
  for (int i = 0; i < P.ngroup; ++i) { js.pa_goff[i] = (int)pagg_desc.goff[i]; js.pa_gbits[i] = (int)pagg_desc.gbits[i]; }
  for (int j = 0; j < P.nmetric; ++j) { js.m[j].sop = (int)P.m[j].sop(); js.pa_moff[j] = (int)pagg_desc.moff[j]; js.pa_mbits[j] = (int)pagg_desc.mbits[j]; }
  // the kernel: looked up or compiled exactly as the scan's is below (background build mode: the worker's job, pending is not failure)
  std::string jerr;
  VhJitKernel* k = nullptr;
  bool pending = false;
  if (build_background(t)) {
    if (vh_jit_peek(js, &k, &jerr) == 0) pending = build_request_kernel(t, js);
    if (!pending && !k && jerr.empty()) jerr = "the build worker is shutting down";
  } else {
    VhJitKernel* had = nullptr;
    std::string ignored;
    const bool known = vh_jit_peek(js, &had, &ignored) != 0;
    k = vh_jit_get(js, &jerr);
    if (!known) ++t->inline_builds;
  }
  if (pending) {
    ++g_build_quiet;
    const int prc = plan_again_prebuilt_planes();
    --g_build_quiet;
    if (!prc && out && *out) (*out)->info.reserved |= VH_INFO_BUILD_PENDING;
    return prc;
  }
  if (!k) {
    if (knobs().jit_verbose) fprintf(stderr, "vh: compiled aggregate on the planes unavailable, the pre-built one answers: %s\n", jerr.c_str());
    if ((p->flags & VH_PLAN_FORCE_JIT) || vh_jit_policy() == VH_JIT_FORCE) return vh_fail(VH_E_UNSUPPORTED, "per-query kernel requested (VH_PLAN_FORCE_JIT / VH_JIT=force) but unavailable: %s", jerr.c_str());
    return plan_again_prebuilt_planes();
  }
  pagg_jk = k;
  pagg_shape = js;
  plane_agg_take(f, v);
  return VH_OK;
}

int QueryBuild::compile_kernel() {
  {   // ---------------- the aggregate on the planes, compiled, where the plan asked for it: then no scan over rows is compiled at all
    bool settled = false;
    if (int rc = compile_plane_agg(&settled)) return rc;
    if (settled) return VH_OK;
  }
  // ---------------- the scan kernel compiled for this plan shape (vh_jit.hip), when there is to be one
  // the no-compaction kernels are pre-built, except DENSE_LDS's over plain 4- / 8-byte arena columns (C2's shape), which has a compiled form
  if (jit_try && lanes && (mode != VH_MODE_DENSE_LDS || test_env("VH_TEST_NO_JIT_LANES"))) jit_try = false;
  if (jit_try) {
    VhJitShape& js = jshape;
    js.mode = mode;
    const size_t qw = (size_t)VJ_QUEUE_CAP * sizeof(uint32_t);       // per wave
    js.lanes = lanes ? 1 : 0;
    if (mode == VH_MODE_DENSE_LDS || (mode == VH_MODE_HASH && !hpart)) {          // an LDS table per block: the widest block whose table + queues stay within the 64 KB a module kernel may ask for
      jit_block = mode == VH_MODE_DENSE_LDS ? 1024 : 512;
      // (the no-compaction form lives off resident waves like its pre-built twin: 256-thread blocks, as many per CU as fit, unless the blocks'
      // table flushes — blocks x groups x metrics atomics at the end — would weigh more than that; same rule as below)
      if (lanes && (uint64_t)g_ctx.num_cu * 5 * G * std::max(1, P.nmetric) <= rows_to_scan / 32) jit_block = 256;
      const size_t lds_room = 64 * 1024 - 1024;          // (the kernels' own static LDS — vh_scan_block_end's counters — shares the 64 KB)
      while (jit_block > 256 && lds_table + (size_t)(jit_block / 64) * qw > lds_room) jit_block /= 2;
      if (lds_table + (size_t)(jit_block / 64) * qw > lds_room) jit_try = false;
      if (mode == VH_MODE_HASH && !P.lds_hash_slots) jit_block = 256;
    }
    if (hpart) jit_block = 1024;      // (one block per CU shares the 256 digits' waiting lines: vj_fan_add)
    js.block = jit_block;
    js.hp_fan = hpart ? 1 : 0;
    js.ablate = knobs().jit_ablate;      // measurement only (profiles/r03/NOTES.md): 1 = no gathers, 2 = nothing behind the gathers
    js.xcd = nxcd > 1 ? 1 : 0;
    js.scope = (mode == VH_MODE_DENSE_GLOBAL || mode == VH_MODE_DENSE_LDS) && nxcd > 1 ? (int)__HIP_MEMORY_SCOPE_WORKGROUP : (int)__HIP_MEMORY_SCOPE_AGENT;
    js.carrier = P.present_carrier;
    js.tw = mode == VH_MODE_DENSE_PART ? P.tw : 1;
    js.key_words = mode == VH_MODE_HASH ? P.key_words : 1;
    js.lds_hash = P.lds_hash_slots ? 1 : 0;
    js.gid32 = mode != VH_MODE_HASH && G <= 0xFFFFFFFFull;
    js.gid_bits = mode == VH_MODE_DENSE_PART ? P.gid_bits : 0;
    js.tuple4 = mode == VH_MODE_DENSE_PART && P.gid_bits && P.tuple4 ? 1 : 0;
    // one- and two-word tuples of up to 64 partitions leave through the BLOCK's ring writer (vj_part_ring_add): whole lines, extents by position with
    // the pool's shared overflow region behind them; wider tuples are appended piece by piece (vh_part_direct_add)
    part_ring = mode == VH_MODE_DENSE_PART && (P.tw == 2 || P.gid_bits) && P.npart <= VH_RING_PARTS_MAX;
    js.part_ring = part_ring ? (P.npart <= VH_RING_PARTS ? VH_RING_PARTS : VH_RING_PARTS_MAX) : 0;
    js.hpart = hpart ? 1 : 0;
    js.bs_off32 = hpart && hp_off32 ? 1 : 0;
    js.hp_pack = hp_pack ? 1 : 0; js.hp_pbits = hp_pbits; js.hp_idbits = hp_idbits;
    // (measurement, VH_HP_AGG_WAVES=6: bound the aggregation's registers so that three of its blocks fit a CU where its LDS tables allow
    // them — measured: 81 -> 73 registers, the same 1.33 ms; occupancy is not what it waits for. Off.)
    if (hpart && hp_pack && knobs().hp_agg_waves > 0) js.hp_agg_waves = knobs().hp_agg_waves;
    js.ng = P.ngroup; js.nm = P.nmetric;
    js.qpay = !lanes ? qpay : 0; js.qpay_slot = js.qpay ? qpay_slot : -1;
    {   // which predicate projection, if any (shape_filter noted what exists): rows -> byte planes, everything else -> bit-sliced planes
      const bool rows_form = lanes || js.qpay != 0;
      const bool have_sliced = js.pp_sliced != 0, have_bytes = js.pp_nplanes != 0;
      if (VhPredPack* settled = have_sliced && !rows_form && !(p->flags & VH_PLAN_NO_SLICED) ? sliced_use : have_bytes ? bytes_use : nullptr) layout_use(t, settled);
      if (have_sliced && !rows_form && !(p->flags & VH_PLAN_NO_SLICED)) { js.pp_nplanes = 0; for (int k = 0; k < js.npred; ++k) { js.pp_off[k] = pp_soff[k]; js.pp_bits[k] = pp_sbits[k]; } }
      else { js.pp_sliced = 0; js.pp_slot = -1; for (int k = 0; k < js.npred; ++k) { js.pp_off[k] = pp_boff[k]; js.pp_bits[k] = pp_bbits[k]; } }
      // (a plan with a set leaf reads bit planes only where every set's field is narrow enough for a truth table — by the columns' recorded
      // ranges, as the builder would size the fields; otherwise it reads rows whatever its form: the automatic builder is asked for byte
      // planes, never for planes the plan cannot read)
      const bool want_rows = rows_form || (has_set && !sets_fit_planes([&](int col) { return predpack_bits_for(t, col); }));
      if (!(p->flags & (VH_PLAN_NO_NARROW | VH_PLAN_NO_PREDPACK)) && (want_rows ? !have_bytes : !have_sliced)) predpack_auto(!want_rows);
    }
    {   // (the records' registers count against the packed predicate registers' budget)
      int nv = 0;
      if (js.pp_sliced) for (int k = 0; k < js.npred; ++k) nv += js.pp_bits[k];
      else if (js.pp_nplanes) for (int q = 0; q < js.pp_nplanes; ++q) nv += VH_SUBSTEPS * js.pp_plane[q].width;
      else for (int k = 0; k < js.npred; ++k) nv += VH_SUBSTEPS * js.pred[k].width;
      if (js.pp_sliced && nv > 64) { js.pp_sliced = 0; js.pp_slot = -1; }      // (more planes than registers to hold them: the columns themselves)
      if (js.qpay && nv + VH_SUBSTEPS * js.qpay > VJ_MAX_NV) { js.qpay = 0; js.qpay_slot = -1; }
    }
    if (!lanes) choose_grouped();
    for (int i = 0; i < P.ngroup; ++i) {
      const VhGroupDev& g = P.g[i];
      VhJitCol& c = js.g[i];
      c.slot = (int)g.slot(); c.type = (int)g.type(); c.pitch = (int)P.colpitch[g.slot()];
      c.rec = slot_rec[g.slot()]; c.off = slot_recoff[g.slot()]; c.stored = slot_stored[g.slot()]; c.bits = slot_bits[g.slot()];
      c.sext = mode != VH_MODE_HASH;
      c.gran = (int)g.gran(); c.nroll = (int)g.nroll(); c.micro = (int)g.micro();
      c.key_word = (int)g.key_word(); c.key_shift = (int)g.key_shift();
      for (int k = 0; k < c.nroll; ++k) c.roll_unit[k] = (int)g.roll_unit(k);
      if (vh_elem_size(c.type) > 4 || c.type == VH_F32) js.gid32 = 0;
    }
    for (int j = 0; j < P.nmetric; ++j) {
      const VhMetricDev& m = P.m[j];
      VhJitCol& c = js.m[j];
      c.rowid = m.slot() == VH_SLOT_ROWID;
      c.bitset = m.sop() == SOP_BITSET;
      if (c.bitset) js.bitset_j = j;
      c.type = (int)m.type(); c.sop = (int)m.sop(); c.tword = (int)m.tword(); c.tshift = (int)m.tshift(); c.tbits = hp_pack || (mode == VH_MODE_DENSE_PART && P.gid_bits) ? (int)m.tbits : 0;
      c.sext = vh_sop_sext((int)m.sop());
      if (!c.rowid && !c.bitset) { c.slot = (int)m.slot(); c.pitch = (int)P.colpitch[m.slot()]; c.rec = slot_rec[m.slot()]; c.off = slot_recoff[m.slot()]; c.stored = slot_stored[m.slot()]; c.bits = slot_bits[m.slot()]; }
    }
    js.drain_depth = vh_jit_drain_depth(js);      // (last: it goes by the columns above)
    if (js.gp_span && !vh_jit_span_ok(js)) { js.gp_span = 0; gpspan = false; }      // (the spanning queue indexes ONE 4-byte record)
    if (jit_try) {
      std::string jerr;
      // background build mode: a lookup. A shape nobody compiled yet (or that is being compiled) is the worker's: this query is planned for the
      // pre-built kernels as below — but pending is not failure: nothing is remembered, nothing is said, VH_PLAN_FORCE_JIT is no error
      bool pending = false;
      if (build_background(t)) {
        if (vh_jit_peek(js, &jk, &jerr) == 0) pending = build_request_kernel(t, js);
        if (!pending && !jk && jerr.empty()) jerr = "the build worker is shutting down";
      } else {
        VhJitKernel* had = nullptr;
        std::string ignored;
        const bool known = vh_jit_peek(js, &had, &ignored) != 0;
        jk = vh_jit_get(js, &jerr);
        if (!known) ++t->inline_builds;
      }
      if (pending) {
        ++g_build_quiet;        // (the second plan counts towards no automatic layout: this query has been counted)
        const int prc = plan_again(true, false);
        --g_build_quiet;
        if (!prc && out && *out) (*out)->info.reserved |= VH_INFO_BUILD_PENDING;
        return prc;
      }
      if (!jk) {
        // no kernel for this shape (hipRTC missing, or the text did not compile): plan again for the pre-built kernels. The
        // failure is remembered per shape, so only the first query of the shape pays for the attempt.
        if (knobs().jit_verbose) fprintf(stderr, "vh: per-query kernel unavailable, falling back: %s\n", jerr.c_str());
        else {      // said ONCE per process, whatever the verbosity: a maintainer must be able to see this cliff (large scans run about half as fast)
          static std::once_flag told;
          std::call_once(told, [&] { fprintf(stderr, "viya_hip: no per-query compiled scan kernels in this process (%s): the pre-built interpreting kernels answer instead; "
                                                     "vh_result_info.reserved bit 5 tells per query (VH_JIT_VERBOSE=1 for every occurrence)\n", jerr.substr(0, 200).c_str()); });
        }
        if ((p->flags & VH_PLAN_FORCE_JIT) || vh_jit_policy() == VH_JIT_FORCE) return vh_fail(VH_E_UNSUPPORTED, "per-query kernel requested (VH_PLAN_FORCE_JIT / VH_JIT=force) but unavailable: %s", jerr.c_str());
        // (the organisation must not depend on whether THIS rank could compile: partitioning chosen because a compiled scan makes tuples
        // cheap stays chosen — the pre-built kernels run it too — so that sharded ranks keep identically laid out partial tables)
        return plan_again(true, false);
      }
    }
  }
  bool lanes_narrow = false;          // the no-compaction form over 1- / 2-byte group or metric columns, or more than VH_LANES_COLS of either: only its compiled kernel takes those
  if (lanes && mode == VH_MODE_DENSE_LDS) {
    lanes_narrow = P.ngroup > VH_LANES_COLS || P.nmetric > VH_LANES_COLS;
    for (int i = 0; i < P.ngroup; ++i) lanes_narrow |= vh_elem_size(P.g[i].type()) < 4;
    for (int j = 0; j < P.nmetric; ++j) lanes_narrow |= vh_elem_size(P.m[j].type()) < 4;
  }
  if (!jk && (packed_compressed || (mode == VH_MODE_DENSE_PART && P.gid_bits) || lanes_narrow || hpart)) {      // compressed records / one-word tuples / narrow lanes columns / the hashed partitioning (its scan writes level A itself) and no compiled kernel to handle them after all: plan again for the pre-built ones
    return plan_again(false, hpart);
  }
  return VH_OK;
}

// The pre-built scan over the bit-sliced planes answers this aggregate (scan_agg_sliced_kernel; include/viya_hip.h states the rule): asked for
// and found possible so far (planes_ready: a filter, every leaf a field of one usable bit-sliced projection, the inline budget, set leaves with
// truth tables, none of the flags that keep a plan off the planes), no compiled kernel after all, and a plan whose sink the kernel carries —
// not a no-compaction form, and of DENSE_PART what vh_launch_scan_fast_part would run: the compacting form with tuples of two words or more. (A plan
// with a specialised drain, P.shape 1 / 2, goes through the generic one here: vh_consume_fast<.., 0> lays the same tuple out from m[j].tword /
// tshift, and never looks at the second digit a one-column shape plan adds.)
// It only changes which kernel evaluates the predicate. The projection is stamped and held like a compiled reader's; nothing is built or queued.
void QueryBuild::choose_sliced_prebuilt() {
  if (!sliced_asked || plane_agg || !planes_ready || jk || lanes || hpart || g_heavy.only || !sliced_use || sliced_use->applied_epoch != t->sync_epoch) return;
  if (mode == VH_MODE_DENSE_PART && (!fast || P.gid_bits)) return;
  sliced_prebuilt = true;
  layout_use(t, sliced_use);
}

// The aggregate is computed ON the bit-sliced planes (scan_agg_planes_kernel; include/viya_hip.h states the rule, "Aggregates on the bit-sliced
// planes"): asked for and not a sharded query (pagg_want), no compiled kernel after all, the dense LDS table with at most VH_PLANE_AGG_MAX_GROUPS
// ids — any number the table holds when VH_PLAN2_PLANE_ROWS asked (pagg_rows): beyond the bound the row sink stands in for the loop over
// ids (D.rows; vh_plane_agg.h) —, no filter or the select's rule on one current projection F (planes_ready), plain group columns, integer SUM / COUNT / AVG / MIN / MAX states
// only, and ONE usable, current bit-sliced projection V with every group column and every metric's source column, the hidden count included
// (F itself when it has them). Whether the plan settled on the lanes form plays no part. It only changes which kernel fills the block's LDS
// table. F and V are stamped and held; nothing is built or queued. The rule but for "no compiled kernel" is plane_agg_rule, which the compiled
// form (compile_plane_agg, VH_PLAN2_PLANE_JIT) calls too: the two cannot drift.
void QueryBuild::choose_plane_agg() {
  if (plane_agg || jk) return;      // (settled already, by its compiled form: compile_plane_agg; or a compiled scan runs the query)
  VhPredPack *f = nullptr, *v = nullptr;
  if (plane_agg_rule(&f, &v)) plane_agg_take(f, v);
}
void QueryBuild::plane_agg_take(VhPredPack* f, VhPredPack* v) {
  plane_agg = true;
  pagg_ref.rows = pagg_desc.rows;      // (here, not with the rest of pagg_ref in layout_scratch: decompose_work asks the launcher for the kernel's name and occupancy first)
  pagg_v = v;
  if (f) layout_use(t, f);
  layout_use(t, v);
}
bool QueryBuild::plane_agg_rule(VhPredPack** fp, VhPredPack** vp) {
  if (!pagg_want || mode != VH_MODE_DENSE_LDS || (P.G > VH_PLANE_AGG_MAX_GROUPS && !pagg_rows) || P.nbitset) return false;
  // The row sink takes a plan that asked for it (VH_PLAN2_PLANE_ROWS) from one id beyond the loop's bound on; the test hook moves that threshold
  // down, so that one process runs the same small plan through both sinks.
  uint64_t rows_min = VH_PLANE_AGG_MAX_GROUPS + 1;
  if (const char* e = test_env("VH_TEST_PLANE_ROWS_MIN")) rows_min = std::min<uint64_t>(rows_min, strtoull(e, nullptr, 10));
  const bool rows = pagg_rows && P.G >= rows_min;
  VhPredPack* f = nullptr;
  if (pagg_filter) {
    if (!planes_ready || !sliced_use || sliced_use->applied_epoch != t->sync_epoch) return false;
    f = sliced_use;
  }
  std::vector<int> cols;
  for (int i = 0; i < P.ngroup; ++i) {
    if (P.g[i].gran() != VH_T_NONE || P.g[i].nroll()) return false;
    cols.push_back(p->groups[i].col);
  }
  for (int j = 0; j < P.nmetric; ++j) {
    const int sop = (int)P.m[j].sop();
    const bool integer = sop == SOP_ADD32 || sop == SOP_ADD64 || (sop >= SOP_MIN_I32 && sop <= SOP_MAX_U64);
    if (!integer || P.m[j].slot() == VH_SLOT_ROWID || metric_col[j] < 0) return false;
    cols.push_back(metric_col[j]);
  }
  std::sort(cols.begin(), cols.end());
  cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
  if (cols.empty()) return false;
  VhPredPack* v = f && std::includes(f->cols.begin(), f->cols.end(), cols.begin(), cols.end()) ? f : predpack_usable(t, cols, 1);
  if (!v || !v->sliced || v->bits > VH_BITS_MAX_FIELD || v->applied_epoch != t->sync_epoch) return false;

  VhPlaneAggDesc& D = pagg_desc;
  D = VhPlaneAggDesc{};
  D.has_filter = pagg_filter ? 1u : 0u;
  auto field = [&](int col, uint32_t* off, uint32_t* bits) {
    const size_t at = (size_t)(std::find(v->cols.begin(), v->cols.end(), col) - v->cols.begin());
    *off = v->bitoff[at]; *bits = v->bitw[at];
    return (*bits >= 32u ? ~0u : (1u << *bits) - 1u) << *off;
  };
  for (int i = 0; i < P.ngroup; ++i) D.care |= field(p->groups[i].col, &D.goff[i], &D.gbits[i]);
  D.need = D.care;
  for (int j = 0; j < P.nmetric; ++j) D.need |= field(metric_col[j], &D.moff[j], &D.mbits[j]);
  D.rows = rows ? 1u : 0u;
  for (uint64_t g = 0; g < P.G && !rows; ++g) {      // id g's digits -> the values its rows hold, at their fields' places (the row sink goes the other way: a row's values -> its id)
    uint32_t pat = 0;
    bool fits = true;
    for (int i = 0; i < P.ngroup; ++i) {
      const uint64_t value = P.g[i].lo + (g / P.g[i].stride) % P.g[i].extent;
      if (value >> D.gbits[i]) fits = false;      // beyond the field: no row holds it
      else pat |= (uint32_t)value << D.goff[i];
    }
    D.pat[g] = pat;
    if (fits) D.valid |= 1ull << g;
  }
  *fp = f; *vp = v;
  return true;
}

// The one place that decides which scan kernel runs. L brings the grid to launch — or, with L.occ / L.name set, what the chosen launcher is to
// answer instead of launching (VhScanLaunch) —; LDS bytes and stream are filled in here. A compiled kernel carries its own name (jk->name).
void QueryBuild::scan_dispatch(VhScanLaunch L) {
  const size_t qb = (size_t)(BLOCK / 64) * VhScanCfg<256>::kQueueCap * sizeof(uint32_t);
  const bool xcd_private = nxcd > 1;
  const uint32_t chunks_per_seg = (uint32_t)std::max<uint64_t>(1, (t->padded_rows + VH_SLICED_CHUNK_ROWS - 1) / VH_SLICED_CHUNK_ROWS);      // the readers of the planes walk 2048-row chunks
  L.lds = ((mode == VH_MODE_DENSE_LDS || mode == VH_MODE_HASH) ? lds_table : 0) + qb;
  L.stream = x->stream();
  if (plane_agg) {      // (no queue: the block's LDS table alone)
    L.lds = lds_table;
    if (pagg_jk) {      // ... compiled for this plan's shape: plan, descriptor and chunks per segment (the row sink's queue is static LDS of the kernel)
      if (L.occ) *L.occ = vh_jit_occupancy(pagg_jk, BLOCK, lds_table);
      else if (!L.name) (void)vh_jit_launch_planes(pagg_jk, P, pagg_ref.D, chunks_per_seg, L.grid, BLOCK, lds_table, L.stream);
    }
    else vh_launch_scan_planes(P, pagg_ref, chunks_per_seg, L, xcd_private);
  }
  else if (sliced_prebuilt) {
    if (mode == VH_MODE_DENSE_PART) L.lds = qb;
    vh_launch_scan_sliced(mode, P, planes_ref, chunks_per_seg, L, xcd_private);
  }
  else if (jk) {
    const size_t jl = ((mode == VH_MODE_DENSE_LDS || (mode == VH_MODE_HASH && !hpart)) ? lds_table : 0) + (size_t)(BLOCK / 64) * (VJ_QUEUE_CAP * sizeof(uint32_t)) +
                      (jshape.hp_fan ? VJ_FAN_LDS_BYTES(BLOCK) : 0) + (jshape.part_ring ? VH_RING_LDS_BYTES(jshape.part_ring, 2, BLOCK) : 0);
    if (L.occ) *L.occ = vh_jit_occupancy(jk, BLOCK, jl);
    else if (!L.name) (void)vh_jit_launch(jk, P, L.grid, BLOCK, jl, L.stream);
  }
  else if (mode == VH_MODE_DENSE_PART) {
    L.lds = lanes ? 4 * vh_part_tile_bytes(P) : qb;      // (the compacting form appends straight to the extents: no tile in LDS)
    if (lanes) vh_launch_scan_lanes_part(P, L);
    else vh_launch_scan_fast_part(P, L);
  }
  else if (!fast) vh_launch_scan_generic(mode, P, L, xcd_private);
  else if (lanes && mode == VH_MODE_HASH) vh_launch_scan_lanes_hash(P, L);
  else if (lanes) vh_launch_scan_lanes_lds(P, BLOCK, L, xcd_private);
  else if (mode == VH_MODE_DENSE_LDS) vh_launch_scan_fast_lds(P, L, xcd_private);   // 1024-thread blocks: one per CU
  else if (mode == VH_MODE_DENSE_GLOBAL) vh_launch_scan_fast_global(P, L, xcd_private);
  else vh_launch_scan_fast_hash(P, L);
}

int QueryBuild::decompose_work() {
  // ---------------- work decomposition
  // The lanes kernels expose the latency of their payload loads (issued and consumed inside a sub-step), so they gain
  // from every extra resident wave: 256-thread blocks, as many per CU as registers and LDS allow (asked of the runtime
  // per instantiation: 5 for one predicate column today, 4 for two or more) — C2 at 1 B rows: 3.67 -> 3.39 ms. The LDS
  // variant pays for more blocks with more table merges at the end (blocks x groups x metrics global atomics), so
  // it keeps one 1024-thread block per CU unless the scan dwarfs that.
  const int env_lanes_block = knobs().lanes_block, env_bpc = knobs().blocks_per_cu, env_unit = knobs().unit_rows;
  choose_plane_agg();           // (first: when both apply, the aggregate on the planes wins)
  choose_sliced_prebuilt();
  BLOCK = jk ? jit_block : mode == VH_MODE_DENSE_LDS && !plane_agg ? 1024 : 256;      // (the aggregate on the planes: 151 registers a lane, three 256-thread blocks per CU; its table has at most 64 groups to flush — with the row sink 105 registers and whatever table the organisation allows)
  // (the compiled plane aggregate, pagg_jk, takes the same 256 threads: at its 62 - 80 registers up to eight blocks fit a CU (occ_cap below) where
  // the pre-built kernel has three, i.e. more table flushes per CU. Block size and blocks per CU were NOT measured separately for it:
  // profiles/r21/NOTES.md shows the result of this choice only)
  if (mode == VH_MODE_DENSE_LDS && lanes && !plane_agg) {
    if (env_lanes_block == 256 || env_lanes_block == 512 || env_lanes_block == 1024) BLOCK = env_lanes_block;
    else if ((uint64_t)g_ctx.num_cu * 5 * G * std::max(1, P.nmetric) <= rows_to_scan / 32) BLOCK = 256;
  }
  // The scan launcher answers, without launching: how many of its kernel's blocks fit a CU, and — a pre-built kernel — what it is called.
  int occupancy = 0;
  {   // the kernel symbol(s) this query runs, as rocprofv3 prints them (vh_result_kernel: bench.py's roofline.kernel)
    char nm[160] = "";
    VhScanLaunch ask;
    const VhJitKernel* compiled = jk ? jk : pagg_jk;
    ask.occ = env_bpc <= 0 ? &occupancy : nullptr; ask.name = compiled ? nullptr : nm; ask.name_cap = sizeof(nm);
    if (ask.occ || ask.name) scan_dispatch(ask);
    r->kernel = compiled ? compiled->name : std::string(nm);
    if (hpart) {      // (the scatter kernel runs twice per query, level A and level B: named twice, so that per-query sums over the names count it twice)
      char hn[160];
      if (hp_fan) snprintf(hn, sizeof(hn), " + hp_ring_scatter_kernel<1024, %d> + ", hp_units);      // (the scan wrote level A itself; level B without barriers)
      else snprintf(hn, sizeof(hn), " + hp_scatter_kernel<1024, %d> + hp_scatter_kernel<1024, %d> + ", hp_units, hp_units);
      r->kernel += hn + jk->name + "_hpagg";
    }
    if (mode == VH_MODE_DENSE_PART) {
      if (P.nlevel == 2) r->kernel += " + " + vh_part_split_name(P);
      r->kernel += " + " + (jit_pagg() ? jk->name + "_pagg" : std::string(vh_part_agg_name()));
    }
  }
  const uint32_t step = BLOCK * (jk && jshape.pp_sliced ? 32u : (uint32_t)VH_LANE_ROWS);      // (bit-sliced predicates: a lane owns 32 consecutive rows per step)
  const uint64_t padded = (t->segment_rows + step - 1) / step * step;
  // all blocks co-resident (the compacting kernels need ~100-130 VGPRs: 4 waves/SIMD), units small enough
  // that the static round-robin leaves < 2 % imbalance
  // The compiled kernels that WRITE tuples (DENSE_PART phase 1, hashed partitioning) run best with fewer resident waves than their
  // 56-69 VGPRs allow: every wave keeps a line or an extent open per partition, and what eight blocks per CU keep open no longer
  // stays in L2 until it is complete (profiles/r03/NOTES.md, "Blocks per CU": a 125 M-row C3 shard 0.44 -> 0.39 ms with 3 instead of
  // 6, C5's scan 1.95 -> 1.6 ms with 4 instead of 8, and the scatter behind it finds fewer half-empty extents)
  // (the compiled no-compaction kernel has a whole step's payload in flight per wave — 16 rows x every column per lane: two 256-thread blocks per
  // CU already stream at full rate, and every block fewer is a table flush fewer: C2 0.315 -> 0.308 ms, 400 M rows 1.217 -> 1.179)
  // (through the block's ring writer a block keeps its partitions' lines open, not every wave: four blocks per CU — over four fresh processes each
  // 1.296-1.312 ms per C3 query against 1.265-1.405 with three and 1.31-1.48 with five; an eighth of the table 0.283 against 0.294)
  // (round 9, the scan reading the clustered planes: no longer bound by bytes and open lines but by the latency of its drains — the gather of
  // a survivor's packed record, the ring writer's LDS round trips — which a fifth block per CU hides: C3's scan + phase 2 0.771 / 0.676 / 0.633 ms
  // with three / four / five, 0.745 / 0.663 / 0.631 with the pipelined drain; five is what 85-88 registers allow. Plans without a packed
  // record were not measured again and keep four: profiles/r09/NOTES.md)
  const int occ_cap = jk && mode == VH_MODE_DENSE_PART ? (jshape.part_ring ? (vh_jit_rec_bytes(jshape) ? 5 : 4) : 3) : jk && hpart ? 4 : jk && lanes ? 2 : 8;
  int blocks_per_cu = env_bpc > 0 ? env_bpc : occupancy > 0 ? std::min(occupancy, occ_cap) : (BLOCK == 1024 ? 1 : 4);
  if (const char* e = test_env("VH_TEST_BLOCKS_PER_CU")) { if (atoi(e) > 0) blocks_per_cu = occupancy > 0 ? std::min(occupancy, atoi(e)) : atoi(e); }   // (measurement: switched between two queries of one process)
  uint32_t unit_rows = step;
  // (units of 4 096 rows lose to longer ones — an eighth of C3 0.342 -> 0.332 ms with 16 K rows, a quarter 0.569 -> 0.542 and the whole table
  // 1.867 -> 1.841 with 32 K, 64 K no better — so a block only needs about eight of them to keep the round-robin even: tools/env_ab_probe.py)
  const uint64_t want_units = (uint64_t)g_ctx.num_cu * blocks_per_cu * (jk ? 8 : 64);
  while (unit_rows * 2 <= (jk ? 32768u : 65536u) && unit_rows * 2 <= padded &&
         (uint64_t)nseg * ((padded + unit_rows * 2 - 1) / (unit_rows * 2)) >= want_units) unit_rows *= 2;
  if (env_unit >= (int)step) unit_rows = (uint32_t)env_unit / step * step;
  if (const char* e = test_env("VH_TEST_UNIT_ROWS")) { if (atoi(e) >= (int)step) unit_rows = (uint32_t)atoi(e) / step * step; }   // (measurement: switched between two queries of one process)
  P.unit_rows = unit_rows;
  P.units_per_seg = (uint32_t)((t->segment_rows + unit_rows - 1) / unit_rows);
  P.nseg = nseg;
  P.total_units = nseg * P.units_per_seg;
  const int env_grid = knobs().grid;
  grid = env_grid > 0 ? env_grid : (int)std::max<uint64_t>(1, std::min<uint64_t>(P.total_units, (uint64_t)g_ctx.num_cu * blocks_per_cu));
  // The second pass over heavy ranges runs WHILE the first pass's rows cross PCIe (result_finalize): the 64 blocks that push them take wave slots
  // on 64 CUs, and a grid that fills the chip exactly then leaves some of its blocks waiting for a whole other block's share (measured: the pass
  // 8.3 -> 10.7-14.7 ms). Eight times the blocks, an eighth of the units each: the dispatcher hands them out as slots come free (9.0-11.9 ms; what is left is the PCIe traffic's
  // own cost to everything that is dispatched beside it).
  if (g_heavy.only && env_grid <= 0) grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(P.total_units, (uint64_t)g_ctx.num_cu * blocks_per_cu * 8));
  return VH_OK;
}

int QueryBuild::layout_scratch() {
  int rc = VH_OK;
  // ---------------- scratch layout
  ScratchPlan sp;
  // [counters | out_count | output key arrays | output state arrays] is one region: it is read back with a
  // single D2H copy when small, and its head is cleared with a single memset
  const size_t o_counters = sp.take(8 * sizeof(unsigned long long));
  const size_t o_outcount = sp.take(sizeof(unsigned long long));
  r->out_cap = mode == VH_MODE_HASH ? capacity + 1 : G;
  // a big result of the hashed partitioning whose groups nothing has to look at on the device first leaves in chunks, copied out while
  // the later chunks still aggregate: VH_HP_CHUNKS regions of the output columns, each with room for its share of the groups (the mixed
  // key spreads GROUPS evenly over the level-A partitions whatever the rows' skew) and a quarter more; a region that overflows all the
  // same voids the attempt like any pool that runs out
  r->hp_direct = hpart && r->nhaving == 0 && r->topk == 0;
  // ... or, in ONE launch, only takes its rows' places off the counter of its region (VH_HP_REGIONS, default off): every range of the aggregation
  // ends with a returning atomic on the result's row counter — 65 536 of them per query, each a block-wide wait. Measured: spreading them over
  // eight words buys nothing (profiles/r05/NOTES.md)
  const bool hp_streamed = knobs().hp_stream > 0 ? capacity >= (1ull << 22) : test_env("VH_TEST_HP_STREAM") != nullptr;
  const bool hp_regions = !hp_streamed && knobs().hp_regions > 1 && capacity >= (1ull << 22);
  if (r->hp_direct && !o.device_rows && (hp_streamed || hp_regions)) {
    int nch = std::min(hp_regions ? knobs().hp_regions : knobs().hp_stream > 0 ? knobs().hp_stream : 4, VH_HP_CHUNKS);
    while (HP_FAN % nch) --nch;
    r->hp_chunks = nch;
    r->hp_one_launch = hp_regions;
    r->hp_chunk_rows = capacity / nch + capacity / (4 * nch) + 4096;
    r->out_cap = r->hp_chunk_rows * nch;
    rc = exec_streaming(x);
    if (rc) return rc;
  }
  size_t o_okey[VH_MAX_GROUP], o_ostate[VH_MAX_METRIC];
  for (int i = 0; i < P.ngroup; ++i) o_okey[i] = sp.take(r->out_cap * vh_elem_size(P.g[i].type()));
  for (int j = 0; j < P.nmetric; ++j) o_ostate[j] = sp.take(r->out_cap * vh_elem_size(r->metric_elem[j]));
  r->out_region_off = o_counters;
  r->out_region_bytes = sp.off - o_counters;
  for (int i = 0; i < P.ngroup; ++i) r->off_key[i] = o_okey[i] - o_counters;
  for (int j = 0; j < P.nmetric; ++j) r->off_state[j] = o_ostate[j] - o_counters;
  o_segrows = sp.take(r->plan_words * sizeof(uint32_t));   // [segment snapshot | program | literals]
  size_t o_present = 0, o_hkeys = 0, o_htags = 0;
  size_t o_state[VH_MAX_METRIC];
  // Phase 2's blocks by the partitions' tuple counts (vh_part_shares): one-level DENSE_PART whose phase 1 goes through the ring writer (it counts), with a
  // private copy of its range per phase-2 block — then a hot partition may take most of the blocks, and as many copies: room for up to 128 of them
  // (256 MB of states at most; the merge only reads the copies a partition's blocks wrote). Not for results small enough for the one-block tail.
  part_balanced = mode == VH_MODE_DENSE_PART && P.nlevel == 1 && jk && jshape.part_ring != 0 && part_bpp > 1 && nxcd == part_bpp && !knobs().skip_phase2 &&
                  !test_env("VH_NO_PART_BALANCE") &&
                  !(r->out_cap <= VH_SMALL_TAIL_MAX && (uint64_t)r->out_cap * (uint64_t)nxcd * (uint64_t)std::max(1, (int)P.nmetric) <= VH_SMALL_TAIL_STATES);
  if (part_balanced) {
    size_t per_copy = P.xcd_stride;      // presence bytes + states
    for (int j = 0; j < P.nmetric; ++j) per_copy += P.xcd_stride * (size_t)vh_sop_bytes(P.m[j].sop());
    const int room = (int)std::max<size_t>(1, ((size_t)256 << 20) / std::max<size_t>(per_copy, 1));
    nxcd = std::max(nxcd, std::min(std::min(128, room), P.npart * part_bpp));
    P.nxcd = nxcd; r->nxcd = nxcd;
  }
  r->part_blocks = (uint32_t)(P.nfine * part_bpp);
  table_n = mode == VH_MODE_HASH ? capacity + 1 : P.xcd_stride * nxcd;
  // single-word keys: one record per slot = key + every metric state (8-byte states first), so that an insert and its
  // updates touch ONE line of a table that is far bigger than any cache
  // Only for tables far bigger than the caches: with few, hot groups three atomics on ONE line serialise more than on three
  // (C2 forced onto the hash table, 1 K groups: 1.75 ms with separate arrays, 2.21 ms with records).
  if (mode == VH_MODE_HASH && P.key_words == 1 && (hpart || ((capacity >= (1ull << 22) || (p->flags & VH_PLAN_FORCE_HASH_RECORDS)) && !(p->flags & VH_PLAN_NO_HASH_RECORDS)))) {
    size_t off = 8;
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < P.nmetric; ++j) {
        const int b = vh_sop_bytes(P.m[j].sop());
        if ((pass == 0) != (b == 8)) continue;
        rec_off[j] = off; off += b;
      }
    off = (off + 7) / 8 * 8;
    if (off <= 64) P.hrec_bytes = (uint32_t)off;
  }
  if (mode == VH_MODE_HASH) {
    o_hkeys = sp.take(P.hrec_bytes ? table_n * P.hrec_bytes : table_n * P.key_words * sizeof(uint64_t));
    if (P.key_words > 1) o_htags = sp.take(table_n * sizeof(uint32_t));
  } else {
    o_present = sp.take(table_n);
  }
  // zero-identity states (every SUM) sit right behind the presence bytes: one memset clears them all
  zero_begin = mode == VH_MODE_HASH ? sp.off : o_present;
  if (P.hrec_bytes) { for (int j = 0; j < P.nmetric; ++j) o_state[j] = o_hkeys + rec_off[j]; }
  else for (int j = 0; j < P.nmetric; ++j) if (P.m[j].ident == 0) o_state[j] = sp.take(table_n * vh_sop_bytes(P.m[j].sop()));
  zero_end = sp.off;
  if (!P.hrec_bytes) for (int j = 0; j < P.nmetric; ++j) if (P.m[j].ident != 0) o_state[j] = sp.take(table_n * vh_sop_bytes(P.m[j].sop()));
  // device top-N: worth it only when the group table is big (small results are read back whole anyway)
  size_t o_tkkeys = 0, o_tkstate = 0, o_okey2[VH_MAX_GROUP] = {}, o_ostate2[VH_MAX_METRIC] = {};
  r->topk_active = r->topk > 0 && r->out_cap > 65536 && !knobs().no_topk;
  if (r->topk_active) {
    o_tkkeys = sp.take(r->out_cap * sizeof(uint64_t));
    o_tkstate = sp.take(sizeof(VhTopkState));
    for (int i = 0; i < P.ngroup; ++i) o_okey2[i] = sp.take(r->out_cap * vh_elem_size(P.g[i].type()));
    for (int j = 0; j < P.nmetric; ++j) o_ostate2[j] = sp.take(r->out_cap * vh_elem_size(r->metric_elem[j]));
  }
  // outputs
  size_t o_tuples = 0, o_emiss = 0, o_epart = 0, o_tuples2 = 0, o_emiss2 = 0, o_epart2 = 0, o_l2 = 0;
  if (part_balanced) o_pcount = sp.take(VH_MAX_PART * VH_PART_COUNT_WAYS * sizeof(uint32_t));
  // hashed partitioning whose groups leave straight into the output columns, planned by a caller that can run a second pass (vh_query_agg): ranges
  // that are too heavy for a block's LDS tables are marked in a bitmap of the 65 536 ranges instead of voiding the attempt
  heavy_marks = hpart && r->hp_direct && !r->hp_chunks && !o.device_rows && g_heavy.allow_mark && !g_heavy.only && P.hp_passes == 1 && !test_env("VH_NO_HEAVY_PASS");
  if (heavy_marks) o_heavy = sp.take(65536 / 8);
  if (hpart) part_tuple_cap = hp_tuple_cap;
  if (mode == VH_MODE_DENSE_PART || hpart) {
    // extent size: big enough that a wave allocates rarely (every allocation is a returning global
    // atomic = a full round trip the wave sits out), small enough that open extents do not waste HBM
    const uint64_t waves = (uint64_t)grid * (uint64_t)(BLOCK / 64);
    // ... and small enough that a wave fills about four of them per partition: the last extent of every (wave, partition) stays part
    // full, and phase 2 walks part-full extents at the price of full ones (C3: 1250 tuples per wave and partition — extents of 1024
    // were 61 % full on average, of 256 they are 90 %: kernels 2.07-2.12 -> 2.00-2.01 ms, an eighth of the table 0.36-0.38 -> 0.35-0.36)
    uint64_t et = 256;                 // a tile writes whole runs (<= VH_PART_TILE tuples) that must fit a fresh extent
    while (et < 4096 && et * 2 <= part_tuple_cap / (waves * P.npart) / 4) et *= 2;
    if (knobs().ext_tuples) et = std::max(256, knobs().ext_tuples);     // measurement
    if (hpart) et = HP_ET / hp_units;  // (the tiles of hp_scatter_kernel are whole source extents: 64 KB of tuples)
    const bool ring1 = jk && jshape.part_ring != 0;      // phase 1 through the block's ring writer: (block, partition) streams, extents by position
    const uint64_t per1 = (uint64_t)grid * (uint64_t)std::max(1, (int)P.npart);
    if (ring1) { et = 256; while (et < 4096 && et * 2 <= part_tuple_cap / per1 / 4) et *= 2; }      // (a power of two: the writer shifts)
    const uint64_t ext_tuples = et;
    P.ext_tuples = (int32_t)ext_tuples;
    // extents of pool 1 start one 128-byte line further apart than they are long (not the stream pools of the hashed partitioning, whose
    // reader takes extents as whole tiles): see VhPlanDev::ext_stride
    const uint64_t ext_stride = hpart ? ext_tuples : ext_tuples + (P.tuple4 ? ((uint64_t)knobs().ext_pad + 31) / 32 * 32 : P.gid_bits ? ((uint64_t)knobs().ext_pad + 15) / 16 * 16 : (uint64_t)knobs().ext_pad);      // (whole 128-byte lines: 8 two-word tuples, 16 one-word ones, 32 four-byte ones)
    P.ext_stride = (int32_t)ext_stride;
    uint64_t max_ext = part_tuple_cap / ext_tuples + waves * (P.npart + VH_EXT_CHUNK) + 64;
    if (max_ext > 0xFFFFFFF0ull) max_ext = 0xFFFFFFF0ull;
    if (hpart) max_ext = 64;      // (the scan writes the level-A pool itself — the plan's second pool —: nothing goes into this one)
    // the ring writer's pool: every (block, partition) stream its share of evenly spread tuples and one more extent BY POSITION, and behind those the
    // shared overflow region — room for all the expected tuples once more, so that ANY skew between the streams fits (one partition taking everything
    // included); only more survivors than estimated void the attempt, and the re-run is sized for the survivors it counted
    uint64_t pos1 = 0;
    if (ring1) { pos1 = part_tuple_cap / per1 / ext_tuples + 1; max_ext = std::min<uint64_t>(pos1 * per1 + part_tuple_cap / ext_tuples + per1 + 64, 0xFFFFFFF0ull); }      // (+ per1: every stream's last, part-filled overflow extent)
    if (!o.rp.part_override && test_env("VH_TEST_PART_EXTENTS")) max_ext = std::max(1, atoi(test_env("VH_TEST_PART_EXTENTS")));   // tests: make the first attempt run out of extents
    const uint32_t test_levels = test_env("VH_TEST_POS_LEVELS") ? (uint32_t)std::max(0, atoi(test_env("VH_TEST_POS_LEVELS"))) : ~0u;      // tests: few (or no) positional levels — the tuples go through the overflow regions
    P.slice_levels_cap = test_levels;
    if (ring1) P.pos_levels = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(pos1, max_ext / per1), test_levels);
    P.max_extents = (uint32_t)max_ext;
    // the scan's waves take their extent chunks by position (no shared cursor, no returning atomics: VhPlanDev::ext_waves). The pool above
    // holds that whenever the waves' tuple counts agree within the 25 % the estimate leaves; a re-run after VH_ERR_PART_FULL goes back to
    // the cursor, which packs the chunks whatever the imbalance
    P.ext_waves = ring1 || o.rp.part_override || test_env("VH_TEST_EXT_CURSOR") || t->part_clustered.count(r->group_sig) ? 0u : (uint32_t)grid * (uint32_t)(BLOCK / 64);
    o_tuples = sp.take(max_ext * ext_stride * (P.tuple4 ? 4 : P.tw * 8));
    o_emiss = sp.take(max_ext * sizeof(uint16_t));
    o_epart = sp.take(max_ext);
    if (P.nlevel == 2) {
      // pool 2: small extents (4096 ranges x every splitting wave keep one open), sized like pool 1 plus what stays open
      split_bpp = std::max(1, 2 * g_ctx.num_cu / std::max(1, P.npart));     // 256-thread blocks, ~2 per CU whatever the partition count: more waves keep more extents open (4 per CU measured slower)
      // one- and two-word tuples are split through the ring writer (vh_part_split_rings): a block is one writer, more of them cost less
      const bool tiled = vh_part_split_rings(P);
      if (tiled) split_bpp = std::max(1, 4 * g_ctx.num_cu / std::max(1, P.npart));
      const uint64_t et2 = tiled ? VH_SPLIT_TILE_TUPLES : 256;
      P.ext_tuples2 = (int32_t)et2;
      uint64_t max2 = (part_tuple_cap + part_tuple_cap / 4) / et2 + (uint64_t)P.npart * ((uint64_t)split_bpp * (tiled ? 1 : 4) * (64 + VH_EXT_CHUNK) + 1) + 64;
      split_ring = tiled;
      // (slices laid out on the device from the partitions' counted tuples — vh_slice_extents: positional extents + an overflow region as big as the count)
      if (split_ring) max2 = 2 * (part_tuple_cap / et2) + (uint64_t)P.npart * (2 * 64 * split_bpp + 2) + 64;
      if (max2 > 0xFFFFFFF0ull) max2 = 0xFFFFFFF0ull;
      if (!o.rp.part_override && test_env("VH_TEST_PART_EXTENTS2")) max2 = std::max(1, atoi(test_env("VH_TEST_PART_EXTENTS2")));   // tests: the second pool runs out first
      P.max_extents2 = (uint32_t)max2;
      o_tuples2 = sp.take(max2 * et2 * (P.tuple4 ? 4 : P.tw * 8));
      o_emiss2 = sp.take(max2 * sizeof(uint16_t));
      o_epart2 = sp.take(max2);
      o_l2 = sp.take((VH_L2_WORDS + VH_MAX_PART) * sizeof(uint32_t));
    }
  }
  // hashed partitioning: the two partitioned pools (vh_hpart.h), their fill / tag arrays and a block of small tables
  hp_meta_bytes = 8 + (size_t)HP_FAN * 4 + (size_t)(2 * HP_FAN + 2) * 4;      // [level-A cursor | tuples per digit | slices + their cursors]
  if (hpart) {
    for (int k = 0; k < 1; ++k) {
      const uint64_t cap = hp_tuple_cap, hp_et = HP_ET / hp_units, hp_es = hp_et + (uint64_t)knobs().ext_pad / hp_units;      // tuples per extent / between extent starts
      // level A: extents by position — extent k of (scan block, digit) is k * blocks * 256 + block * 256 + digit: a (block, digit)'s share and one more —,
      // then the shared overflow region: all the tuples once more (any skew between the digits fits)
      const uint64_t per = (uint64_t)grid * HP_FAN, posa = cap / per / hp_et + 1;
      uint64_t ma = posa * per + cap / hp_et + per + 64;
      if (!o.rp.part_override && test_env("VH_TEST_PART_EXTENTS")) ma = std::max(1, atoi(test_env("VH_TEST_PART_EXTENTS")));      // tests: the first attempt's pool is too small
      P.pos_levels2 = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(posa, ma / per), test_env("VH_TEST_POS_LEVELS") ? (uint64_t)std::max(0, atoi(test_env("VH_TEST_POS_LEVELS"))) : ~0ull);
      // level B: hp_plan_kernel's slices — positional extents + an overflow region as big as the partition's count (vh_slice_extents).
      hp_ring_nb = 1;      // (level-B blocks per partition. Measured, C5: two or four of them write level B no faster — 0.425 / 0.421 / 0.397 ms — and leave the
                           //  aggregation two or four extents per range to walk: 1.08 / 1.24 / 1.69 ms)
      uint64_t mb = 2 * (cap / hp_et) + (uint64_t)HP_FAN * (2 * HP_FAN * hp_ring_nb + 2) + 64;
      if (!o.rp.part_override && test_env("VH_TEST_PART_EXTENTS2")) mb = std::max(1, atoi(test_env("VH_TEST_PART_EXTENTS2")));   // tests: the last pool runs out
      hpo[k].maxa = ma; hpo[k].maxb = mb;
      hpo[k].ta = sp.take(ma * hp_es * 16 * hp_units); hpo[k].fa = sp.take(ma * 2); hpo[k].ga = sp.take(ma);
      hpo[k].tb = sp.take(mb * hp_es * 16 * hp_units); hpo[k].fb = sp.take(mb * 2); hpo[k].gb = sp.take(mb);
      hpo[k].meta = sp.take(hp_meta_bytes);
    }
    o_hpargs = sp.take(sizeof(VhHpArgs));
  }
  size_t o_fbs[VH_MAX_BITSET] = {};
  for (size_t k = 0; k < r->filter_bitset_cols.size(); ++k) o_fbs[k] = sp.take(std::max<uint32_t>(nseg, 1) * 8);
  size_t o_bsptr[VH_MAX_BITSET][2] = {}, o_dkeys[VH_MAX_BITSET] = {}, o_dtags[VH_MAX_BITSET] = {};
  for (int b = 0; b < P.nbitset; ++b) {
    o_bsptr[b][0] = sp.take(std::max<uint32_t>(nseg, 1) * 8);
    o_bsptr[b][1] = sp.take(std::max<uint32_t>(nseg, 1) * 8);
    if (hpart) continue;             // (its count-distinct lives in the LDS sets of hp_aggregate_kernel)
    // the (group, id) set can never hold more pairs than there are ids in the scanned segments
    uint64_t cap = 1024;
    const uint64_t ids = g_heavy.only ? std::min<uint64_t>(bitset_ids[b], g_heavy.ids_bound) : bitset_ids[b];      // (a heavy pass: the ids its ranges can hold)
    while (cap < ids * 2) cap <<= 1;
    P.dset_mask[b] = cap - 1;
    if (P.bs_wide[b]) { o_dkeys[b] = sp.take(cap * 16); o_dtags[b] = sp.take(cap * 4); }
    else {
      if (table_n >= 0xFFFFFFFFull) { return vh_fail(VH_E_UNSUPPORTED, "count-distinct over more than 2^32 group slots"); }
      o_dkeys[b] = sp.take(cap * 8);
    }
  }
  rc = ensure_scratch(x, sp.off);
  if (rc) { return rc; }
  S = x->scratch;
  P.counters = reinterpret_cast<unsigned long long*>(S + o_counters);
  P.seg_rows = reinterpret_cast<const uint32_t*>(S + o_segrows);
  P.prog = reinterpret_cast<const VhProgOp*>(S + o_segrows + r->seg_words * 4);
  P.lits = reinterpret_cast<const uint64_t*>(S + o_segrows + r->seg_words * 4 + r->h_prog.size() * sizeof(VhProgOp));
  P.set = r->place_sets(x->h_segrows, S + o_segrows);
  if (planes_ready) {      // the program over the planes, into the staging block behind the sets (BEFORE the upload reads it) ...
    planes_prog.set = P.set;
    memcpy(x->h_segrows + planes_word, &planes_prog, sizeof(VhBitsProg));
  }
  if (sliced_prebuilt) {   // ... and where the kernel finds it
    planes_ref.B = reinterpret_cast<const VhBitsProg*>(S + o_segrows + planes_word * 4);
    planes_ref.L.planes = sliced_use->plane[0].ptr; planes_ref.L.stride = sliced_use->plane[0].stride; planes_ref.L.pitch = sliced_use->pitch;
  }
  if (pagg_want) {         // the descriptor of the aggregate on the planes (zeros when the rule did not hold after all), and the kernel's view
    memcpy(x->h_segrows + pagg_word, &pagg_desc, sizeof(VhPlaneAggDesc));
    if (plane_agg) {
      const VhPredPack* f = pagg_filter ? sliced_use : pagg_v;
      pagg_ref.B = pagg_filter ? reinterpret_cast<const VhBitsProg*>(S + o_segrows + planes_word * 4) : nullptr;
      pagg_ref.D = reinterpret_cast<const VhPlaneAggDesc*>(S + o_segrows + pagg_word * 4);
      pagg_ref.F.planes = f->plane[0].ptr; pagg_ref.F.stride = f->plane[0].stride; pagg_ref.F.pitch = f->pitch;
      pagg_ref.V.planes = pagg_v->plane[0].ptr; pagg_ref.V.stride = pagg_v->plane[0].stride; pagg_ref.V.pitch = pagg_v->pitch;    }
  }
  if (mode == VH_MODE_HASH) {
    P.hkeys = reinterpret_cast<uint64_t*>(S + o_hkeys);
    P.htags = P.key_words > 1 ? reinterpret_cast<uint32_t*>(S + o_htags) : nullptr;
  } else {
    P.present = reinterpret_cast<uint8_t*>(S + o_present);
  }
  for (int j = 0; j < P.nmetric; ++j) P.m[j].state = S + o_state[j];
  r->d_out_count = reinterpret_cast<unsigned long long*>(S + o_outcount);
  P.part_count = part_balanced ? reinterpret_cast<uint32_t*>(S + o_pcount) : nullptr;
  P.heavy_mark = heavy_marks ? reinterpret_cast<uint32_t*>(S + o_heavy) : nullptr;
  P.heavy_only = g_heavy.only;
  if (mode == VH_MODE_DENSE_PART || hpart) {
    P.tuples = reinterpret_cast<uint64_t*>(S + o_tuples);
    P.extent_missing = reinterpret_cast<uint16_t*>(S + o_emiss);
    P.extent_part = reinterpret_cast<uint8_t*>(S + o_epart);
    if (P.nlevel == 2) {
      P.tuples2 = reinterpret_cast<uint64_t*>(S + o_tuples2);
      P.extent_missing2 = reinterpret_cast<uint16_t*>(S + o_emiss2);
      P.extent_part2 = reinterpret_cast<uint8_t*>(S + o_epart2);
      P.l2 = reinterpret_cast<uint32_t*>(S + o_l2);
    }
  }
  for (size_t k = 0; k < r->filter_bitset_cols.size(); ++k) {
    const VhColumn& c = t->cols[r->filter_bitset_cols[k]];
    for (uint32_t sgi : live) if (!c.bs_offsets[sgi]) return vh_fail(VH_E_INVALID, "bitset column %d of segment %u was never synced", r->filter_bitset_cols[k], sgi);
    P.fbs_offs[k] = reinterpret_cast<const uint64_t* const*>(S + o_fbs[k]);
    if (nseg) HIP_TRY(hipMemcpy(S + o_fbs[k], c.bs_offsets.data(), nseg * 8, hipMemcpyHostToDevice));
  }
  if (P.nbitset) {
    for (int b = 0; b < P.nbitset; ++b) {
      P.dset_keys[b] = hpart ? nullptr : reinterpret_cast<uint64_t*>(S + o_dkeys[b]);
      P.dset_tags[b] = P.bs_wide[b] && !hpart ? reinterpret_cast<uint32_t*>(S + o_dtags[b]) : nullptr;
      const VhColumn& c = t->cols[bitset_col[b]];
      P.bs_offs[b] = reinterpret_cast<const uint64_t* const*>(S + o_bsptr[b][0]);
      P.bs_vals[b] = reinterpret_cast<const void* const*>(S + o_bsptr[b][1]);
      if (nseg) {
        // (the compiled scan of the hashed partitioning reads the 32-bit copies of the offsets: the same table of pointers, other arrays)
        HIP_TRY(hipMemcpy(S + o_bsptr[b][0], hpart && hp_off32 ? (const void*)c.bs_offsets32.data() : (const void*)c.bs_offsets.data(), nseg * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S + o_bsptr[b][1], c.bs_values.data(), nseg * 8, hipMemcpyHostToDevice));
      }
    }
  }
  for (int i = 0; i < P.ngroup; ++i) r->d_out_key[i] = S + o_okey[i];
  for (int j = 0; j < P.nmetric; ++j) r->d_out_state[j] = S + o_ostate[j];
  if (r->topk_active) {
    r->d_topk_keys = reinterpret_cast<uint64_t*>(S + o_tkkeys);
    r->d_topk_state = reinterpret_cast<VhTopkState*>(S + o_tkstate);
    for (int i = 0; i < P.ngroup; ++i) r->d_out_key2[i] = S + o_okey2[i];
    for (int j = 0; j < P.nmetric; ++j) r->d_out_state2[j] = S + o_ostate2[j];
  }
  return VH_OK;
}

// What follows a query's scan on its stream: the event behind the scan, whether the result takes the one-launch tail, and the merge of a dense
// result's private copies where it does not. launch() ends with it; a batch calls it for a member whose scan it launched itself — fused with
// others', or alone after all (vh_query_agg_batch, vhh_finalize.h).
static int query_scan_tail(vh_result* r, VhExec* x) {
  const VhPlanDev& P = r->plan;
  hipStream_t st = x->stream();
  HIP_TRY(hipEventRecord(x->ev[2], st));
  HIP_TRY(hipGetLastError());
  // a small dense result that will go straight into pinned host memory (result_finalize's `direct`): its whole tail is one launch there
  // ... bounded by the states that ONE block then reads (entries x private copies x metrics), not by the entries alone: beyond ~64 K of them
  // the three parallel launches it replaces are the faster tail
  r->small_tail = r->mode != VH_MODE_HASH && r->out_cap <= VH_SMALL_TAIL_MAX && r->out_region_bytes <= (8u << 20) && !r->topk_active && !r->hp_chunks &&
                  (uint64_t)r->out_cap * (uint64_t)std::max(1, r->nxcd) * (uint64_t)std::max(1, (int)P.nmetric) <= VH_SMALL_TAIL_STATES &&
                  !r->device_rows && !knobs().no_direct_emit && !test_env("VH_TEST_NO_SMALL_TAIL");
  if (r->mode != VH_MODE_HASH && r->nxcd > 1) {
    r->unmerged = true;
    if (!r->small_tail) { if (int mrc = merge_copies_now(r, st)) return mrc; }
  }
  return VH_OK;
}

int QueryBuild::launch() {
  int rc = VH_OK;
  // ---------------- init + launch
  hipStream_t st = x->stream();
  if (int frc = derived_fence(t, st)) return frc;      // derived layouts refreshed for this query are still on the table's stream
  HIP_TRY(hipEventRecord(x->ev[0], st));
  VhInitArgs IA{};              // everything that is cleared goes into one launch (init_regions_kernel)
  auto clear = [&](void* ptr, size_t bytes, uint32_t byte_pattern) {
    if (!bytes) return;
    const uint64_t units = (bytes + 15) / 16;                       // (regions are padded to 256 B: rounding up stays inside)
    if (IA.n == VH_INIT_MAX) { (void)hipMemsetAsync(ptr, (int)(byte_pattern & 0xFFu), bytes, st); return; }
    IA.p[IA.n] = static_cast<char*>(ptr); IA.end[IA.n] = (IA.n ? IA.end[IA.n - 1] : 0) + units; IA.pat[IA.n] = byte_pattern * 0x01010101u; ++IA.n;
  };
  clear(P.counters, 512, 0);   // counters + out_count (adjacent 256 B slots)
  IA.cp_src = x->h_segrows; IA.cp_dst = reinterpret_cast<uint32_t*>(S + o_segrows); IA.cp_words = (uint32_t)r->plan_words;      // (copied by init_regions_kernel below: the counters' clear is always there)
  if (mode == VH_MODE_HASH && !hpart) {      // (hashed partitioning writes its group records as a compact list: nothing to pre-fill)
    if (P.hrec_bytes) {          // records: empty key + the metrics' identities, one template for every slot
      VhRecordTemplate T{};
      T.w[0] = VH_HASH_EMPTY;
      for (int j = 0; j < P.nmetric; ++j)
        memcpy(reinterpret_cast<char*>(T.w) + rec_off[j], &P.m[j].ident, vh_sop_bytes(P.m[j].sop()));
      const uint64_t nwords = table_n * (P.hrec_bytes / 8);
      hipLaunchKernelGGL(fill_records_kernel, dim3((unsigned)std::min<uint64_t>((nwords + 255) / 256, (uint64_t)g_ctx.num_cu * 16)), dim3(256), 0, st,
                         P.hkeys, nwords, P.hrec_bytes / 8, T);
      HIP_TRY(hipGetLastError());
    }
    else if (P.key_words == 1) clear(P.hkeys, table_n * sizeof(uint64_t), 0xFF);
    else clear(P.htags, table_n * sizeof(uint32_t), 0);
  }
  // (DENSE_PART whose blocks each keep a private copy of their range store EVERY group of every copy, present or not: clearing 19
  // copies of C3's tables, 30 MB, before every query was two thirds of this launch's 17 us. A range's sole block stores present groups only.)
  const bool part_owned = mode == VH_MODE_DENSE_PART && part_bpp > 1 && (nxcd == part_bpp || part_balanced) && !knobs().skip_phase2 && P.total_units != 0;      // (no units: phase 2 does not run and nobody stores the copies — they are cleared like any table)
  if (zero_end > zero_begin && !part_owned) clear(S + zero_begin, zero_end - zero_begin, 0);
  r->zero_begin = S + zero_begin; r->zero_end = S + zero_end;
  for (int b = 0; b < P.nbitset && !hpart; ++b) {
    if (P.bs_wide[b]) clear(P.dset_tags[b], (P.dset_mask[b] + 1) * 4, 0);
    else clear(P.dset_keys[b], (P.dset_mask[b] + 1) * 8, 0xFF);
  }
  VhHpArgs* d_hpargs = nullptr;
  if (hpart) {          // the pools behind the scan (vh_hpart.h): descriptors for the kernels, fill arrays and small tables cleared with everything else
    VhHpArgs& HA = r->hp_args;
    memset(&HA, 0, sizeof(HA));
    HA.units = hp_units; HA.pk = hp_pack ? 1 : 0; HA.pk_pbits = hp_pbits; HA.pk_idbits = hp_idbits;
    HA.passes = P.hp_passes; HA.gslots = P.hp_gslots; HA.sslots = P.hp_sslots; HA.keys_off = P.hp_keys_off; HA.set_off = P.hp_set_off;
    HA.bitset_j = -1;
    for (int j = 0; j < P.nmetric; ++j) if (P.m[j].sop() == SOP_BITSET) HA.bitset_j = j;
    HA.list_cap = capacity; HA.chunk = hp_chunk; HA.ablate = knobs().hp_ablate; HA.slice_levels_cap = P.slice_levels_cap; HA.heavy_mark = P.heavy_mark;
    // no HAVING and no top-N to look at the groups first: the aggregation kernel emits them itself (C5: no 0.85 GB list, no 0.85 ms kernel)
    HA.direct = r->hp_direct ? 1 : 0; HA.ngroup = P.ngroup; HA.out_count = r->d_out_count;
    HA.nchunks = r->hp_chunks; HA.chunk_rows = r->hp_chunk_rows;
    for (int i = 0; i < P.ngroup; ++i) { HA.out_key[i] = r->d_out_key[i]; HA.gkey_shift[i] = P.g[i].key_shift(); HA.gesize[i] = (uint32_t)vh_elem_size(P.g[i].type()); }
    for (int j = 0; j < P.nmetric; ++j) { HA.out_state[j] = r->d_out_state[j]; HA.mesize[j] = (uint32_t)vh_elem_size(r->metric_elem[j]); }
    for (int k = 0; k < 1; ++k) {
      VhHpKind& K = HA.k[k];
      char* meta = S + hpo[k].meta;
      K.a.stride = K.b.stride = (uint32_t)(HP_ET / hp_units) + (uint32_t)knobs().ext_pad / (uint32_t)hp_units;
      K.a.tuples = reinterpret_cast<uint64_t*>(S + hpo[k].ta); K.a.fill = reinterpret_cast<uint16_t*>(S + hpo[k].fa); K.a.tag = reinterpret_cast<uint8_t*>(S + hpo[k].ga);
      K.a.max_extents = (uint32_t)std::min<uint64_t>(hpo[k].maxa, 0xFFFFFFF0ull);
      K.b.tuples = reinterpret_cast<uint64_t*>(S + hpo[k].tb); K.b.fill = reinterpret_cast<uint16_t*>(S + hpo[k].fb); K.b.tag = reinterpret_cast<uint8_t*>(S + hpo[k].gb);
      K.b.max_extents = (uint32_t)std::min<uint64_t>(hpo[k].maxb, 0xFFFFFFF0ull);
      K.b.ovf_base = K.b.max_extents; K.b.ovf_cursor = nullptr;      // (pool b's slices carry their own overflow regions and cursors)
      // the scan kernel's view of pool a (the second pool's fields of the plan: DENSE_PART's two-level plans are the other user); behind its positional
      // levels the shared overflow region the scan's writer takes extents from (counters[10])
      P.tuples2 = K.a.tuples; P.extent_missing2 = K.a.fill; P.extent_part2 = K.a.tag; P.max_extents2 = K.a.max_extents; P.ext_tuples2 = (int32_t)K.a.stride;
      K.a.ovf_base = (uint32_t)std::min<uint64_t>((uint64_t)P.pos_levels2 * (uint64_t)grid * HP_FAN, K.a.max_extents);
      K.a.ovf_cursor = P.counters + 10;
      K.count = reinterpret_cast<uint32_t*>(meta + 8);
      K.slice = reinterpret_cast<uint32_t*>(meta + 8 + (size_t)HP_FAN * 4);
      clear(K.a.fill, (size_t)K.a.max_extents * 2, 0);
      clear(K.b.fill, (size_t)K.b.max_extents * 2, 0);
      clear(meta, hp_meta_bytes, 0);
    }
    d_hpargs = reinterpret_cast<VhHpArgs*>(S + o_hpargs);
    r->d_hp_args = d_hpargs; r->hp_scan_blocks = grid;
    HIP_TRY(hipMemcpyAsync(d_hpargs, &HA, sizeof(HA), hipMemcpyHostToDevice, st));
  }
  if (part_balanced) clear(P.part_count, VH_MAX_PART * VH_PART_COUNT_WAYS * sizeof(uint32_t), 0);
  if (heavy_marks) clear(P.heavy_mark, 65536 / 8, 0);
  if (mode == VH_MODE_DENSE_PART || hpart) {
    clear(P.extent_missing, (size_t)P.max_extents * sizeof(uint16_t), 0);
    clear(P.extent_part, (size_t)P.max_extents, 0xFF);
    if (P.nlevel == 2) {
      clear(P.extent_missing2, (size_t)P.max_extents2 * sizeof(uint16_t), 0);
      clear(P.extent_part2, (size_t)P.max_extents2, 0xFF);
      clear(P.l2, (VH_L2_WORDS + VH_MAX_PART) * sizeof(uint32_t), 0);
    }
  }
  for (int j = 0; j < P.nmetric; ++j) {
    if (P.m[j].ident == 0 || P.hrec_bytes || hpart || part_owned) continue;      // (part_owned: phase 2's blocks store every group of every copy that is read)
    rc = fill_states(P.m[j].state, table_n, vh_sop_bytes(P.m[j].sop()), P.m[j].ident, st);
    if (rc) { return rc; }
  }
  if (IA.n) {
    const uint64_t units = IA.end[IA.n - 1];
    hipLaunchKernelGGL(init_regions_kernel, dim3((unsigned)std::min<uint64_t>((units + 255) / 256, (uint64_t)g_ctx.num_cu * 16)), dim3(256), 0, st, IA);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(x->ev[1], st));
  if (lanes && !jk)       // the pre-built lanes kernels read 4-byte predicate columns only (vh_preload<NP, false>)
    for (int k = 0; k < P.npred; ++k) if (P.pred_width[k] != 4) { P.pred_slot[k] = (uint8_t)pred_wide_slot[k]; P.pred_width[k] = 4; }
  bool narrowed = false;
  for (int k = 0; k < P.npred; ++k) narrowed |= P.pred_width[k] != 4;
  if (jk) { narrowed = jshape.pp_nplanes || jshape.pp_sliced; for (int k = 0; k < jshape.npred; ++k) narrowed |= jshape.pred[k].width != vh_elem_size(jshape.pred[k].type); }
  r->hpart = hpart;
  VhWhatRan w;
  w.hpart = hpart; w.fast = fastj || jk; w.fastj = fastj; w.jk = jk != nullptr; w.lanes = lanes; w.lds_hash = P.lds_hash_slots != 0;
  w.packed = packed; w.packed_compressed = packed_compressed; w.packed_bits = packed_bits; w.packed_rec = packed_rec;
  w.narrowed = narrowed; w.hp_pack = hp_pack; w.dense_part = mode == VH_MODE_DENSE_PART; w.gid_bits = P.gid_bits != 0; w.tuple4 = P.tuple4 != 0;
  w.pp_planes = jshape.pp_nplanes != 0; w.pp_sliced = jshape.pp_sliced != 0; w.qpay = jshape.qpay != 0;
  w.has_set = has_set; w.set_search = set_search; w.set_truth = set_truth; w.build_pending = build_pending;
  w.grouped = grouped; w.gplanes = gplanes; w.subtrim = subtrim; w.gpspan = gpspan; w.sliced_prebuilt = sliced_prebuilt; w.plane_agg = plane_agg;
  w.plane_jit = plane_agg && pagg_jk != nullptr;
  r->info.reserved = vh_info_compose(w);
  r->plane_sink = !plane_agg ? 0u : pagg_desc.rows ? 2u : 1u;      // (vh_result_plane_sink: `reserved` has no bit left for it)
  r->fast_scan = w.fast;      // (VH_INFO_FAST as planned: a pre-built reader of the planes clears the bit in the result's word)
  if (r->hp_chunks) memset(x->h_chunk, 0, VH_HP_CHUNKS * sizeof(unsigned long long));      // (what the context's previous query left there)
  // a second pass over heavy level-A partitions of a hashed partitioning: from the first pass's tuples when this plan's table can take them as
  // they are (one key word laid out as the first pass's, narrow ids) — else from the table's rows behind the bitmap, like any heavy range
  bool from_tuples = false;
  if (const vh_result* m = g_heavy.only ? g_heavy.tuples_of : nullptr) {
    const VhPlanDev& M = m->plan;
    from_tuples = mode == VH_MODE_HASH && !hpart && !jk && P.key_words == 1 && M.key_words == 1 && P.ngroup == M.ngroup && P.nmetric == M.nmetric && P.nbitset <= 1 && m->d_hp_args;
    for (int i = 0; i < P.ngroup && from_tuples; ++i) from_tuples = P.g[i].key_shift() == M.g[i].key_shift() && P.g[i].key_word() == M.g[i].key_word();
    for (int b = 0; b < P.nbitset && from_tuples; ++b) from_tuples = !P.bs_wide[b];
    if (from_tuples) {
      VhHeavyTuples HT{};
      HT.HA = m->d_hp_args; HT.src_blocks = (uint32_t)m->hp_scan_blocks;
      HT.units = m->hp_args.units; HT.pk = m->hp_args.pk; HT.pbits = m->hp_args.pk_pbits; HT.idbits = m->hp_args.pk_idbits;
      HT.nmetric = P.nmetric; HT.bitset_j = -1;
      for (int j = 0; j < P.nmetric; ++j) {
        if (P.m[j].sop() == SOP_BITSET) HT.bitset_j = j;
        from_tuples = from_tuples && (P.m[j].sop() == SOP_BITSET) == (M.m[j].sop() == SOP_BITSET);
        HT.tshift[j] = (uint8_t)M.m[j].tshift(); HT.tbits[j] = M.m[j].tbits; HT.tbytes[j] = (uint8_t)vh_sop_bytes(M.m[j].sop()); HT.tsext[j] = vh_sop_sext(M.m[j].sop()) ? 1 : 0;
      }
      if (from_tuples) { vh_launch_heavy_tuples(P, HT, g_ctx.num_cu, st); r->kernel = HT.units == 2 ? "hp_heavy_tuples_kernel<2, false>" : HT.pk ? "hp_heavy_tuples_kernel<1, true>" : "hp_heavy_tuples_kernel<1, false>"; }
    }
  }
  if (g_heavy.only && !from_tuples && g_heavy.epoch != t->sync_epoch)       // the table has moved on since the first pass: its rows are no longer the rows that pass saw
    return vh_fail(VH_E_RANGE, "second pass over heavy ranges: the table changed since the first pass");      // (heavy_pass_finish gives up; the caller re-plans the whole query)
  if (from_tuples) {
  } else if (P.total_units && plane_agg && o.fuse && (!pagg_jit || pagg_jk)) {      // (a member that asked for the compiled form and has no kernel of its own is answered as the single query it is)
    // A member of a batch whose scan may share a fused launch (vh_query_agg_batch): everything up to ev[1] is enqueued; the scan and what
    // follows it are the batch's to launch, once it knows the groups. The plan goes by value: it is complete here.
    VhDeferredScan& d = o.fuse->scan[o.fuse->member];
    d.r = r; d.x = x; d.P = P; d.A = pagg_ref; d.B = pagg_filter ? planes_prog : VhBitsProg{}; d.D = pagg_desc; d.grid = grid; d.lds_table = lds_table; d.xcd_private = nxcd > 1; d.v_serial = pagg_v->serial;
    d.f_serial = (pagg_filter ? sliced_use : pagg_v)->serial; d.segrows = x->h_segrows;
    d.chunks_per_seg = (uint32_t)std::max<uint64_t>(1, (t->padded_rows + VH_SLICED_CHUNK_ROWS - 1) / VH_SLICED_CHUNK_ROWS);
    d.pagg_jk = pagg_jk;      // (a compiled candidate: vh_batch.h)
    if (pagg_jk) d.js = pagg_shape;
    *out = holder.release();
    done = true;
    return VH_OK;
  } else if (P.total_units) {
    scan_dispatch(VhScanLaunch{grid});
    if (hpart) {
      vh_launch_hpart(P, d_hpargs, hp_units, g_ctx.num_cu, grid, hp_ring_nb, st);
      if (!r->hp_chunks) HIP_TRY(vh_jit_launch_hpagg(jk, P, d_hpargs, hp_bpp, 0, HP_FAN * hp_bpp, lds_table, st));
      else if (r->hp_one_launch) {      // regions without streaming: one launch, every region's row count into pinned memory behind it
        HIP_TRY(vh_jit_launch_hpagg(jk, P, d_hpargs, hp_bpp, 0, HP_FAN * hp_bpp, lds_table, st));
        for (int c = 0; c < r->hp_chunks; ++c) hipLaunchKernelGGL(publish_count_kernel, dim3(1), dim3(64), 0, st, x->h_chunk + c, r->d_out_count + c);
        for (int c = 0; c < r->hp_chunks; ++c) HIP_TRY(hipEventRecord(x->ev_chunk[c], st));
      } else {
        // chunk c = level-A partitions [c * per, (c + 1) * per), alternately on the query's stream and on `aux` (both behind level B), each
        // followed by its row count into pinned memory and an event the host waits for (result_finalize)
        const int per = HP_FAN / r->hp_chunks;
        HIP_TRY(hipEventRecord(x->ev_fork, st));
        HIP_TRY(hipStreamWaitEvent(x->aux, x->ev_fork, 0));
        for (int c = 0; c < r->hp_chunks; ++c) {
          hipStream_t cs = (c & 1) ? x->aux : st;
          HIP_TRY(vh_jit_launch_hpagg(jk, P, d_hpargs, hp_bpp, c * per, per * hp_bpp, lds_table, cs));
          hipLaunchKernelGGL(publish_count_kernel, dim3(1), dim3(64), 0, cs, x->h_chunk + c, r->d_out_count + c);
          HIP_TRY(hipEventRecord(x->ev_chunk[c], cs));
        }
        for (int c = 0; c < r->hp_chunks; ++c) if (c & 1) HIP_TRY(hipStreamWaitEvent(st, x->ev_chunk[c], 0));      // the query's stream ends behind every chunk
      }
    }
    if (mode == VH_MODE_DENSE_PART) {
      const bool skip_phase2 = knobs().skip_phase2;     // measurement only (wrong results): phase 1 alone between the events
      if (P.nlevel == 2 && !skip_phase2) vh_launch_part_split(P, split_bpp, split_ring, st);
      if (!skip_phase2) {
        if (jit_pagg()) HIP_TRY(vh_jit_launch_pagg(jk, P, part_bpp, lds_table, st));      // phase 2 compiled for this plan's tuple layout
        else vh_launch_part_agg(P, part_bpp, lds_table, st);
      }
    }
  }
  if (int trc = query_scan_tail(r, x)) return trc;
  *out = holder.release();
  done = true;
  return VH_OK;
}

// One tick per query (a plan that starts over keeps it): what the layouts this plan reads are stamped with (layout_use). When the outermost
// holder ends, a budget that a refresh pushed past — the table grew, a projection was rebuilt wider — is restored at the cost of layouts
// this plan does not read, and the result says whether anything was evicted on its behalf.
// A sharded query's summary pass and the heavy second pass of a hashed partitioning are further passes of ONE query: they take a tick of
// their own (what they hold is safe from their own builds) but count as no use, and what they evict is reported on the query's result.
// A BATCH (vh_query_agg_batch) holds the outer tick itself, over all its members' plans and its fused launches: every layout any member
// reads carries the one stamp, so no later member's build and no trim evicts the planes of a scan that is not enqueued yet — table_quiesce
// would find that member's stream idle and free them under the kernel to come. Its members' own ticks are passive (g_plan_depth); the trim
// runs once, when the batch's tick ends, still under the table's lock; g_plan_evicted then tells the batch what to report (out == nullptr).
struct PlanTick {
  vh_table* t; vh_result** out; bool outer, further, was_unstamped;
  PlanTick(vh_table* t_, vh_result** out_, bool further_) : t(t_), out(out_), outer(g_plan_depth++ == 0), further(further_), was_unstamped(g_plan_unstamped) {
    if (!outer) return;
    ++t->use_tick;
    g_plan_evicted = g_plan_carry; g_plan_carry = false;
    g_plan_unstamped = further;
    if (g_preparing && !further) g_prepare_reads.clear();
  }
  ~PlanTick() {
    --g_plan_depth;
    if (!outer) return;
    g_plan_unstamped = was_unstamped;
    if (!t->layout_budget) return;
    derived_trim(t, true);
    if (further) g_plan_carry = g_plan_evicted;
    else if (g_plan_evicted && out && *out) (*out)->info.reserved |= VH_INFO_EVICTED;
  }
};
static int query_launch_locked(vh_table* t, VhExec* x, const vh_plan* p, vh_result** out, const VhLaunchOpts& o) {
  if (int src = sync_resolve(t)) return src;      // a batched sync may still be on its way: its rows and its share of the stats, before anything is planned
  PlanTick tick(t, out, o.summary_out != nullptr || g_heavy.only != nullptr);
  QueryBuild b(t, x, p, out, o);
  int (QueryBuild::* const steps[])() = {&QueryBuild::shape_filter, &QueryBuild::snapshot_segments, &QueryBuild::shape_groups, &QueryBuild::shape_metrics,
                                         &QueryBuild::choose_organisation, &QueryBuild::plan_hashed_partitioning, &QueryBuild::choose_projection,
                                         &QueryBuild::compile_kernel, &QueryBuild::decompose_work, &QueryBuild::layout_scratch, &QueryBuild::launch};
  const bool timed = knobs().times;
  double us[12] = {};
  int k = 0;
  for (auto step : steps) {
    const auto s0 = timed ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    if (int rc = (b.*step)()) return rc;
    if (timed) us[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - s0).count();
    ++k;
    if (b.done) break;
  }
  if (timed) fprintf(stderr, "vh plan steps (us): filter %.1f, segments %.1f, groups %.1f, metrics %.1f, organisation %.1f, hpart %.1f, projection %.1f, kernel %.1f, work %.1f, scratch %.1f, launch %.1f\n",
                     us[0], us[1], us[2], us[3], us[4], us[5], us[6], us[7], us[8], us[9], us[10]);
  return VH_OK;
}

