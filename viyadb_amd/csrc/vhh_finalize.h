// vhh_finalize.h — host side of libviya_hip, part of viya_hip.hip's translation unit (included there, in order; not a stand-alone header):
// the end of a query: emission, delivery to pinned host memory, verdict and re-plan loop; vh_query_agg, vh_table_prepare.
// The end of a query is a host wait for a few hundred microseconds to a few milliseconds of device work: poll the event
// (a blocking hipStreamSynchronize adds tens of microseconds of wake-up latency to every query), fall back to a
// blocking wait when the work turns out to be long.
static hipError_t wait_event_spinning(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return hipEventSynchronize(ev);
  }
}

// The second pass of a hashed partitioning that marked heavy ranges (VhPlanDev::heavy_mark): the caller's plan once more, through the plain hash
// organisation, over the rows of exactly those ranges (the generic scan drops every other survivor behind its key: VhPlanDev::heavy_only) — a group
// with a tenth of the table's rows, or with more ids than a range's LDS set takes, costs its query that, not the whole organisation. In two steps,
// so that a big result's rows cross PCIe WHILE the pass scans (C5 with a hot key: 10 ms of copy over 8.5 ms of scan): heavy_pass_launch enqueues
// the pass on a context of its own, heavy_pass_finish waits for it (and re-runs it with a bigger table when that one filled). H.r2: the
// finalised result (nullptr: it could not be had — the caller falls back as before).
static int result_finalize(vh_result* r, int* retry, const vh_plan* plan = nullptr);
struct VhHeavyRun { VhExec* x2 = nullptr; vh_result* r2 = nullptr; vh_plan p2{}; uint64_t cap = 0, ids_bound = 0; bool from_tuples = false; };
static int heavy_pass_enqueue(vh_result* r, VhHeavyRun& H) {
  vh_table* t = r->table;
  std::lock_guard<std::mutex> lk(t->mu);
  g_heavy.only = r->plan.heavy_mark; g_heavy.ids_bound = H.ids_bound; g_heavy.allow_mark = false;
  g_heavy.tuples_of = H.from_tuples ? r : nullptr; g_heavy.epoch = r->launch_epoch;
  VhLaunchOpts o;
  o.rp.cap_override = H.cap; o.rp.force_hash = true; o.rp.no_hpart = true;
  const int rc = query_launch_locked(t, H.x2, &H.p2, &H.r2, o);
  g_heavy = VhHeavyCtx{};
  if (g_plan_carry) { r->info.reserved |= VH_INFO_EVICTED; g_plan_carry = false; }      // (what the pass evicted is the query's to report)
  if (rc) H.r2 = nullptr; else H.r2->exec = H.x2;
  return rc;
}
static void heavy_pass_drop(vh_result* r, VhHeavyRun& H) {
  if (H.r2) { H.r2->exec = nullptr; delete H.r2; H.r2 = nullptr; }
  if (H.x2) { (void)hipStreamSynchronize(H.x2->stream()); exec_release(r->table, H.x2); H.x2 = nullptr; }
  (void)hipGetLastError();
}
static void heavy_pass_launch(vh_result* r, const vh_plan* plan, uint64_t ranges, uint64_t tuples_bound, uint64_t whole_partitions, VhHeavyRun& H) {
  H.from_tuples = ranges == whole_partitions * 256ull && !test_env("VH_HEAVY_RESCAN");      // (every marked range lies in a partition that was left out whole: its tuples are in pool a)
  if (exec_acquire(r->table, &H.x2, false) != VH_OK) { H.x2 = nullptr; return; }      // (never waits for a context while holding one: two such queries would wait for each other — the caller re-plans instead)
  H.p2 = *plan;
  H.p2.flags = (H.p2.flags | VH_PLAN_FORCE_HASH | VH_PLAN_NO_JIT | VH_PLAN_NO_FAST | VH_PLAN_NO_LANES | VH_PLAN_NO_HPART) & ~(uint32_t)(VH_PLAN_FORCE_JIT | VH_PLAN_FORCE_HPART | VH_PLAN_FORCE_LANES);
  H.p2.groups_hint = 0;
  H.cap = 1ull << 16;
  while (H.cap < ranges * 8192ull && H.cap < (1ull << 30)) H.cap <<= 1;      // (a range holds ~500 groups when the keys are spread evenly; heavy_pass_finish regrows)
  H.ids_bound = 2 * tuples_bound + 1024;
  if (heavy_pass_enqueue(r, H)) heavy_pass_drop(r, H);
}
static void heavy_pass_finish(vh_result* r, VhHeavyRun& H) {
  for (int attempt = 0; H.r2; ++attempt) {
    int retry2 = 0;
    const int rc = result_finalize(H.r2, &retry2);
    if (!rc && !retry2) { H.r2->stream_quiet = true; H.x2 = nullptr; return; }      // (the result owns the context from here)
    H.r2->exec = nullptr; delete H.r2; H.r2 = nullptr;
    if (rc || retry2 != 1 || attempt >= 5) break;                               // anything but a full table: give up, the caller falls back
    H.cap <<= 2;
    if (heavy_pass_enqueue(r, H)) break;
  }
  heavy_pass_drop(r, H);
}

// returns VH_OK, or a positive "retry" request: 1 = grow hash table, 2 = fall back to hash
static int result_finalize(vh_result* r, int* retry, const vh_plan* plan) {
  VhExec* x = r->exec;   // staging buffers, scratch and events of this query's context
  const VhPlanDev& P = r->plan;
  hipStream_t st = x->stream();
  *retry = 0;
  // pinned staging buffer (two alternate per context: a zero-copy view stays readable after vh_result_free until the
  // second-next query); a re-planned attempt of the same query reuses its slot. Small results take the output region as it lies in the
  // scratch (one copy, or none: direct emission below); big ones are PACKED on their way out — a staging buffer for the rows that
  // exist, not for the rows the tables could hold (C5: 0.7 GB instead of 2.7 GB per slot; what does not fit the GPU's own NUMA node
  // is copied to at half the rate).
  const int slot = r->h_slot >= 0 ? r->h_slot : (x->h_out_next ^= 1);
  r->h_slot = slot;
  auto stage = [&](size_t bytes) -> int {
    if (x->h_out_bytes[slot] >= bytes) return VH_OK;
    if (x->h_out[slot]) HIP_TRY(hipHostFree(x->h_out[slot]));
    x->h_out[slot] = nullptr; x->h_out_bytes[slot] = 0;
    const size_t nb = std::max<size_t>(bytes + bytes / 8, 1 << 20);
    // coherent (fine-grained): the emission kernel writes small results straight into this buffer, and the host must see
    // them when the event behind the kernel has completed, whatever HIP_HOST_COHERENT says
    HIP_TRY(host_alloc_near_device((void**)&x->h_out[slot], nb, hipHostMallocCoherent));
    x->h_out_bytes[slot] = nb;
    return VH_OK;
  };
  const bool env_no_direct = knobs().no_direct_emit;
  const bool one_shot = r->out_region_bytes <= (8u << 20) && !r->topk_active && !r->hp_chunks;      // (a streamed result's rows are packed on their way out: never the region as a whole)
  const bool direct = one_shot && r->mode != VH_MODE_HASH && !env_no_direct && !r->device_rows;
  if (one_shot) { if (int src = stage(r->out_region_bytes)) return src; }
  // Small results of the dense paths are written by the emission kernel straight into that pinned host buffer
  // (posted PCIe writes, coalesced per column) and a one-wave kernel publishes the 512-byte header behind them: no
  // DMA-engine copy at the end of the query (its start-up costs 20-100 us, more than the 2 MB it moves).
  if (direct) {
    for (int i = 0; i < P.ngroup; ++i) r->d_out_key[i] = x->h_out[slot] + r->off_key[i];
    for (int j = 0; j < P.nmetric; ++j) r->d_out_state[j] = x->h_out[slot] + r->off_state[j];
  }
  VhEmitArgs A{};
  A.mode = r->mode == VH_MODE_DENSE_PART ? VH_MODE_DENSE_GLOBAL : r->mode; A.ngroup = P.ngroup; A.nmetric = P.nmetric; A.key_words = P.key_words;
  A.hstride = P.hrec_bytes ? P.hrec_bytes / 8u : (uint32_t)P.key_words;
  A.n = r->out_cap; A.present = P.present; A.present_carrier = (r->mode == VH_MODE_DENSE_GLOBAL || r->mode == VH_MODE_DENSE_PART) ? P.present_carrier : -1; A.hkeys = P.hkeys; A.htags = P.htags; A.counters = P.counters;
  A.out_count = r->d_out_count;
  A.n_dev = r->hpart ? P.counters + 1 : nullptr;         // hashed partitioning: entries [0, *n_dev) of the table are a compact list of group records
  for (int i = 0; i < P.ngroup; ++i) {
    A.glo[i] = P.g[i].lo; A.gextent[i] = P.g[i].extent; A.gstride[i] = P.g[i].stride;
    A.gtype[i] = P.g[i].type(); A.gkey_word[i] = P.g[i].key_word(); A.gkey_shift[i] = P.g[i].key_shift();
    A.out_key[i] = r->d_out_key[i];
  }
  for (int j = 0; j < P.nmetric; ++j) {
    A.state[j] = P.m[j].state; A.out_state[j] = r->d_out_state[j]; A.sop[j] = P.m[j].sop(); A.mtype[j] = (uint8_t)r->metric_elem[j];
    A.state_stride[j] = r->mode == VH_MODE_HASH && P.hrec_bytes ? P.hrec_bytes : (uint32_t)vh_sop_bytes(P.m[j].sop());
  }
  A.nhaving = r->nhaving;
  A.total_groups = P.counters + 6;
  for (int i = 0; i < r->nhaving; ++i) { A.hprog[i] = r->hprog[i]; A.htype[i] = r->htype[i]; }
  for (int i = 0; i < VH_MAX_HAVING_LITS; ++i) A.hlits[i] = r->hlits[i];
  // a small dense result: private copies, emission and header in ONE launch (small_tail_kernel); anything else merges first if nobody has
  const bool fused_tail = r->small_tail && direct && A.n <= VH_SMALL_TAIL_MAX;
  if (r->unmerged && !fused_tail) { if (int mrc = merge_copies_now(r, st)) return mrc; }
  if (fused_tail) {
    VhMergeArgs M;
    merge_args_of(r, &M);
    if (!r->unmerged) M.nxcd = 1;
    hipLaunchKernelGGL(small_tail_kernel, dim3(1), dim3(1024), 0, st, M, A, reinterpret_cast<unsigned long long*>(x->h_out[slot]),
                       reinterpret_cast<const unsigned long long*>(x->scratch + r->out_region_off));
    r->unmerged = false;
    r->tail.kind = VH_TAIL_FUSED;
    if (M.nxcd > 1) r->tail.merged = VH_MERGE_FUSED;
  }
  else if (r->hp_direct && r->nhaving == 0 && !r->topk_active) { r->tail.kind = VH_TAIL_NONE; /* hp_aggregate_kernel wrote the output columns and counted the rows */ }
  else if (A.n <= (4u << 20)) { r->tail.kind = VH_TAIL_EMIT2; hipLaunchKernelGGL(emit_groups_kernel<2>, dim3((unsigned)((A.n + 256 * 2 - 1) / (256 * 2))), dim3(256), 0, st, A); }
  else { r->tail.kind = VH_TAIL_EMIT16; hipLaunchKernelGGL(emit_groups_kernel<16>, dim3((unsigned)((A.n + 256 * 16 - 1) / (256 * 16))), dim3(256), 0, st, A); }
  r->tail.direct = direct ? 1 : 0; r->tail.copies = std::max(1, r->nxcd); r->tail.entries = r->out_cap;
  r->tail.states_per_entry = (uint32_t)P.nmetric; r->tail.region_bytes = r->out_region_bytes;
  HIP_TRY(hipGetLastError());
  if (r->topk_active) {
    // radix select of the top_k-th best sort key among the emitted rows (8 x 8 bits, no host round trip), then keep
    // every row that ties with or beats it. Row count is only known on the device: grids are sized by out_cap.
    VhTopkState init{};
    init.k_remaining = r->topk;
    HIP_TRY(hipMemcpyAsync(r->d_topk_state, &init, sizeof(init), hipMemcpyHostToDevice, st));
    const unsigned g1 = (unsigned)std::min<uint64_t>((r->out_cap + 255) / 256, (uint64_t)g_ctx.num_cu * 8);
    const void* src = r->topk_src_is_key ? r->d_out_key[r->topk_src] : r->d_out_state[r->topk_src];
    hipLaunchKernelGGL(topk_keys_kernel, dim3(g1), dim3(256), 0, st, src, r->topk_elem, (uint32_t)vh_elem_size(r->topk_elem),
                       r->topk_cls, r->topk_desc, (const unsigned long long*)r->d_out_count, r->d_topk_keys);
    for (int shift = 56; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(topk_hist_kernel, dim3(g1), dim3(256), 0, st, (const uint64_t*)r->d_topk_keys,
                         (const unsigned long long*)r->d_out_count, shift, r->d_topk_state);
      hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(64), 0, st, shift, r->d_topk_state);
    }
    VhTopkCompact C{};
    C.ncols = P.ngroup + P.nmetric;
    // formatter rounding ("%.15g" / "%g") makes nearby values compare equal in the reference: the margin that covers it (vh_topk_key.h)
    C.slack = vh_topk_slack(r->topk_cls, r->topk_elem);
    for (int i = 0; i < P.ngroup; ++i) { C.src[i] = r->d_out_key[i]; C.dst[i] = r->d_out_key2[i]; C.esize[i] = (uint32_t)vh_elem_size(P.g[i].type()); }
    for (int j = 0; j < P.nmetric; ++j) {
      C.src[P.ngroup + j] = r->d_out_state[j]; C.dst[P.ngroup + j] = r->d_out_state2[j];
      C.esize[P.ngroup + j] = (uint32_t)vh_elem_size(r->metric_elem[j]);
    }
    hipLaunchKernelGGL(topk_compact_kernel, dim3((unsigned)((r->out_cap + 255) / 256)), dim3(256), 0, st, C,
                       (const uint64_t*)r->d_topk_keys, (const unsigned long long*)r->d_out_count, (unsigned long long)r->topk, r->d_topk_state);
    HIP_TRY(hipGetLastError());
  }
  const char* D = x->scratch + r->out_region_off;
  // packed layout of a big result in the staging buffer: [512-byte header | key columns | state columns], each column `rows` long
  struct Packed { size_t key[VH_MAX_GROUP], state[VH_MAX_METRIC], bytes; };
  auto packed_for = [&](uint64_t rows) {
    Packed L{};
    size_t o = 512;
    for (int i = 0; i < P.ngroup; ++i) { L.key[i] = o; o += (std::max<uint64_t>(rows, 1) * vh_elem_size(P.g[i].type()) + 255) / 256 * 256; }
    for (int j = 0; j < P.nmetric; ++j) { L.state[j] = o; o += (std::max<uint64_t>(rows, 1) * vh_elem_size(r->metric_elem[j]) + 255) / 256 * 256; }
    L.bytes = o;
    return L;
  };
  auto copy_rows = [&](const Packed& L, uint64_t dst_row, uint64_t src_row, uint64_t n, bool second, hipStream_t cs) -> int {
    char* H = x->h_out[slot];
    uint64_t row_bytes = 0;
    for (int i = 0; i < P.ngroup; ++i) row_bytes += vh_elem_size(P.g[i].type());
    for (int j = 0; j < P.nmetric; ++j) row_bytes += vh_elem_size(r->metric_elem[j]);
    if (n * row_bytes >= ((uint64_t)1 << 20) && P.ngroup + P.nmetric <= VH_DELIVER_COLS && knobs().deliver_blocks > 0) {      // (deliver_kernel: why not the DMA engine)
      VhDeliverArgs A{};
      for (int i = 0; i < P.ngroup; ++i) {
        const size_t es = vh_elem_size(P.g[i].type());
        A.src[A.ncols] = (second ? (const char*)r->d_out_key2[i] : (const char*)r->d_out_key[i]) + src_row * es; A.dst[A.ncols] = H + L.key[i] + dst_row * es; A.bytes[A.ncols++] = n * es;
      }
      for (int j = 0; j < P.nmetric; ++j) {
        const size_t es = vh_elem_size(r->metric_elem[j]);
        A.src[A.ncols] = (second ? (const char*)r->d_out_state2[j] : (const char*)r->d_out_state[j]) + src_row * es; A.dst[A.ncols] = H + L.state[j] + dst_row * es; A.bytes[A.ncols++] = n * es;
      }
      hipLaunchKernelGGL(deliver_kernel, dim3((unsigned)knobs().deliver_blocks), dim3(256), 0, cs, A);
      HIP_TRY(hipGetLastError());
      return VH_OK;
    }
    for (int i = 0; i < P.ngroup; ++i) {
      const size_t es = vh_elem_size(P.g[i].type());
      HIP_TRY(hipMemcpyAsync(H + L.key[i] + dst_row * es, (second ? (const char*)r->d_out_key2[i] : (const char*)r->d_out_key[i]) + src_row * es, n * es, hipMemcpyDeviceToHost, cs));
    }
    for (int j = 0; j < P.nmetric; ++j) {
      const size_t es = vh_elem_size(r->metric_elem[j]);
      HIP_TRY(hipMemcpyAsync(H + L.state[j] + dst_row * es, (second ? (const char*)r->d_out_state2[j] : (const char*)r->d_out_state[j]) + src_row * es, n * es, hipMemcpyDeviceToHost, cs));
    }
    return VH_OK;
  };
  // streamed result: every finished chunk's rows go out on the copy stream, packed one chunk behind the other, while the next chunks run.
  // The staging buffer is sized when the first chunk's count is in (the mixed key deals the groups evenly: eight times that, and a bit);
  // should the rest not fit after all, everything is copied once more when all counts are known.
  uint64_t streamed = 0;
  Packed L{};
  if (r->hp_chunks) {
    uint64_t cnt[VH_HP_CHUNKS] = {}, rows_cap = 0;
    bool redo = false;
    for (int c = 0; c < r->hp_chunks; ++c) {
      HIP_TRY(wait_event_spinning(x->ev_chunk[c]));
      cnt[c] = std::min<uint64_t>(reinterpret_cast<volatile unsigned long long*>(x->h_chunk)[c], r->hp_chunk_rows);      // (more: the region overflowed, the attempt is void — flagged in the header)
      if (c == 0) {
        rows_cap = cnt[0] * (uint64_t)r->hp_chunks + cnt[0] / 4 + 65536;
        L = packed_for(rows_cap);
        if (int src = stage(L.bytes)) return src;
      }
      if (streamed + cnt[c] > rows_cap) redo = true;
      if (cnt[c] && !redo) { if (int crc = copy_rows(L, streamed, (uint64_t)c * r->hp_chunk_rows, cnt[c], false, x->copy)) return crc; }
      streamed += cnt[c];
    }
    if (redo) {
      HIP_TRY(hipStreamSynchronize(x->copy));
      L = packed_for(streamed);
      if (int src = stage(L.bytes)) return src;
      uint64_t at = 0;
      for (int c = 0; c < r->hp_chunks; ++c) { if (cnt[c]) { if (int crc = copy_rows(L, at, (uint64_t)c * r->hp_chunk_rows, cnt[c], false, x->copy)) return crc; } at += cnt[c]; }
    }
  }
  VhTopkState tk{};
  if (r->topk_active) HIP_TRY(hipMemcpyAsync(&tk, r->d_topk_state, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  // small results: counters, group count and every output array come back in ONE copy + ONE sync; big ones: the header first
  unsigned long long* const head = one_shot ? reinterpret_cast<unsigned long long*>(x->h_out[slot]) : x->h_counters + 16;
  if (direct) {
    if (!fused_tail) hipLaunchKernelGGL(publish_header_kernel, dim3(1), dim3(64), 0, st, head, reinterpret_cast<const unsigned long long*>(D));
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemcpyAsync(head, D, one_shot ? r->out_region_bytes : 512, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipEventRecord(x->ev[3], st));
  HIP_TRY(wait_event_spinning(x->ev[3]));
  const unsigned long long* hc = head;
  const unsigned long long err = hc[2];
  if (r->hp_chunks) HIP_TRY(hipStreamSynchronize(x->copy));      // (also when the attempt is void: the next one rewrites what the copies read)
  if (err & VH_ERR_HP_WIDE) { *retry = 6; return VH_OK; }        // packed tuples met a value beyond the recorded min / max: the plain hash table
  if (err & VH_ERR_HPART_FULL) { *retry = 4; return VH_OK; }
  if (err & VH_ERR_HASH_FULL) { *retry = 1; return VH_OK; }
  if (err & VH_ERR_PART_FULL) { r->info.passed_recs = hc[0]; *retry = 3; return VH_OK; }   // phase 1 ran to the end: the survivors are counted
  if (err & VH_ERR_RANGE) { *retry = 2; return VH_OK; }
  uint64_t ng = r->hp_chunks ? streamed : hc[32];                                 // rows emitted (after HAVING): the word at byte 256
  r->info.ngroups = r->nhaving ? hc[6] : ng;                                     // agg_map.size()
  if (r->topk_active) ng = tk.out_count;                                          // rows kept by the top-N superset
  r->info.returned_groups = ng;
  r->ngroups_host = ng;
  r->info.passed_recs = hc[0];
  // heavy ranges of a hashed partitioning (hc[11] of them, at most hc[12] tuples): their groups come from a second pass through the plain hash
  // organisation and are appended behind the rows the ranges' kernel wrote
  std::unique_ptr<vh_result> heavy;
  uint64_t n2 = 0;
  VhHeavyRun HR;
  struct HeavyGuard { vh_result* r; VhHeavyRun& H; ~HeavyGuard() { if (H.x2) heavy_pass_drop(r, H); } } heavy_guard{r, HR};      // (an early return leaves no context behind)
  const bool heavy_wanted = r->hpart && P.heavy_mark && hc[11];
  // a big result in one piece: its rows cross PCIe WHILE the pass scans — the staging buffer then has room for the rows the pass can add at most
  // (a group per tuple of the marked ranges); beyond a quarter of a gigabyte of such slack the pass is waited for first
  uint64_t row_bytes = 0;
  for (int i = 0; i < P.ngroup; ++i) row_bytes += vh_elem_size(P.g[i].type());
  for (int j = 0; j < P.nmetric; ++j) row_bytes += vh_elem_size(r->metric_elem[j]);
  const bool overlap = heavy_wanted && plan && !one_shot && !r->hp_chunks && hc[12] * row_bytes <= (256ull << 20) && !test_env("VH_NO_HEAVY_OVERLAP");
  if (heavy_wanted && plan && !overlap) heavy_pass_launch(r, plan, hc[11], hc[12], hc[13], HR);
  auto heavy_join = [&]() -> bool {             // false: no second pass to be had — the plain table for everything, as before
    heavy_pass_finish(r, HR);
    if (!HR.r2 || (one_shot && ng + HR.r2->ngroups_host > r->out_cap)) { delete HR.r2; HR.r2 = nullptr; *retry = 4; r->plan.hp_passes = 64; return false; }
    heavy.reset(HR.r2);
    n2 = HR.r2->ngroups_host;
    r->info.retries += 1;       // (counted like an attempt: the caller sees that the query took more than one pass)
    if (r->kernel.find(HR.r2->kernel) == std::string::npos) r->kernel += " + " + HR.r2->kernel;      // (vh_result_kernel: what the second pass ran)
    return true;
  };
  auto append_heavy = [&](const size_t* key_off, const size_t* state_off) {      // the second pass's rows behind row ng of this result's host columns
    char* H = x->h_out[slot];
    for (int i = 0; i < P.ngroup; ++i) { const size_t es = vh_elem_size(P.g[i].type()); memcpy(H + key_off[i] + ng * es, heavy->h_base + heavy->off_key[i], n2 * es); }
    for (int j = 0; j < P.nmetric; ++j) { const size_t es = vh_elem_size(r->metric_elem[j]); memcpy(H + state_off[j] + ng * es, heavy->h_base + heavy->off_state[j], n2 * es); }
  };
  if (!one_shot) {
    if (!r->hp_chunks) {           // a big result in one piece: the staging buffer is sized for the rows there are
      if (heavy_wanted && !overlap) { if (!heavy_join()) return VH_OK; }
      L = packed_for(ng + (overlap ? hc[12] : n2));
      if (int src = stage(L.bytes)) return src;
      // (the pass is enqueued BEFORE the copy's kernel: its clears and its scan are under way when the 64 blocks that push rows over PCIe start)
      const auto h0 = std::chrono::steady_clock::now();
      if (overlap) heavy_pass_launch(r, plan, hc[11], hc[12], hc[13], HR);
      if (ng) { if (int crc = copy_rows(L, 0, 0, ng, r->topk_active, st)) return crc; }
      HIP_TRY(hipEventRecord(x->ev[3], st));
      if (overlap) {
        const bool joined = heavy_join();
        const auto h1 = std::chrono::steady_clock::now();
        if (!joined) { (void)wait_event_spinning(x->ev[3]); return VH_OK; }
        HIP_TRY(wait_event_spinning(x->ev[3]));
        if (knobs().times) {
          const auto ms = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count() / 1e3; };
          fprintf(stderr, "vh heavy pass: done %.3f ms after its launch, the copy of the first pass's rows %.3f ms after that (ranges %llu, tuples <= %llu, rows %llu)\n", ms(h0, h1),
                  ms(h1, std::chrono::steady_clock::now()), hc[11], hc[12], (unsigned long long)n2);
        }
      }
      HIP_TRY(wait_event_spinning(x->ev[3]));
      if (n2) append_heavy(L.key, L.state);
    } else if (heavy_wanted) { if (!heavy_join()) return VH_OK; }
    memcpy(x->h_out[slot], head, 512);
    for (int i = 0; i < P.ngroup; ++i) r->off_key[i] = L.key[i];      // (the host view: where vh_result_view finds the columns)
    for (int j = 0; j < P.nmetric; ++j) r->off_state[j] = L.state[j];
  } else if (heavy_wanted) {
    if (!heavy_join()) return VH_OK;
    if (n2) append_heavy(r->off_key, r->off_state);
  }
  if (n2) { ng += n2; r->info.ngroups += n2; r->info.returned_groups = ng; r->ngroups_host = ng; }
  heavy.reset();
  r->h_base = x->h_out[slot];
  float ms = 0;
  (void)hipEventElapsedTime(&ms, x->ev[1], x->ev[2]); r->info.scan_kernel_ms = ms;
  (void)hipEventElapsedTime(&ms, x->ev[0], x->ev[3]); r->info.total_ms = ms;
  if (knobs().times) {   // where a query's device time goes: setup (clears, uploads) | scan | emission + read-back
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, x->ev[0], x->ev[1]); (void)hipEventElapsedTime(&b, x->ev[2], x->ev[3]);
    fprintf(stderr, "vh times: setup %.3f ms, scan %.3f ms, emit+readback %.3f ms (groups %llu, returned %llu)\n", a, r->info.scan_kernel_ms, b,
            (unsigned long long)r->info.ngroups, (unsigned long long)r->info.returned_groups);
  }
  r->finalized = true;
  return VH_OK;
}


extern "C" int vh_query_launch(vh_table* t, const vh_plan* plan, vh_result** out) {
  if (!t || !plan || !out) return vh_fail(VH_E_INVALID, "null argument");
  VH_ENTER();
  VhExec* x = nullptr;
  if (int rc = exec_acquire(t, &x)) return rc;
  vh_result* r = nullptr;
  int rc;
  { std::lock_guard<std::mutex> lk(t->mu); rc = query_launch_locked(t, x, plan, &r); }
  if (rc) { (void)hipStreamSynchronize(x->stream()); exec_release(t, x); return rc; }
  r->exec = x;
  *out = r;
  return VH_OK;
}

extern "C" int vh_result_finalize(vh_result* r) {
  if (!r) return vh_fail(VH_E_INVALID, "null result");
  if (r->finalized) return VH_OK;
  VH_ENTER();
  int retry = 0;
  int rc = result_finalize(r, &retry);
  if (rc) return rc;
  if (retry) return vh_fail(VH_E_RANGE, "partial result needs a re-plan (code %d); use vh_query_agg", retry);
  return VH_OK;
}

// One attempt's verdict -> the overrides of the next one (VhReplan, vhh_plan.h). Shared by vh_query_agg and the sharded form.
static void replan_after(vh_table* t, vh_result* r, int retry, VhReplan* rp) {
  if (retry == 1) {
    // table too small. The number of groups is bounded by the number of surviving rows: estimate those
    // once with the selectivity probe and size for them, instead of quadrupling blindly
    uint64_t next = (r->plan.hmask + 1) * 4;
    if (!rp->cap_override) {
      double sel = 1.0;
      if (r->fast_scan) { std::lock_guard<std::mutex> lk(t->mu); (void)estimate_selectivity(t, r->exec, r->plan, r->h_prog, r->h_lits, r->plan.nseg, &sel, nullptr, nullptr, !r->h_sets.empty(), &r->h_sets); }      // (set leaves: the interpreting kernel counts)
      uint64_t survivors = (uint64_t)((double)r->info.scanned_recs * std::min(1.0, sel * 1.1)) + 1024;
      uint64_t sized = 1;
      while (sized < survivors * 2) sized <<= 1;
      next = std::max(next, sized);
    }
    rp->cap_override = next;
  }
  else if (retry == 6) { if (r->hpart) rp->no_hpart = true; else rp->no_part = true; }      // a value beyond its column's recorded range in a packed tuple
  else if (retry == 4) {                                     // hashed partitioning: a range held more groups (or ids) than its passes' LDS tables take
    // ... skewed beyond help (a group with more ids than any number of passes fits into a range's LDS set): the plain hash table — and the table
    // remembers the shape, like groups_seen for hash sizing: its next queries start there instead of paying for the void attempts every time
    if (r->plan.hp_passes >= 64) { rp->no_hpart = true; std::lock_guard<std::mutex> lk(t->mu); t->hpart_hopeless.insert(r->group_sig); }
    else rp->hp_passes = (uint32_t)r->plan.hp_passes * 4;
    if (rp->hp_passes > 64) rp->hp_passes = 64;
  }
  else if (retry == 3 && r->hpart) {                         // hashed partitioning ran out of tuple extents: size for the survivors it counted, then give up
    // (the ring writer's pools hold any skew between their streams — positional extents + a shared overflow region as big as the estimate —, so
    // running out means more survivors than estimated: the re-run is sized for what this attempt counted, through the same writer)
    if (rp->part_override) rp->no_hpart = true;
    else rp->part_override = std::max<uint64_t>(r->info.passed_recs + r->info.passed_recs / 16 + 1024, 1ull << 16);
  }
  else if (retry == 3) {                                     // tuple extents exhausted: more room, then give up on partitioning
    // the attempt counted its survivors even though it dropped their tuples: the next one is sized for exactly that many
    const uint64_t had = (uint64_t)r->plan.max_extents * r->plan.ext_tuples;
    // the piecewise writers' positional chunks (VhPlanDev::ext_waves: tuples of three or more words, the pre-built kernels) ran out with room to
    // spare: some waves met far more survivors than others. Remembered for the shape, like groups_seen for hash sizing: its next queries start on the
    // shared cursor. (The ring writer needs no such memory: its streams overflow into the pool's shared region inside the kernel.)
    if (r->plan.ext_waves && r->info.passed_recs + r->info.passed_recs / 16 <= had) { std::lock_guard<std::mutex> lk(t->mu); t->part_clustered.insert(r->group_sig); }
    if (rp->part_override && had >= r->info.scanned_recs) rp->no_part = true;
    else rp->part_override = std::max<uint64_t>(std::max<uint64_t>(rp->part_override * 2, r->info.passed_recs + r->info.passed_recs / 16), 1ull << 16);
  }
  else rp->force_hash = true;                                // a digit left its planned range
}

// More metrics than one pass carries (VH_MAX_METRIC states per group in the kernel arguments): several passes over
// the same snapshot, each with a slice of the metrics, joined on the group key. The reference has no such limit
// (AggTuple::Metrics is a generated struct of any width, store.cc:31-169).
static int query_agg_multipass(vh_table* t, const vh_plan* plan, vh_result** out) {
  if (plan->nhaving || plan->top_k)
    return vh_fail(VH_E_UNSUPPORTED, "%d metrics take several passes: apply HAVING / top-N to the returned groups", plan->nmetrics);
  const int per = VH_MAX_METRIC - 4;
  std::vector<std::unique_ptr<vh_result>> parts;
  int count_col = -1;
  for (int j = 0; j < plan->nmetrics; ++j)
    if (plan->metrics[j] >= 0 && (size_t)plan->metrics[j] < t->cols.size() && t->cols[plan->metrics[j]].kind == VH_METRIC_COUNT) count_col = plan->metrics[j];
  std::vector<int> part_user;                                  // metrics of each pass that belong to the caller's list
  for (int off = 0; off < plan->nmetrics; off += per) {
    const int nm = std::min(per, plan->nmetrics - off);
    std::vector<int32_t> cm(plan->metrics + off, plan->metrics + off + nm);
    bool avg = false, cnt = false;
    for (int32_t c : cm) if (c >= 0 && (size_t)c < t->cols.size()) { avg |= t->cols[c].kind == VH_METRIC_AVG; cnt |= t->cols[c].kind == VH_METRIC_COUNT; }
    if (avg && !cnt && count_col >= 0) cm.push_back(count_col);   // an AVG slice still divides by the query's COUNT (scan.cc:239-241): it rides along
    vh_plan cp = *plan;
    cp.metrics = cm.data(); cp.nmetrics = (int32_t)cm.size();
    vh_result* r = nullptr;
    if (int rc = vh_query_agg(t, &cp, &r)) return rc;
    parts.emplace_back(r);
    part_user.push_back(nm);
  }
  vh_result* base = parts[0].get();
  const uint64_t n = base->ngroups_host;
  const int nk = base->plan.ngroup;
  std::unique_ptr<vh_result> rf(new vh_result());
  rf->table = t; rf->info = base->info; rf->mode = base->mode; rf->kernel = base->kernel;
  rf->plan.ngroup = nk; rf->plan.key_words = base->plan.key_words;
  for (int i = 0; i < nk; ++i) rf->plan.g[i] = base->plan.g[i];
  rf->group_elem = base->group_elem;
  auto key_of = [&](const vh_result* r, uint64_t row) {
    std::string k;
    for (int i = 0; i < nk; ++i) { const int es = vh_elem_size(r->plan.g[i].type()); k.append(r->h_base + r->off_key[i] + row * es, es); }
    return k;
  };
  std::unordered_map<std::string, uint64_t> where;
  if (parts.size() > 1) { where.reserve(n * 2); for (uint64_t row = 0; row < n; ++row) where.emplace(key_of(base, row), row); }
  // layout of the joined result: keys, then every pass's user metrics in plan order, then the hidden count (if the plan has one)
  const vh_result* hidden_from = nullptr;
  bool any_count = false;
  for (int j = 0; j < plan->nmetrics; ++j) any_count |= plan->metrics[j] >= 0 && t->cols[plan->metrics[j]].kind == VH_METRIC_COUNT;
  for (auto& pr : parts) if (pr->info.has_hidden_count && !any_count && !hidden_from) hidden_from = pr.get();
  size_t bytes = 0;
  for (int i = 0; i < nk; ++i) { rf->off_key[i] = bytes; bytes += (std::max<uint64_t>(n, 1) * vh_elem_size(base->plan.g[i].type()) + 255) / 256 * 256; }
  std::vector<std::pair<const vh_result*, int>> src;      // joined device-metric index -> (pass, its device metric)
  for (size_t k = 0; k < parts.size(); ++k) for (int j = 0; j < part_user[k]; ++j) src.push_back({parts[k].get(), parts[k]->user_metric[j]});
  if (hidden_from) src.push_back({hidden_from, hidden_from->plan.nmetric - 1});
  if (src.size() > 4096) return vh_fail(VH_E_UNSUPPORTED, "too many metrics");
  std::vector<size_t> off_state(src.size());
  for (size_t u = 0; u < src.size(); ++u) {
    rf->metric_elem.push_back(src[u].first->metric_elem[src[u].second]);
    off_state[u] = bytes; bytes += (std::max<uint64_t>(n, 1) * vh_elem_size(rf->metric_elem.back()) + 255) / 256 * 256;
  }
  HIP_TRY(host_alloc_near_device((void**)&rf->h_own, bytes, hipHostMallocDefault));
  for (int i = 0; i < nk; ++i) if (n) memcpy(rf->h_own + rf->off_key[i], base->h_base + base->off_key[i], n * vh_elem_size(base->plan.g[i].type()));
  for (size_t u = 0; u < src.size(); ++u) {
    const vh_result* pr = src[u].first;
    const int es = vh_elem_size(rf->metric_elem[u]);
    const char* from = pr->h_base + pr->off_state[src[u].second];
    char* to = rf->h_own + off_state[u];
    if (pr == base) { if (n) memcpy(to, from, n * es); continue; }
    if (pr->ngroups_host != n) return vh_fail(VH_E_DEVICE, "passes of one query returned %llu and %llu groups", (unsigned long long)n, (unsigned long long)pr->ngroups_host);
    for (uint64_t row = 0; row < n; ++row) {
      auto it = where.find(key_of(pr, row));
      if (it == where.end()) return vh_fail(VH_E_DEVICE, "passes of one query returned different groups");
      memcpy(to + it->second * es, from + row * es, es);
    }
  }
  rf->wide_off_state = off_state;
  for (int j = 0; j < plan->nmetrics; ++j) rf->user_metric.push_back(j);
  rf->info.nmetrics = plan->nmetrics; rf->info.has_hidden_count = hidden_from ? 1 : 0;
  rf->plan.nmetric = (int32_t)std::min<size_t>(src.size(), VH_MAX_METRIC);
  rf->h_base = rf->h_own; rf->ngroups_host = n; rf->finalized = true;
  *out = rf.release();
  return VH_OK;
}

static int place_layouts(vh_table* t, const vh_plan* plan, vh_result_info* info_out, double budget_ms);
static bool placing_now();
// The attempts of ONE query on context x: plan and launch, finalise, and where the verdict asks for it plan again (replan_after). It takes the
// context over: the result owns it, or it is released. `first`: an attempt that is launched already and not finalised yet — a member of a
// batch, whose re-plan is this loop too — in place of the first plan.
static int query_agg_attempts(vh_table* t, VhExec* x, const vh_plan* plan, vh_result** out, vh_result* first = nullptr) {
  VhReplan rp;
  int rc = VH_OK;
  for (uint32_t attempt = 0; attempt < 12; ++attempt) {
    vh_result* r = attempt == 0 ? first : nullptr;
    const auto h0 = std::chrono::steady_clock::now();
    // planned and launched under the table lock; the wait for the device and the read-back happen outside it, so
    // queries of other threads on this table run meanwhile (each on its own context)
    if (!r) {
      std::lock_guard<std::mutex> lk(t->mu);
      g_heavy.allow_mark = true;        // (this caller can run the second pass over heavy ranges: it holds the plan when the verdict is in)
      VhLaunchOpts o;
      o.rp = rp;
      rc = query_launch_locked(t, x, plan, &r, o);
      g_heavy = VhHeavyCtx{};
    }
    if (rc) break;
    r->exec = x;
    int retry = 0;
    const auto h1 = std::chrono::steady_clock::now();
    rc = result_finalize(r, &retry, plan);
    if (knobs().times) fprintf(stderr, "vh host: plan + enqueue %.1f us, finalize (enqueue tail + wait + read-back) %.1f us\n", std::chrono::duration<double, std::micro>(h1 - h0).count(),
                               std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h1).count());
    if (rc) { r->exec = nullptr; delete r; break; }
    if (!retry) {
      r->info.retries += attempt;                              // (+ 1 where a second pass took the heavy ranges of a hashed partitioning)
      r->stream_quiet = true;                                  // (result_finalize waited for everything it enqueued)
      if (r->mode == VH_MODE_HASH) { std::lock_guard<std::mutex> lk(t->mu); t->groups_seen[r->group_sig] = r->info.ngroups; }
      *out = r;
      return VH_OK;
    }
    replan_after(t, r, retry, &rp);
    r->exec = nullptr;                                       // the next attempt runs on the same context
    delete r;
    rc = vh_fail(VH_E_NOMEM, "aggregate table kept overflowing");
  }
  (void)hipStreamSynchronize(x->stream());
  exec_release(t, x);
  return rc;
}

extern "C" int vh_query_agg(vh_table* t, const vh_plan* plan, vh_result** out) {
  if (!t || !plan || !out) return vh_fail(VH_E_INVALID, "null argument");
  VH_ENTER();
  if (plan->nmetrics > VH_MAX_METRIC - 1 && plan->metrics) return query_agg_multipass(t, plan, out);
  VhExec* x = nullptr;
  if (int rc = exec_acquire(t, &x, !placing_now())) return rc;      // (a placement's own queries never wait for a context: its caller may hold the last one — no placement then)
  return query_agg_attempts(t, x, plan, out);
}

// ------------------------------------------------------------------ a batch of aggregates (include/viya_hip.h, vh_query_agg_batch)
// The scans the members' plans handed over (QueryBuild::launch), enqueued: vh_batch.h forms the groups; a group's members are answered by ONE
// launch of scan_agg_planes_batch_kernel on the stream of its first member, the lead; a candidate that stays alone gets the launch its plan
// would have made. Behind either, each member's own tail on its own stream (query_scan_tail). t->mu is held, and so is the batch's tick.
// Within a group, vh_batch_share (vh_batch.h) says which members take an earlier member's pass mask (VhBatchMember::mask_of); no_share: every
// member evaluates its own (VH_TEST_NO_BATCH_SHARE).
// COMPILED candidates (vh_batch.h; members that asked for the compiled plane aggregate and have their own kernel) form groups of their own. Such
// a group is answered by the kernel compiled for its BATCH SHAPE (batch_kernel below): the members' shapes in launch order, the mask_of
// vector — vh_batch_share's with one more condition, equal filter member-shapes — and the scope. While that kernel is pending, and where it
// failed or the generator has no shape for the group, the group is dissolved before anything is launched: each member is launched by its own
// compiled kernel, the single compiled query it would have been (never an error, VH_PLAN_FORCE_JIT or not).
static_assert(VH_SHARE_KIND_REL == VH_F_REL && VH_SHARE_KIND_IN == VH_F_IN && VH_SHARE_KIND_INSET == VH_F_INSET, "vh_batch.h restates enum vh_fkind");
static_assert(sizeof(VhBitsOp) == 8 && offsetof(VhBitsOp, w0) == 0 && offsetof(VhBitsOp, w1) == 4, "vh_batch.h reads an op as two words");
struct VhBatchGroups { uint32_t n = 0, compiled = 0; int32_t of[VH_BATCH_MAX]; uint32_t lead[VH_BATCH_MAX]; };
// The kernel of a compiled group's batch shape, by the single shape's paths (compile_plane_agg): inline mode compiles here and counts it in
// inline_builds, background mode asks the worker. nullptr: *pending says whether the worker has it; else `why` holds the reason.
static VhJitKernel* batch_kernel(vh_table* t, const VhJitShape& js, bool* pending, std::string* why) {
  *pending = false;
  if (!vh_jit_batch_ok(js)) { *why = "the generator has no shape for this group"; return nullptr; }
  VhJitKernel* k = nullptr;
  if (build_background(t)) {
    if (vh_jit_peek(js, &k, why) == 0) *pending = build_request_kernel(t, js);
    if (!*pending && !k && why->empty()) *why = "the build worker is shutting down";
    if (*pending) *why = "the batch kernel is being compiled";
  } else {
    VhJitKernel* had = nullptr;
    std::string ignored;
    const bool known = vh_jit_peek(js, &had, &ignored) != 0;
    k = vh_jit_get(js, why);
    if (!known) ++t->inline_builds;
  }
  return k;
}
static int batch_launch_scans(vh_table* t, VhBatchFuse& F, uint32_t n, VhBatchGroups* G, uint32_t* failed, bool no_share) {
  VhFuseDesc d[VH_BATCH_MAX] = {};
  VhShareDesc sh[VH_BATCH_MAX] = {};
  std::string fshape[VH_BATCH_MAX];
  for (uint32_t i = 0; i < n; ++i) {
    const VhDeferredScan& s = F.scan[i];
    if (!s.r) continue;
    d[i].candidate = 1; d[i].scope = s.xcd_private ? 1u : 0u; d[i].v_serial = s.v_serial; d[i].nseg = (uint32_t)s.P.nseg; d[i].chunks_per_seg = s.chunks_per_seg;
    d[i].lds_bytes = (uint32_t)((s.lds_table + 15) / 16 * 16);
    d[i].compiled = s.pagg_jk ? 1u : 0u;
    VhShareDesc& h = sh[i];
    h.has_filter = s.D.has_filter; h.f_serial = s.f_serial;
    h.f_planes = (uint64_t)(uintptr_t)s.A.F.planes; h.f_stride = s.A.F.stride; h.f_pitch = s.A.F.pitch;
    h.nprog = s.B.nprog; h.flat = s.B.flat; h.ops = &s.B.op[0].w0; h.lits = s.B.lits; h.nlits = VH_BITS_MAX_LITS;
    h.nseg = (uint32_t)s.P.nseg; h.seg_rows = s.segrows;
    if (s.pagg_jk) {      // (equal filter member-shapes, equal numbers: the first such member's position + 1)
      fshape[i] = vh_jit_filter_key(s.js);
      h.filter_shape = i + 1;
      for (uint32_t j = 0; j < i; ++j) if (F.scan[j].r && F.scan[j].pagg_jk && fshape[j] == fshape[i]) { h.filter_shape = j + 1; break; }
    }
  }
  G->n = vh_batch_group(d, n, G->of);
  // the compiled groups' kernels first: a group whose batch kernel is not at hand is no group (its members: their own compiled kernels)
  VhJitKernel* bk[VH_BATCH_MAX] = {};
  uint32_t share_of[VH_BATCH_MAX][VH_BATCH_MAX], share_classes[VH_BATCH_MAX] = {};
  {
    uint32_t kept = 0;
    bool pend[VH_BATCH_MAX] = {};
    for (uint32_t g = 0; g < G->n; ++g) {
      uint32_t m[VH_BATCH_MAX], cnt = 0;
      for (uint32_t i = 0; i < n; ++i) if (G->of[i] == (int32_t)g) m[cnt++] = i;
      uint32_t mask_of[VH_BATCH_MAX], classes = cnt;
      if (no_share) for (uint32_t k = 0; k < cnt; ++k) mask_of[k] = k;
      else classes = vh_batch_share(sh, m, cnt, mask_of);
      VhJitKernel* k = nullptr;
      bool dissolve = false;
      if (d[m[0]].compiled) {
        VhJitShape js;
        js.mode = VH_MODE_DENSE_LDS; js.block = 256;
        js.scope = F.scan[m[0]].js.scope; js.xcd = F.scan[m[0]].js.xcd;      // (part of the fuse key: the same for every member)
        for (uint32_t q = 0; q < cnt; ++q) { js.members.push_back(F.scan[m[q]].js); js.mask_of.push_back((int)mask_of[q]); }
        bool pending = false;
        std::string why;
        *failed = m[0];
        k = batch_kernel(t, js, &pending, &why);
        if (!k) {
          if (knobs().jit_verbose) fprintf(stderr, "vh: no compiled fused launch for %u members, each runs its own compiled kernel: %s\n", cnt, why.c_str());
          dissolve = true;
          for (uint32_t q = 0; q < cnt; ++q) { G->of[m[q]] = -1; pend[m[q]] = pending; }
        }
      }
      if (dissolve) continue;
      for (uint32_t q = 0; q < cnt; ++q) { G->of[m[q]] = (int32_t)kept; share_of[kept][q] = mask_of[q]; }
      share_classes[kept] = classes; bk[kept] = k;
      if (k) ++G->compiled;
      ++kept;
    }
    G->n = kept;
    for (uint32_t i = 0; i < n; ++i) if (pend[i]) F.scan[i].r->info.reserved |= VH_INFO_BUILD_PENDING;
  }
  for (uint32_t i = 0; i < n; ++i) {      // alone after all: the single query's launch
    const VhDeferredScan& s = F.scan[i];
    if (!s.r || G->of[i] >= 0) continue;
    *failed = i;
    VhScanLaunch L;
    L.grid = s.grid; L.lds = s.lds_table; L.stream = s.x->stream();
    if (s.pagg_jk) HIP_TRY(vh_jit_launch_planes(s.pagg_jk, s.P, s.A.D, s.chunks_per_seg, s.grid, 256, s.lds_table, L.stream));      // (scan_dispatch's launch of the single compiled query)
    else vh_launch_scan_planes(s.P, s.A, s.chunks_per_seg, L, s.xcd_private);
    if (int rc = query_scan_tail(s.r, s.x)) return rc;
  }
  for (uint32_t g = 0; g < G->n; ++g) {
    uint32_t m[VH_BATCH_MAX], cnt = 0;
    for (uint32_t i = 0; i < n; ++i) if (G->of[i] == (int32_t)g) m[cnt++] = i;
    const VhDeferredScan& lead = F.scan[m[0]];
    G->lead[g] = m[0]; *failed = m[0];
    VhExec* lx = lead.x;
    if (int rc = exec_batch(lx)) return rc;
    hipStream_t ls = lx->stream();
    uint32_t lds = 0;
    int grid = 0;
    bool rows = false;      // any row member: the instantiation that carries the row sink
    const uint32_t* mask_of = share_of[g];
    const uint32_t classes = share_classes[g];
    for (uint32_t k = 0; k < cnt; ++k) {      // the lead's stream behind every member's clears and uploads; the members' array, staged
      const VhDeferredScan& s = F.scan[m[k]];
      if (s.x->stream() != ls) HIP_TRY(hipStreamWaitEvent(ls, s.x->ev[1], 0));
      VhBatchMember& M = lx->h_batch[k];
      M.P = s.P; M.B = s.B; M.D = s.D; M.F = s.A.F; M.lds_base = lds; M.mask_of = mask_of[k];
      lds += d[m[k]].lds_bytes;
      grid = std::max(grid, s.grid);
      rows = rows || s.D.rows != 0;
    }
    HIP_TRY(hipMemcpyAsync(lx->d_batch, lx->h_batch, cnt * sizeof(VhBatchMember), hipMemcpyHostToDevice, ls));
    HIP_TRY(hipEventRecord(lx->ev_batch[0], ls));
    char nm[160] = "";
    if (bk[g]) {      // a compiled group: the kernel of its batch shape (the row sink's queue is static LDS of a text with a row member)
      snprintf(nm, sizeof(nm), "%s", bk[g]->name.c_str());
      HIP_TRY(vh_jit_launch_planes_batch(bk[g], lx->d_batch, lead.chunks_per_seg, grid, 256, lds, ls));
    } else {
      VhScanLaunch L;
      L.name = nm; L.name_cap = sizeof(nm);
      vh_launch_scan_planes_batch(lx->d_batch, cnt, lead.A.V, lead.chunks_per_seg, L, lead.xcd_private, rows);      // (its name)
      L = VhScanLaunch{};
      L.grid = grid; L.lds = lds; L.stream = ls;
      vh_launch_scan_planes_batch(lx->d_batch, cnt, lead.A.V, lead.chunks_per_seg, L, lead.xcd_private, rows);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(lx->ev_batch[1], ls));
    for (uint32_t k = 0; k < cnt; ++k) {      // every member's stream behind the launch, then its own tail there
      const VhDeferredScan& s = F.scan[m[k]];
      *failed = m[k];
      if (s.x->stream() != ls) HIP_TRY(hipStreamWaitEvent(s.x->stream(), lx->ev_batch[1], 0));
      s.r->kernel = nm;
      s.r->info.reserved |= VH_INFO_BATCH_FUSED;
      s.r->batch_member = vh_batch_member_info{1u, g, k, cnt, mask_of[k], classes};
      if (int rc = query_scan_tail(s.r, s.x)) return rc;
    }
  }
  return VH_OK;
}

extern "C" int vh_query_agg_batch(vh_table* t, const vh_plan* const* plans, uint32_t n, vh_result** out, vh_batch_info* info) {
  if (info) *info = vh_batch_info{};
  if (!t) return vh_fail(VH_E_INVALID, "null argument");
  if (n > VH_BATCH_MAX) return vh_fail(VH_E_INVALID, "a batch of %u plans (max %d)", n, VH_BATCH_MAX);
  if (n == 0) return VH_OK;
  if (!plans || !out) return vh_fail(VH_E_INVALID, "null argument");
  for (uint32_t i = 0; i < n; ++i) out[i] = nullptr;
  for (uint32_t i = 0; i < n; ++i) if (!plans[i]) return vh_fail(VH_E_INVALID, "plan %u: null plan", i);
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  VH_ENTER();
  const char* const nf = test_env("VH_TEST_NO_BATCH_FUSE");      // tests, probe: every member answered singly (an A/B inside one process)
  const bool no_fuse = nf && atoi(nf) != 0;
  const char* const ns = test_env("VH_TEST_NO_BATCH_SHARE");     // tests, probe: every fused member evaluates its own pass mask (the fused launch without sharing)
  const bool no_share = ns && atoi(ns) != 0;
  VhExec* xs[VH_BATCH_MAX] = {};          // a member's context while no result owns it
  vh_result* rs[VH_BATCH_MAX] = {};       // a member's launched attempt (it owns the context)
  bool wide[VH_BATCH_MAX] = {};           // more metrics than one pass carries: vh_query_agg's passes, behind the others
  auto fail = [&](int rc, uint32_t i) {   // all or nothing
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s", g_err);
    for (uint32_t k = 0; k < n; ++k) {
      if (out[k]) { delete out[k]; out[k] = nullptr; }
      if (rs[k]) { delete rs[k]; rs[k] = nullptr; }
      else if (xs[k]) { (void)hipStreamSynchronize(xs[k]->stream()); exec_release(t, xs[k]); }
      xs[k] = nullptr;
    }
    (void)hipGetLastError();
    return vh_fail(rc, "plan %u: %.480s", i, msg);
  };
  for (uint32_t i = 0; i < n; ++i) {
    wide[i] = plans[i]->nmetrics > VH_MAX_METRIC - 1 && plans[i]->metrics;
    if (wide[i]) continue;
    if (int rc = exec_acquire(t, &xs[i], !placing_now())) { xs[i] = nullptr; return fail(rc, i); }
  }
  std::unique_ptr<VhBatchFuse> fuse(new VhBatchFuse());
  VhBatchGroups G;
  for (uint32_t i = 0; i < n; ++i) G.of[i] = -1;
  int rc = VH_OK;
  uint32_t failed = 0;
  bool evicted = false;
  {
    // every member planned and enqueued within ONE hold of the lock — one state of the table — and under ONE tick (PlanTick, vhh_launch.h):
    // it ends, and trims a layout budget, behind the last fused launch and before the lock is released
    std::lock_guard<std::mutex> lk(t->mu);
    {
      PlanTick tick(t, nullptr, false);
      for (uint32_t i = 0; i < n && !rc; ++i) {
        if (wide[i]) continue;
        failed = i;
        fuse->member = i;
        g_heavy.allow_mark = true;
        VhLaunchOpts o;
        o.fuse = no_fuse ? nullptr : fuse.get();
        rc = query_launch_locked(t, xs[i], plans[i], &rs[i], o);
        g_heavy = VhHeavyCtx{};
        if (rc) { rs[i] = nullptr; break; }
        rs[i]->exec = xs[i];
      }
      if (!rc) rc = batch_launch_scans(t, *fuse, n, &G, &failed, no_share);
    }
    evicted = t->layout_budget != 0 && g_plan_evicted;
  }
  if (rc) return fail(rc, failed);
  // outside the lock: every member's wait and read-back, and its re-plan where the verdict asks for one, by vh_query_agg's own loop
  for (uint32_t i = 0; i < n; ++i) {
    if (wide[i]) rc = query_agg_multipass(t, plans[i], &out[i]);
    else {
      vh_result* r = rs[i];
      rs[i] = nullptr; xs[i] = nullptr;      // (the loop takes context and attempt over)
      rc = query_agg_attempts(t, r->exec, plans[i], &out[i], r);
    }
    if (rc) { out[i] = nullptr; return fail(rc, i); }
  }
  vh_batch_info bi{};
  bi.nplans = n; bi.fused_groups = G.n;
  for (uint32_t g = 0; g < G.n; ++g) {      // (every member's stream waited for the launch's end: the events have completed)
    float ms = 0;
    (void)hipEventElapsedTime(&ms, fuse->scan[G.lead[g]].x->ev_batch[0], fuse->scan[G.lead[g]].x->ev_batch[1]);
    bi.fused_kernel_ms += ms;
    for (uint32_t i = 0; i < n; ++i)
      if (G.of[i] == (int32_t)g && (out[i]->info.reserved & VH_INFO_BATCH_FUSED)) { out[i]->info.scan_kernel_ms = ms; ++bi.fused_members; }      // (a member that was planned again is a single query's result)
  }
  bi.singles = n - bi.fused_members;
  bi.reserved = G.compiled;      // (the compiled fused launches among fused_groups)
  if (evicted) for (uint32_t i = 0; i < n; ++i) out[i]->info.reserved |= VH_INFO_EVICTED;
  if (info) *info = bi;
  return VH_OK;
}

// A place for the derived layouts a plan reads (vhh_derived.h, derived_move): up to `prepare_place` other places tried, each measured with three
// queries, the fastest kept. Only where it can matter (a scan of 0.3 ms and more through a projection or predicate planes) and while the
// candidates fit the free device memory next to a quarter of the device. Called by vh_table_prepare only: doing the same from inside the first
// query that finds unprepared layouts in use was built and taken out again — its queries run on a second execution context while the caller's
// result holds the first (seconds of pinned staging memory behind a big result), and a fresh allocation of a few GB takes the driver 2 ms or
// 400 depending on what the memory was last used for: first queries of 3.4 s were seen. A setup call can afford that; a query cannot.
static thread_local bool g_placing = false;
static bool placing_now() { return g_placing; }
static int place_layouts(vh_table* t, const vh_plan* plan, vh_result_info* info_out, double budget_ms) {
  const auto t_begin = std::chrono::steady_clock::now();
  struct Guard { Guard() { g_placing = true; } ~Guard() { g_placing = false; } } guard;
  // test hooks (test_env): VH_TEST_PLACE_CANDIDATES=n tries exactly n places whatever the scan takes and however long they take (the free-memory
  // guard stays); VH_TEST_PLACE_VERDICT=keep|reject|alternate decides each candidate instead of its timing (noise on a small table);
  // VH_TEST_PLACE_WAIT_SYNC=1 holds every candidate, after its move and before its measuring queries, until a sync of another thread has landed
  // (outside t->mu): each window between derived_move and derived_settle then sees one — or the prepare fails, so no test passes without the race
  const char* env_cand = test_env("VH_TEST_PLACE_CANDIDATES");
  const char* env_verdict = test_env("VH_TEST_PLACE_VERDICT");
  const bool wait_sync = test_env("VH_TEST_PLACE_WAIT_SYNC") != nullptr;
  const bool forced = env_cand != nullptr;
  const int cand = forced ? std::max(0, atoi(env_cand)) : knobs().prepare_place;
  const int verdict = !env_verdict ? -1 : !strcmp(env_verdict, "keep") ? 1 : !strcmp(env_verdict, "reject") ? 0 : !strcmp(env_verdict, "alternate") ? 2 : -1;
  if (env_verdict && verdict < 0) return vh_fail(VH_E_INVALID, "VH_TEST_PLACE_VERDICT=%s: keep, reject or alternate", env_verdict);
  auto measure = [&](float* ms) -> int {
    *ms = 1e30f;
    for (int i = 0; i < 3; ++i) {
      vh_result* r = nullptr;
      if (int rc = vh_query_agg(t, plan, &r)) return rc;
      *ms = std::min(*ms, r->info.scan_kernel_ms);
      if (info_out) *info_out = r->info;
      vh_result_free(r);
    }
    return VH_OK;
  };
  if (cand > 0) {
    float best = 0;
    if (int rc = measure(&best)) return rc;
    std::vector<char*> held;
    for (int k = 0; k < cand && (forced || best >= 0.3f); ++k) {
      // (a fresh allocation of a few GB takes the driver 2 ms or 400, depending on what the memory was last used for: the candidates stop when the
      // budget is spent — a second inside vh_table_prepare, 0.3 s inside a query that places layouts nobody prepared)
      if (!forced && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() > budget_ms) break;
      std::vector<VhMoved> moved;
      // (both layouts, then the planes alone, then the projections alone, and again: what decides is how the two lie to each other as much as
      // where either lies; a spacer of 1-3 GB in front, because neighbouring allocations tend to behave alike)
      const uint32_t which = k % 3 == 0 ? 3u : k % 3 == 1 ? 2u : 1u;
      const auto tk0 = std::chrono::steady_clock::now();
      uint64_t moved_epoch = 0;
      {
        std::lock_guard<std::mutex> lk(t->mu);
        moved_epoch = t->sync_epoch;
        size_t free_b = 0, total_b = 0;
        const size_t spacer = (size_t)(1 + k % 3) << 30;
        if (!device_mem(&free_b, &total_b) || free_b < derived_bytes(t, which) + spacer + total_b / 4) break;
        char* sp = nullptr;
        if (hipMalloc(&sp, spacer) == hipSuccess) held.push_back(sp); else (void)hipGetLastError();
        if (int rc = derived_move(t, which, &moved)) { derived_settle(t, moved, false, &held); for (char* p : held) (void)hipFree(p); return rc; }
      }
      if (knobs().times) fprintf(stderr, "vh prepare: candidate %d: spacer + allocations + copies in %.1f ms\n", k, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0).count());
      if (moved.empty()) break;
      if (wait_sync) {
        const auto tw0 = std::chrono::steady_clock::now();
        for (;;) {
          { std::lock_guard<std::mutex> lk(t->mu); if (t->sync_epoch > moved_epoch) break; }
          if (std::chrono::steady_clock::now() - tw0 > std::chrono::seconds(10)) {
            { std::lock_guard<std::mutex> lk(t->mu); derived_settle(t, moved, false, &held); }
            for (char* p : held) (void)hipFree(p);
            return vh_fail(VH_E_INVALID, "vh_table_prepare: VH_TEST_PLACE_WAIT_SYNC: no sync landed within 10 s of candidate %d's move", k);
          }
          std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
      }
      float ms = 0;
      const auto tm0 = std::chrono::steady_clock::now();
      const int mrc = measure(&ms);
      if (knobs().times) fprintf(stderr, "vh prepare: candidate %d: three queries in %.1f ms\n", k, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count());
      const bool keep = !mrc && (verdict < 0 ? ms < best * 0.985f : verdict == 2 ? k % 2 == 0 : verdict == 1);
      if (knobs().times) fprintf(stderr, "vh prepare: %s at another place: %.4f ms against %.4f ms (%s)\n", which == 3u ? "projections and predicate planes" : which == 2u ? "predicate planes" : "projections", ms, best, keep ? "kept" : "given back");
      { std::lock_guard<std::mutex> lk(t->mu); derived_settle(t, moved, keep, &held); }
      if (mrc) { for (char* p : held) (void)hipFree(p); return mrc; }
      if (keep) best = ms;
    }
    if (!held.empty()) {
      const auto tf0 = std::chrono::steady_clock::now();
      std::lock_guard<std::mutex> lk(t->mu);
      table_quiesce(t);
      for (char* p : held) (void)hipFree(p);
      if (knobs().times) fprintf(stderr, "vh prepare: %zu buffers released in %.1f ms\n", held.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
    }
  }
  return VH_OK;
}

// First-use costs paid up front: the scan kernel compiled for the plan's shape (1-2 s of hipRTC, or milliseconds from the disk
// cache), the payload projection and the narrow predicate copies a selective query reads (built at once instead of after VH_AUTO_PACK /
// VH_AUTO_NARROW uses). (Rounds 3-5 also searched for a good place for a big tuple pool here; see vhh_place.h for why that is gone.) The reference's analogue is Compiler::Compile running when a
// query shape is first seen (src/codegen/compiler.cc:97-144, QueryStats::compile_time); a caller that knows its hot shapes at table-load
// time runs them through here. The plan is executed (up to three times: a narrow copy, then a projection can appear) and
// the last attempt's info is returned, so the caller sees what a steady-state query of this shape will run on.
static int table_prepare(vh_table* t, const vh_plan* plan, vh_result_info* info_out);
// What the prepared plan reads stays, whatever the budget: its queries pin every layout as they stamp it (layout_use, under the table lock, so no
// query of another thread evicts it between two rounds). When the prepare ends, the pins it made itself are taken back where it failed or
// where its last query no longer read the layout (a narrow copy a predicate projection replaced); what is unpinned then makes room.
extern "C" int vh_table_prepare(vh_table* t, const vh_plan* plan, vh_result_info* info_out) {
  if (!t || !plan) return vh_fail(VH_E_INVALID, "null argument");
  g_prepare_reads.clear(); g_prepare_pinned.clear();
  const int rc = table_prepare(t, plan, info_out);
  {
    std::lock_guard<std::mutex> lk(t->mu);
    VhLayoutRef v;
    for (uint64_t serial : g_prepare_pinned)
      if ((rc || std::find(g_prepare_reads.begin(), g_prepare_reads.end(), serial) == g_prepare_reads.end()) && layout_by_serial(t, serial, &v)) v.L->pinned = false;
    derived_trim(t, false);
  }
  g_prepare_reads.clear(); g_prepare_pinned.clear();
  return rc;
}
static int table_prepare(vh_table* t, const vh_plan* plan, vh_result_info* info_out) {
  (void)build_wait(t, 0, nullptr);      // (background build mode: a job of this table that is queued or running is joined, not duplicated)
  struct Guard { Guard() { g_preparing = true; } ~Guard() { g_preparing = false; } } guard;
  uint32_t last = ~0u;
  for (int round = 0; round < 3; ++round) {
    vh_result* r = nullptr;
    if (int rc = vh_query_agg(t, plan, &r)) return rc;
    const uint32_t now = r->info.reserved & ~(uint32_t)VH_INFO_EVICTED;      // (whether the round evicted something is no property of the plan)
    if (info_out) *info_out = r->info;
    vh_result_free(r);
    if (now == last) break;
    last = now;
  }
  return last & (VH_INFO_PACKED | VH_INFO_PREDPACK) ? place_layouts(t, plan, info_out, 1000.0) : VH_OK;
}

