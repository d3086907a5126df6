// viya_hip.hip — C-ABI implementation (include/viya_hip.h) over the gfx950 kernels.
//
// Host-side responsibilities that the reference performs inside the generated
// function and that therefore live on this side of the boundary:
//   * segment skipping from per-segment min/max (SegmentSkipBuilder,
//     src/codegen/query/filter.cc:263-335; use at src/codegen/query/scan.cc:48-51)
//   * stats.scanned_recs / scanned_segments / aggregated_recs bookkeeping
//     (scan.cc:44,51,246)
//   * choosing the aggregate-table organisation (the reference always uses
//     std::unordered_map, scan.cc:174-177; here: LDS-resident dense table, per-XCD
//     private dense tables in HBM/L2, or an open-addressing hash table in HBM).
#include "vh_small_kernels.h"
#include "vh_launch.h"
#include "vh_jit.h"
#include "vh_hpart.h"
#include "vh_batch.h"

#include <sched.h>
#include <algorithm>
#include <cctype>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

// ------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";
static int vh_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return vh_fail(e_ == hipErrorOutOfMemory ? VH_E_NOMEM : VH_E_DEVICE, "%s failed: %s (%s:%d)", \
                     #expr, hipGetErrorString(e_), __FILE__, __LINE__);                        \
  } while (0)

// ------------------------------------------------------------------ context
struct VhContext {
  bool inited = false;
  int device = 0;
  int num_cu = 256;
  int num_xcd = 8;
  size_t lds_per_block = 65536;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
};
static VhContext g_ctx;
static std::mutex g_mu;

// Every environment knob of the library, read ONCE (first use, normally vh_init) instead of wherever the planner happened to want
// one. They exist for measurements and tests: defaults are what every reported number was taken with (DESIGN.md "Knobs"). The
// VH_TEST_* / VH_POISON / VH_PART_TABLE_KB / VH_NO_HP_PACK / VH_NO_OFF32 hooks are the exception — tests switch them between two
// queries of one process — and go through test_env(): one gate (VH_TEST_HOOKS, read once; tests/conftest.py sets it) in front of them, so
// that a serving process never walks its environment on the query path. Among them: VH_TEST_PLACE_CANDIDATES / VH_TEST_PLACE_VERDICT /
// VH_TEST_PLACE_WAIT_SYNC make vh_table_prepare's placement of the derived layouts deterministic (vhh_finalize.h, place_layouts), and
// VH_TEST_JOURNAL_CAP replaces the 2^18 entries at which the table's journal drops its older half (vhh_table.h, table_note_change);
// VH_TEST_NO_BATCH_FUSE=1 makes vh_query_agg_batch answer every member singly, and VH_TEST_NO_BATCH_SHARE=1 keeps its fused launches but
// has every member evaluate its own pass mask (mask_of = its own position: the fused launch without sharing) — both read per call, the
// A/B of tools/batch_probe.py inside one process (vhh_finalize.h).
static const char* test_env(const char* name) {
  static const bool hooks = getenv("VH_TEST_HOOKS") != nullptr;
  return hooks ? getenv(name) : nullptr;
}
struct VhKnobs {
  bool trace_alloc, no_topk, jit_verbose, skip_phase2, no_direct_emit, times, no_jit_pagg, predpack_bytes, build_background, sliced_prebuilt, plane_agg, plane_jit;
  int max_exec, prepare_place, auto_narrow, auto_pack, jit_ablate, hp_ablate, hp_bpp, pack_plain, lanes_block, blocks_per_cu, unit_rows, grid, ext_tuples, ext_pad, bw_blocks_per_cu, hp_stream, hp_regions, hp_agg_waves, deliver_blocks;
  double hp_load_g, hp_load_s, qpay_min_sel;
  uint64_t layout_budget;
};
static const VhKnobs& knobs() {
  static const VhKnobs k = [] {
    auto flag = [](const char* n) { return getenv(n) != nullptr; };
    auto num = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
    auto real = [](const char* n, double dflt) { const char* e = getenv(n); return e ? atof(e) : dflt; };
    VhKnobs x{};
    x.trace_alloc = flag("VH_TRACE_ALLOC"); x.jit_verbose = flag("VH_JIT_VERBOSE"); x.times = flag("VH_TIMES");
    x.max_exec = std::max(1, num("VH_MAX_EXEC", 16));
    x.prepare_place = std::max(0, num("VH_PREPARE_PLACE", 8));      // other places vh_table_prepare tries for the derived layouts a plan reads (0: none)
    x.auto_narrow = num("VH_AUTO_NARROW", 3); x.auto_pack = num("VH_AUTO_PACK", 3);
    { const char* e = getenv("VH_BUILD"); x.build_background = e && !strcmp(e, "background"); }      // the build mode new tables start in (vh_table_set_build_mode; vhh_build.h)
    { const char* e = getenv("VH_LAYOUT_BUDGET"); x.layout_budget = e ? strtoull(e, nullptr, 10) : 0; }      // bytes the derived layouts of a new table may hold (0: no budget; vh_table_set_layout_budget, vhh_derived.h)
    { const char* e = getenv("VH_SLICED_PREBUILT"); x.sliced_prebuilt = e && atoi(e) != 0; }      // every aggregate plan of the process carries VH_PLAN_SLICED_PREBUILT (opt-in: profiles/r14/NOTES.md)
    { const char* e = getenv("VH_PLANE_AGG"); x.plane_agg = e && atoi(e) != 0; }      // ... VH_PLAN2_PLANE_AGG (opt-in: profiles/r15/NOTES.md)
    { const char* e = getenv("VH_PLANE_JIT"); x.plane_jit = e && atoi(e) != 0; }      // ... VH_PLAN2_PLANE_JIT (opt-in: profiles/r21/NOTES.md)
    x.hp_stream = num("VH_HP_STREAM", 0);             // chunk launches of a streamed result (0: off — measured: the link, not the wait for the kernels, bounds the delivery; profiles/r04/NOTES.md)
    x.qpay_min_sel = real("VH_QPAY_MIN_SEL", 0.15);        // selectivity from which the compiled scan streams 4-byte payload records instead of gathering them (measured: profiles/r05/NOTES.md)
    // What rounds 2-5 could switch from the environment for a measurement and round 6 fixed at the measured value (the notes of the round that
    // measured it say why; an A/B now means a line changed here and a rebuild): VH_NO_TOPK, VH_ABLATE_NO_PHASE2, VH_NO_DIRECT_EMIT, VH_NO_JIT_PAGG,
    // VH_PREDPACK_BYTES, VH_JIT_ABLATE, VH_HP_ABLATE, VH_HP_BPP, VH_PACK_PLAIN, VH_LANES_BLOCK, VH_BLOCKS_PER_CU, VH_UNIT_ROWS, VH_GRID, VH_EXT_TUPLES,
    // VH_EXT_PAD, VH_HP_AGG_WAVES, VH_HP_REGIONS, VH_DELIVER_BLOCKS, VH_BW_BLOCKS_PER_CU, VH_HP_LOAD_G / _S.
    x.no_topk = false; x.skip_phase2 = false; x.no_direct_emit = false; x.no_jit_pagg = false; x.predpack_bytes = false;
    x.jit_ablate = 0; x.hp_ablate = 0; x.hp_bpp = 0; x.pack_plain = 0; x.lanes_block = 0; x.blocks_per_cu = 0; x.unit_rows = 0; x.grid = 0;
    x.ext_tuples = 0; x.ext_pad = 8; x.hp_agg_waves = 0;
    x.hp_regions = 0;           // regions (row counters) of a big hashed-partitioning result written in ONE launch (measured: C5 14.4 vs 13.9 ms per query, the row counter is not what the aggregation waits for; profiles/r05/NOTES.md)
    x.deliver_blocks = 64;      // blocks of deliver_kernel
    x.bw_blocks_per_cu = 8;
    x.hp_load_g = 0.7; x.hp_load_s = 0.7;
    return x;
  }();
  return k;
}

// Pinned host memory NEXT TO THE GPU. Linux places pages on the NUMA node of the CPU that first touches them, and hipHostMalloc pins (touches)
// them in the calling thread: on a two-socket host the staging buffer of a big result landed on either socket, and device-to-host copies
// into the far one run at 30 GB/s instead of 57 (tools/experiments/d2h_bw2.hip; C5 delivered its 35 M groups in 23 ms or in 13). The calling
// thread therefore sits on the CPUs of the device's own node (sysfs: the PCI device's numa_node and that node's cpulist) while the buffer is
// allocated and touched, and gets its affinity back afterwards. No node information (one socket, a container that hides sysfs): plain allocation.
static std::vector<int> device_node_cpus() {
  std::vector<int> cpus;
  char bdf[64] = "";
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), g_ctx.device) != hipSuccess) return cpus;
  for (char* c = bdf; *c; ++c) *c = (char)tolower(*c);
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  int node = -1;
  if (FILE* f = fopen(path, "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
  if (getenv("VH_HOST_NUMA_NODE")) node = atoi(getenv("VH_HOST_NUMA_NODE"));      // measurement / hosts whose sysfs says -1
  if (node < 0) return cpus;
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE* f = fopen(path, "r");
  if (!f) return cpus;
  char list[4096] = "";
  if (!fgets(list, sizeof(list), f)) list[0] = 0;
  fclose(f);
  for (char* p = list; *p;) {          // "0-63,128-191"
    char* end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    p = end;
    if (*p == '-') { b = strtol(p + 1, &end, 10); p = end; }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c) cpus.push_back((int)c);
    if (*p == ',') ++p; else break;
  }
  return cpus;
}
static hipError_t host_alloc_near_device(void** out, size_t bytes, unsigned flags) {
  static const std::vector<int> cpus = device_node_cpus();
  cpu_set_t old_set, near_set;
  bool moved = false;
  if (!cpus.empty() && bytes >= ((size_t)1 << 20) && sched_getaffinity(0, sizeof(old_set), &old_set) == 0) {
    CPU_ZERO(&near_set);
    int n = 0;
    for (int c : cpus) if (CPU_ISSET(c, &old_set)) { CPU_SET(c, &near_set); ++n; }      // (only CPUs the thread may run on anyway: a cpuset is respected)
    moved = n > 0 && sched_setaffinity(0, sizeof(near_set), &near_set) == 0;
  }
  hipError_t he = hipHostMalloc(out, bytes, flags);
  if (he == hipSuccess && moved) { volatile char* p = static_cast<volatile char*>(*out); for (size_t i = 0; i < bytes; i += 4096) p[i] = 0; }
  if (moved) (void)sched_setaffinity(0, sizeof(old_set), &old_set);
  return he;
}

// The HIP current device is per thread: every entry point that allocates or launches binds the calling thread to the
// library's device first (query threads of a server pool never called vh_init themselves).
#define VH_ENTER() do { if (g_ctx.inited) (void)hipSetDevice(g_ctx.device); } while (0)

extern "C" const char* vh_last_error(void) { return g_err; }
extern "C" const char* vh_version(void) { return "viya_hip 0.1 (gfx950)"; }

extern "C" int vh_init(int device_id) {
  std::lock_guard<std::mutex> lk(g_mu);
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  g_ctx.device = device_id;
  g_ctx.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  g_ctx.lds_per_block = prop.sharedMemPerBlock ? prop.sharedMemPerBlock : 65536;
  g_ctx.num_xcd = 8;
  if (!g_ctx.own_stream) HIP_TRY(hipStreamCreateWithFlags(&g_ctx.own_stream, hipStreamNonBlocking));
  if (!g_ctx.stream) g_ctx.stream = g_ctx.own_stream;
  g_ctx.inited = true;
  (void)knobs();
  return VH_OK;
}

extern "C" int vh_set_stream(void* hip_stream) {
  if (!g_ctx.inited) return vh_fail(VH_E_INVALID, "vh_init has not been called");
  // NULL is a real stream (the legacy default stream, which is what torch.cuda.current_stream() is unless
  // the caller changed it); VH_OWN_STREAM restores the library's private stream
  g_ctx.stream = hip_stream == VH_OWN_STREAM ? g_ctx.own_stream : (hipStream_t)hip_stream;
  return VH_OK;
}


// The host side continues in these files, one translation unit (they share the static state above and each other's types, in this order):
#include "vhh_table.h"
#include "vhh_place.h"
#include "vhh_sync.h"
#include "vhh_derived.h"
#include "vhh_build.h"
#include "vhh_result.h"
#include "vhh_plan.h"
#include "vhh_launch.h"
#include "vhh_exchange.h"
#include "vhh_finalize.h"
#include "vhh_select.h"

extern "C" int vh_measure_read_bandwidth(uint64_t bytes, int32_t iters, double* bytes_per_sec) {
  if (!g_ctx.inited || !bytes_per_sec || iters <= 0) return vh_fail(VH_E_INVALID, "bad argument");
  VH_ENTER();
  bytes = bytes / 16 * 16;
  char* buf = nullptr; unsigned long long* sink = nullptr;
  HIP_TRY(hipMalloc(&buf, bytes));
  HIP_TRY(hipMalloc(&sink, 8));
  HIP_TRY(hipMemsetAsync(buf, 1, bytes, g_ctx.stream));
  HIP_TRY(hipMemsetAsync(sink, 0, 8, g_ctx.stream));
  hipEvent_t a, b;
  HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
  const int grid = g_ctx.num_cu * knobs().bw_blocks_per_cu;   // 256-thread blocks: 8 per CU = 8 waves/SIMD
  hipLaunchKernelGGL(read_bw_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const vh_u32x4*)buf, bytes / 16, sink);
  HIP_TRY(hipEventRecord(a, g_ctx.stream));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(read_bw_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const vh_u32x4*)buf, bytes / 16, sink);
  HIP_TRY(hipEventRecord(b, g_ctx.stream));
  HIP_TRY(hipStreamSynchronize(g_ctx.stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, a, b));
  *bytes_per_sec = (double)bytes * iters / (ms * 1e-3);
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  (void)hipFree(buf); (void)hipFree(sink);
  return VH_OK;
}

#include "vh_sharded.h"

