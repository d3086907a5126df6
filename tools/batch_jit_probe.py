#!/usr/bin/env python3
"""What a batch of VH_PLAN2_PLANE_JIT members gains or loses when ONE kernel compiled for the batch shape answers it (vh_jit_planes_batch.h),
three legs inside ONE process and on one table (boxes and processes differ by more than the legs do). The table is tools/batch_probe.py's:
C3 generated on the device, 125 segments of 1 M rows, m4 drawn from 50 000 values, F = [d2, d3, d4] and V = [d2, m0, count, m4] built
explicitly. Batches of K = 2, 4 and 8 in three shapes:
  1. breakdowns_one_filter  K different breakdowns — totals and GROUP BY d2 over K selections of V's metrics — under C3's ONE filter (one mask class)
  2. totals_k_literals      K totals, SUM(m0) + COUNT, under C3's filter with K different literals for d3 (K mask classes: 22 K filter planes —
                            K = 2 alone fits the 64 planes a batch shape may read; at K = 4 and 8 leg A is what the library does then, K
                            compiled singles, and says so: compiled_groups 0)
  3. totals_k_metrics       K totals without a filter over K different selections of V's metrics (one mask class)
Each batch is measured three ways, rounds interleaved after a warm-up, each round the median of 5:
  A. the plans with VH_PLAN2_PLANE_JIT through vh_query_agg_batch: the compiled fused launch
  B. the same plans with VH_PLAN_NO_JIT | VH_PLAN2_PLANE_AGG: the pre-built fused launch (what the library did for such a dashboard before)
  C. leg A's plans as K vh_query_agg calls, one FINISHED before the next: K compiled single queries whose kernels cannot overlap
  D. leg A's plans through vh_query_agg_batch under VH_TEST_NO_BATCH_FUSE=1: what the library did for a batch of flagged members before — K
     compiled singles launched as they are planned, on K streams, where they overlap. WALL time only: a member's scan_kernel_ms is an
     interval on its own stream and covers the others' run time, so their sum is no kernel time (it is printed, labelled as what it is)
and two figures each: wall time of the call(s) (host clock, results delivered) and kernel time — fused_kernel_ms for a fused launch, the sum
of the K scan_kernel_ms for C. Where a group has no batch shape leg A is the library's fallback, K compiled singles on K streams: wall time
only, like D. All legs must return the same rows. B, C and D are measured in the same process as A: no figure of the code under test is
its own yardstick. Per (shape, K) one JSON line with min / median / max over the rounds, the ratios B / A and C / A of the
minima (> 1: A is faster) in kernel time and, against D too, in wall time, C's own min-to-max spread and whether A beats C by more than that, A's kernel name with its registers and its
compile time (read back from the library's VH_JIT_VERBOSE lines; the disk cache is off so that every kernel is compiled here); then the same
as a Markdown table. A (shape, K) whose legs disagree or did not run as the leg says ends the run there, status 1: nothing more is started.
The library's stderr goes to a file so that the probe can read it back; what is not a `vh jit:` line is passed on to the probe's own stderr
at the end, with the probe's traceback if it failed. The limit that ends a hung run is the CALLER's: run the probe under `timeout -k 10 <seconds>`.
usage: batch_jit_probe.py [segments] [rounds] [shape ...]"""
import atexit, json, os, re, sys, tempfile, time, traceback
os.environ["VH_TEST_HOOKS"] = "1"      # (read once when the library loads: VH_TEST_NO_BATCH_FUSE is then read per call)
os.environ["VH_JIT_NO_DISK_CACHE"] = "1"
os.environ["VH_JIT_VERBOSE"] = "1"
os.environ.pop("VH_TEST_NO_BATCH_FUSE", None)
os.environ.pop("VH_TEST_NO_BATCH_SHARE", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the library's stderr, "vh jit: <name> compiled (<ms> ms, <n> VGPRs)" among it — and this script's own: BATCH_JIT_PROBE_LOG=<path> keeps the file
LOG = open(os.environ["BATCH_JIT_PROBE_LOG"], "w+") if os.environ.get("BATCH_JIT_PROBE_LOG") else tempfile.NamedTemporaryFile(prefix="batch_jit_probe_", suffix=".log")
STDERR = os.fdopen(os.dup(2), "w")      # the probe's own stderr, kept


def replay():
    sys.stderr.flush()
    for line in open(LOG.name, errors="replace"):
        if not line.startswith("vh jit:"):
            STDERR.write(line)
    STDERR.flush()


atexit.register(replay)
os.dup2(LOG.fileno(), 2)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
only = sys.argv[3:]
executor.init(0)
w = synth.c3()
w.columns[11] = synth.SynthColumn("m4", capi.METRIC_MIN, capi.U32, (synth.U, 50_000, 0, 1.0), "uint_min")      # 16 bits instead of 20: V's four fields take 30 of a projection's 32 planes
t = synth.create_device_table(w, seg)
D2, D3, D4, M0, COUNT, M4 = 2, 3, 4, 7, 9, 11
t.predpack([D2, D3, D4], sliced=True)
t.predpack([D2, M0, COUNT, M4], sliced=True)
NOJ, AGG, JIT = capi.PLAN_NO_JIT, capi.PLAN2_PLANE_AGG, capi.PLAN2_PLANE_JIT


def c3_with(k):
    return [("rel", D2, capi.OP_EQ, 1), ("rel", D3, capi.OP_LT, 447 - 25 * k), ("rel", D4, capi.OP_GE, 553), ("and", 3)]


METRICS = [[M0, COUNT], [M0], [COUNT], [M4], [M0, M4], [COUNT, M4], [M0, COUNT, M4], [M4, M0]]


def shapes(K):
    yield "breakdowns_one_filter", [(c3_with(0), [GroupSpec(D2)] if k % 2 else [], METRICS[k]) for k in range(K)], K <= 8
    yield "totals_k_literals", [(c3_with(k), [], [M0, COUNT]) for k in range(K)], 22 * K <= 64
    yield "totals_k_metrics", [([], [], METRICS[k]) for k in range(K)], True


def batch(plans):
    t0 = time.perf_counter()
    res, info = t.query_agg_batch(plans, copy=False)
    wall = (time.perf_counter() - t0) * 1e3
    kern = info.fused_kernel_ms + sum(r.scan_kernel_ms for r in res if not r.batch_fused)      # (a kernel time only where nothing overlaps: see the legs)
    return wall, kern, res, info


def sequential(plans):
    t0 = time.perf_counter()
    res = [t.query_agg(p, copy=False) for p in plans]      # (each waited for and read back before the next is planned)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, sum(r.scan_kernel_ms for r in res), res, None


def singles(plans):
    os.environ["VH_TEST_NO_BATCH_FUSE"] = "1"
    try:
        return batch(plans)
    finally:
        del os.environ["VH_TEST_NO_BATCH_FUSE"]


def rows(r):
    return (r.ngroups, r.passed_recs, [int(x) for k in r.keys for x in k], [int(x) for s in r.states for x in s])


def stat(v):
    return {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)}


def compiled_lines():
    out = {}
    for line in open(LOG.name, errors="replace"):
        m = re.match(r"vh jit: (\S+) compiled \((\d+) ms, (\d+) VGPRs\)", line)
        if m:
            out[m.group(1)] = {"compile_ms": int(m.group(2)), "vgprs": int(m.group(3))}
    return out


def main():
    table = []
    for K in (2, 4, 8):
        for name, spec, fits in shapes(K):
            if only and name not in only:
                continue
            pa = [AggPlan(filter=f, groups=g, metrics=m, flags=0, flags2=JIT) for f, g, m in spec]
            pb = [AggPlan(filter=f, groups=g, metrics=m, flags=NOJ, flags2=AGG) for f, g, m in spec]
            legs = (("A", batch, pa), ("B", batch, pb), ("C", sequential, pa), ("D", singles, pa))
            for _ in range(3):
                for _, run, plans in legs:
                    run(plans)
            # (private copies: a view outlives only the next query of its context)
            va, vb, vc = t.query_agg_batch(pa)[0], t.query_agg_batch(pb)[0], [t.query_agg(p) for p in pa]
            os.environ["VH_TEST_NO_BATCH_FUSE"] = "1"
            vd = t.query_agg_batch(pa)[0]
            del os.environ["VH_TEST_NO_BATCH_FUSE"]
            same = all(rows(a) == rows(b) == rows(c) == rows(d) for a, b, c, d in zip(va, vb, vc, vd))
            wall, kern, last = {l: [] for l, _, _ in legs}, {l: [] for l, _, _ in legs}, {}
            for _ in range(rounds):
                for leg, run, plans in legs:
                    ws, ks = [], []
                    for _ in range(5):
                        wl, kn, res, info = run(plans)
                        ws.append(wl)
                        ks.append(kn)
                    wall[leg].append(sorted(ws)[2])
                    kern[leg].append(sorted(ks)[2])
                    last[leg] = (res, info)
            (ar, ai), (br, bi), (cr, _), (dr, di) = last["A"], last["B"], last["C"], last["D"]
            expected = (ai.compiled_groups == (1 if fits else 0) and all(r.plane_jit and r.batch_fused == fits for r in ar) and
                        bi.fused_groups == 1 and bi.compiled_groups == 0 and all(r.batch_fused and not r.jit for r in br) and
                        all(r.plane_jit and not r.batch_fused for r in cr) and
                        di.fused_groups == 0 and all(r.plane_jit and not r.batch_fused for r in dr))
            sw, sk = {l: stat(v) for l, v in wall.items()}, {l: stat(v) for l, v in kern.items()}
            ratio = lambda s, a, b: round(s[a]["min"] / max(s[b]["min"], 1e-9), 2)
            c_spread = round(sk["C"]["max"] - sk["C"]["min"], 4)
            how = compiled_lines().get(ar[0].kernel, {}) if fits else {}
            overlapping = {"D": sk.pop("D")}      # sums of intervals that overlap: no kernel times
            if not fits:
                overlapping["A"] = sk.pop("A")
            rec = {"shape": name, "K": K, "segments": seg, "legs_agree": same, "as_expected": bool(expected), "A_compiled_fused": bool(fits),
                   "passed_recs": [r.passed_recs for r in ar], "wall_ms": sw, "kernel_ms": sk, "summed_overlapping_intervals_ms": overlapping,
                   "kernel_B_over_A": ratio(sk, "B", "A") if fits else None, "kernel_C_over_A": ratio(sk, "C", "A") if fits else None,
                   "wall_B_over_A": ratio(sw, "B", "A"), "wall_C_over_A": ratio(sw, "C", "A"), "wall_D_over_A": ratio(sw, "D", "A"),
                   "C_spread_ms": c_spread, "A_beats_C_beyond_its_spread": bool(sk["C"]["min"] - sk["A"]["min"] > c_spread) if fits else None,
                   "A_kernel": ar[0].kernel, "A_vgprs": how.get("vgprs"), "A_compile_ms": how.get("compile_ms"), "B_kernel": br[0].kernel}
            print(json.dumps(rec), flush=True)
            table.append(rec)
            if not (same and expected):
                print(json.dumps({"error": "the legs disagree or did not run as they say", "shape": name, "K": K}), flush=True)
                return 1, table
    return 0, table


try:
    status, table = main()
except BaseException:
    traceback.print_exc(file=STDERR)
    STDERR.write(f"(the library's stderr: {LOG.name})\n")
    status, table = 2, []
cell = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}" if s else "-"
print("\n| shape | K | A compiled fused, kernel (min / median / max ms) | B pre-built fused, kernel | C K compiled singles one after the other, kernel | B / A | C / A | C spread ms | A beats C beyond it | A wall | B wall | C wall | D wall (K singles as a batch: they overlap) | wall D / A | A VGPRs | A compile ms |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in table:
    k, wl = r["kernel_ms"], r["wall_ms"]
    yes = {True: "yes", False: "no", None: "-"}[r["A_beats_C_beyond_its_spread"]]
    print(f"| {r['shape']}{'' if r['A_compiled_fused'] else ' (A: no batch shape, K singles)'} | {r['K']} | {cell(k.get('A'))} | {cell(k['B'])} | {cell(k['C'])} | {r['kernel_B_over_A']} | {r['kernel_C_over_A']} | "
          f"{r['C_spread_ms']} | {yes} | {cell(wl['A'])} | {cell(wl['B'])} | {cell(wl['C'])} | {cell(wl['D'])} | {r['wall_D_over_A']} | {r['A_vgprs']} | {r['A_compile_ms']} |")
t.close()
sys.exit(status)
