#!/usr/bin/env python3
"""bench.py — the hot path (filtered GROUP-BY aggregate) on N MI355X GPUs of one node.

A "step" = one execution of the workload's aggregate query over the table shard(s)
resident in HBM: plan upload -> scan/filter/aggregate kernel -> [per-XCD merge] ->
[N>1: RCCL reduce of the dense partial tables to rank 0 over xGMI] -> group
materialisation in host memory (SURVEY.md §8(d) timing window).

Workload (BASELINE.json): N=1 runs configs[2] "C3" — 1 B rows / 12 columns (60 GB in HBM),
conjunctive 3-predicate filter (~5 %), GROUP BY 2 dims (~100 K groups), SUM + COUNT — the
configuration the metric (rows/s + achieved HBM GB/s) is quoted on.  N>1 runs configs[3]
"C4": the SAME 1 B rows sharded as contiguous blocks of segments across the ranks (strong
scaling: total work fixed), with an RCCL reduce of the per-GPU partial aggregates.

A plain run does what the headline needs and nothing else: it generates and prepares the table, runs the warm-up steps, times the
steps, writes --dump-outputs if asked and prints the line (roofline included: it is computed from the timed steps and the committed
PMC summaries, no run of its own). --full adds everything else the benchmark measures or checks, as it always has: the parity gate
before the warm-up, and at N=1 after the timed steps the reference-layout leg, the unprepared-caller leg and both CPU baselines.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)
DUMP_LIMIT_BYTES = 64_000_000   # --dump-outputs: at most this much in all (64 MB)
DUMP_SEED = 42                # ... and the sample of the groups it takes above that


def kernel_sources_hash() -> str:
    """Identity of the device code a profile was taken with: a hash over every file of viyadb_amd/csrc/ and include/ (the
    GPU box has no .git to ask). tools/profile_round.sh stamps each PMC summary with it; a summary whose stamp differs from
    the tree being timed describes other kernels and is refused (the round-2 line replayed a stale profile)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "viyadb_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def measured_traffic(workload: str, rows_on_rank: int, kernel: str, packed: bool, narrow: bool):
    """HBM bytes per launch from the newest committed rocprofv3 PMC summary (profiles/rNN/) whose recorded kernel is the
    kernel that just ran AND whose device sources are the ones being timed, scaled by rows. PMC counters cannot be read inside
    a normal run (tools/profile_round.sh collects them with the same command line); a summary taken with another kernel, another
    layout or other sources is refused: traffic = null, and the reason is reported."""
    import glob
    first = kernel.split(" + ")[0]
    want = kernel_sources_hash()
    why = "no PMC summary of kernel %s under profiles/" % first
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "%s_1gpu_pmc_hbm*.json" % workload.lower())), reverse=True):
        d = json.load(open(f))
        if first and first in d.get("kernel", "") and bool(d.get("packed", False)) == bool(packed) and bool(d.get("narrow", False)) == bool(narrow):
            if d.get("sources") != want:
                why = "%s was taken with other device sources (%s, this tree is %s)" % (os.path.relpath(f, ROOT), d.get("sources"), want)
                continue
            scale = rows_on_rank / d["rows"]
            return d["B_meas_per_launch"] * scale, os.path.relpath(f, ROOT), d.get("head"), d.get("write_bytes_raw", 0) * scale, None
    return None, None, None, None, why


def parity_gate(table, w, plan, my_segments, executor):
    """Before anything is timed ("parity gate before any number is reported"), on this rank's shard, through the
    library calls the timed loop makes: (1) an exact comparison with the oracle on a window of segments of the SAME generated
    rows; (2) size-independent properties over the whole shard — the plan's result against an independent table organisation
    (the open-addressing hash table) bit for bit, and its totals against a GROUP-BY-less query (another kernel instantiation)."""
    import numpy as np
    from oracle import viya_oracle as vo
    from tests.parity import build_oracle_table, compare
    t0 = time.time()
    has_sets = any(c.elem >= 10 for c in w.columns)              # per-row id sets: the numpy oracle walks them one by one
    win = 1 if has_sets else min(2, my_segments)
    win_rows = min(w.segment_rows, 100_000) if has_sets else w.segment_rows
    first = max(0, my_segments // 2 - 1)
    snap = [0] * my_segments
    for s in range(first, first + win):
        snap[s] = win_rows
    p = executor.AggPlan(filter=plan.filter, groups=plan.groups, metrics=plan.metrics, flags=plan.flags, groups_hint=plan.groups_hint, seg_rows=snap)
    res = table.query_agg(p)
    base = getattr(table, "_row_base", 0) + first * w.segment_rows
    st = vo.scan_aggregate(vo.parse_query(build_oracle_table(w, win, win_rows, row_base=base), w.query), now=getattr(w, "now", None))
    st.scanned_recs, st.scanned_segments = res.scanned_recs, res.scanned_segments     # hidden segments still count as scanned
    compare(res, st, "bench parity gate (oracle window)")
    full = table.query_agg(plan)
    other = table.query_agg(executor.AggPlan(filter=plan.filter, groups=plan.groups, metrics=plan.metrics, flags=1, groups_hint=plan.groups_hint))
    assert full.ngroups == other.ngroups and full.passed_recs == other.passed_recs, "table organisations disagree"

    def canon(r):
        o = np.lexsort([k for k in reversed(r.keys)]) if r.keys else np.arange(r.ngroups)
        return [k[o] for k in r.keys] + [x[o] for x in r.states]
    for a, b in zip(canon(full), canon(other)):
        assert np.array_equal(a, b), "table organisations disagree"
    tot = table.query_agg(executor.AggPlan(filter=plan.filter, groups=[], metrics=plan.metrics))
    for j, sj in enumerate(full.states):
        if sj.dtype.kind in "iu" and table.cols[plan.metrics[j]][0] in (18, 20):       # SUM / COUNT: wrap like the column's own type
            assert int(sj.sum(dtype=np.uint64 if sj.dtype.kind == "u" else np.int64)) & ((1 << (8 * sj.dtype.itemsize)) - 1) == \
                int(tot.states[j][0]) & ((1 << (8 * sj.dtype.itemsize)) - 1), "totals disagree"
    return {"oracle_window_segments": win, "oracle_window_rows": win * win_rows, "oracle_groups": st.ngroups,
            "cross_path": "dense vs hash organisation, bit-exact over %d rows" % full.scanned_recs, "seconds": round(time.time() - t0, 2)}


def dump_outputs(res, w, plan, out_dir: str) -> dict:
    """--dump-outputs: what the timed path returned in its last step — the group keys, the metric states and (AVG) the hidden counts —
    as <out_dir>/<name>.npy in float64. The groups are written sorted by their keys (the library's order depends on the table path),
    so that two builds can be compared array for array. When the arrays exceed DUMP_LIMIT_BYTES, a fixed seeded sample of the sorted
    groups is written instead, and group_index.npy holds the samples' positions in the sorted order."""
    import numpy as np
    arrays = [("key%d_%s" % (i, w.columns[g.col].name), k) for i, (g, k) in enumerate(zip(plan.groups, res.keys))]
    arrays += [("state%d_%s" % (j, w.columns[m].name), s) for j, (m, s) in enumerate(zip(plan.metrics, res.states))]
    if res.hidden_count is not None:
        arrays.append(("hidden_count", res.hidden_count))
    ng = len(arrays[0][1]) if arrays else 0
    order = np.lexsort([k for k in reversed(res.keys)]) if res.keys else np.arange(ng)
    keep = (DUMP_LIMIT_BYTES - 4096 * (len(arrays) + 1)) // (8 * (len(arrays) + 1))      # (+1: group_index; 4 KB per .npy header)
    sampled = ng > keep
    if sampled:
        pos = np.sort(np.random.default_rng(DUMP_SEED).choice(ng, keep, replace=False))
        order = order[pos]
        arrays.append(("group_index", pos))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays:
        np.save(os.path.join(out_dir, name + ".npy"), (a if name == "group_index" else a[order]).astype(np.float64))
    return {"dir": out_dir, "arrays": [n for n, _ in arrays], "groups": ng, "written_groups": len(order), "sampled": sampled}


def cpu_baseline(w, sample_segments: int):
    """The reference's algorithm (oracle/cpu_twin.py: emitted C++, the reference's g++ flags,
    one thread) on a bounded sample of the same synthetic rows. Checker-side code only."""
    from oracle import cpu_twin
    from tests.parity import build_oracle_table
    rows_per_seg = w.segment_rows
    # "pinned to 1 core (taskset)". The process is bound to ONE core before the sample table is generated, so that its pages
    # are first touched — and therefore placed — on that core's NUMA node, and stays there for the timed runs.
    pinned, old_aff = None, None
    if hasattr(os, "sched_setaffinity"):
        try:
            old_aff = os.sched_getaffinity(0)
            pinned = sorted(old_aff)[len(old_aff) // 2]          # (not core 0: interrupts and the launcher tend to live there)
            os.sched_setaffinity(0, {pinned})
        except OSError:
            pinned, old_aff = None, None
    try:
        return _cpu_baseline_pinned(w, sample_segments, rows_per_seg, pinned, cpu_twin, build_oracle_table)
    finally:
        if old_aff is not None:
            os.sched_setaffinity(0, old_aff)


def _cpu_baseline_pinned(w, sample_segments, rows_per_seg, pinned, cpu_twin, build_oracle_table):
    ot = build_oracle_table(w, sample_segments, rows_per_seg, csr=True)      # (bitset columns as CSR arrays: the twin reads them as they are)
    tw = cpu_twin.Twin(ot, w.query)
    now = getattr(w, "now", None)
    state = tw.run(now=now)  # warm-up (page-in); its groups also check the GPU's answer over the same rows (main)
    secs = []
    for _ in range(7):
        tw.run(now=now)
        secs.append(tw.last_seconds)
    best = sorted(secs)[len(secs) // 2]
    rows = sample_segments * rows_per_seg
    return {"value": rows / best, "unit": "rows/s", "cores": 1, "kind": "port", "pinned_core": pinned,
            "sample": "%d segments x %d rows of %s (same generator, same query), median of 7 runs, "
                      "g++ -O2 -funroll-loops -march=native, 1 thread %s; %.2f GB/s of referenced bytes%s"
                      % (sample_segments, rows_per_seg, w.name, ("pinned to core %d (sched_setaffinity)" % pinned) if pinned is not None else "(not pinned: no sched_setaffinity)",
                         rows * w.bytes_per_row_referenced / best / 1e9,
                         "; count distinct: CRoaring replaced by a lazily compacted std::vector per group (oracle/cpu_twin.py: errs on the fast side)" if any(c.elem >= 10 for c in w.columns) else ""),
            "cpu": _cpu_model()}, state


def cpu_baseline_parallel(w, seconds: float = 3.0, segments_per_worker: int = 2):
    """Courtesy baseline #2 of SURVEY 8(d) — NOT reference behaviour (the reference runs a query on one thread): the
    same emitted loop, segment-parallel, one process per core, each over its own segments inside a common window."""
    import subprocess
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    workers = max(1, min(cores, 64))
    start = time.time() + 12.0 + 0.05 * workers          # generation of the shards happens before the window opens (a worker that comes late says so)
    procs = [subprocess.Popen([sys.executable, "-m", "oracle.parallel_worker", w.name, str(segments_per_worker),
                               str(i * segments_per_worker), repr(start), repr(seconds)], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True) for i in range(workers)]
    rows, ok, missed = 0, 0, 0
    for p in procs:
        out, _ = p.communicate(timeout=180)
        try:
            d = json.loads(out.strip().splitlines()[-1])
            rows += d["rows"]
            ok += 1
            missed += 1 if d.get("missed", 0) > 0.05 else 0
        except Exception:
            pass
    return {"value": rows / seconds if ok else None, "unit": "rows/s", "cores": ok, "kind": "port, segment-parallel (not reference behaviour)",
            "sample": "%d processes x %d segments of %s, each looping over its own segments for the same %.0f s window; %d of the %d started more than "
                      "50 ms late (their share of the window is overstated by that much)" % (ok, segments_per_worker, w.name, seconds, missed, ok)}


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` from a plain shell (no WORLD_SIZE / RANK in the environment): re-execute this very command line as
    N ranks of one node under torch.distributed.run — what the contract's launcher line does — on a free port of 127.0.0.1. Rank 0's JSON
    line is the only thing the ranks write to stdout; it passes through, the ranks' stderr too. Returns the launcher's exit code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on these hosts: RCCL's peer mappings need it
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: launching %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def rendezvous_only(rank: int, world: int, local_rank: int):
    """The launcher's own check (tests/test_bench_launch.py, no GPU needed): the ranks meet over gloo and rank 0 says who came."""
    import socket
    import torch.distributed as dist
    dist.init_process_group("gloo")
    who = [None] * world
    dist.all_gather_object(who, {"rank": rank, "local_rank": local_rank, "pid": os.getpid(), "host": socket.gethostname()})
    dist.barrier()
    if rank == 0:
        print(json.dumps({"launched": True, "n_ranks": world, "ranks": who}), flush=True)
    dist.destroy_process_group()


def comm_report(comm, dist, world: int, backend: str):
    """The "rccl" object of the output line: what every rank's communicator says it is (vh_comm_info, read back from RCCL itself, gathered
    over the control plane) — rank count, devices, transport — so that a line measured over a fallback transport cannot pass for RCCL."""
    mine = comm.info()
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    transports = sorted({e["transport"] for e in everyone})
    ok = transports == ["rccl"] and all(e["nranks"] == world for e in everyone) and len({e["pci_bus_id"] for e in everyone}) == world
    return {"nranks": everyone[0]["nranks"], "ranks_agree": all(e["nranks"] == everyone[0]["nranks"] for e in everyone),
            "devices": ["%s (hip:%d)" % (e["pci_bus_id"], e["device"]) for e in everyone],
            "distinct_devices": len({e["pci_bus_id"] for e in everyone}),
            "transport": "rccl" if transports == ["rccl"] else "gloo-fallback", "detail": backend}, not ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--segments", type=int, default=0, help="total segments (default: 1000 for C3, 100 for C2, 10 for C1)")
    ap.add_argument("--segment-rows", type=int, default=1_000_000)
    ap.add_argument("--full", action="store_true", help="also run what the headline does not need: the parity gate, and at N=1 the reference-layout "
                                                         "and unprepared-caller legs and both CPU baselines (each --no-* below leaves one out again)")
    ap.add_argument("--cpu-segments", type=int, default=100, help="CPU baseline sample (--full): this many segments of the same workload")
    ap.add_argument("--no-cpu", action="store_true", help="skip both CPU baselines of --full")
    ap.add_argument("--cpu-parallel", action="store_true", help="(default of --full at N=1) also time the courtesy all-cores CPU baseline (adds ~20 s)")
    ap.add_argument("--no-cpu-parallel", action="store_true", help="skip the courtesy all-cores CPU baseline of --full")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--no-pack", action="store_true", help="ablation: no payload projection (survivors gather from the column arenas)")
    ap.add_argument("--no-check", action="store_true", help="skip the parity gate of --full (profiling runs)")
    ap.add_argument("--no-predpack", action="store_true", help="ablation: narrow copies of the predicate columns (round 4's layout) instead of the bit-packed predicate projection")
    ap.add_argument("--no-warm", action="store_true", help="no vh_table_prepare: the first queries pay the first-use costs")
    ap.add_argument("--no-reference-layout", action="store_true", help="skip the arena-only leg of --full (profiling runs)")
    ap.add_argument("--no-unprepared", action="store_true", help="skip the unprepared-caller leg of --full (a second table: profiling runs)")
    ap.add_argument("--rendezvous-only", action="store_true", help="launch the ranks, meet over gloo, print who came, stop (the launcher's own test: needs no GPU)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the last step's result arrays to DIR/<name>.npy (float64, groups sorted by key, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        raise SystemExit(self_launch(args.gpus))       # a plain `python bench.py --gpus N`: become N ranks under torch.distributed.run

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: the two must agree (a plain `python bench.py --gpus N` launches its own ranks)" % (args.gpus, world))
    if args.rendezvous_only:
        return rendezvous_only(rank, world, local_rank)
    # One rank per GPU. torch.distributed (gloo) is the CONTROL plane only: rendezvous, the RCCL unique id, barriers and the
    # max-over-ranks of the timing. The data plane — plan agreement, verdict all-reduce, ncclReduce of the partial tables — is
    # the library's own RCCL communicator behind vh_query_agg_sharded. VH_BENCH_BACKEND=gloo swaps that transport for
    # callbacks over gloo so the N>1 flow can run on a box with fewer GPUs than ranks (tests).
    backend = os.environ.get("VH_BENCH_BACKEND", "nccl")
    local_rank %= max(1, torch.cuda.device_count())     # (more ranks than GPUs only happens in tests; RCCL then refuses and the gloo transport takes over)
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")

    from viyadb_amd import capi, distributed, executor, synth
    executor.init(local_rank)
    comm = None
    if world > 1:
        if backend == "nccl":
            # RCCL inside the library; if the communicator cannot be created on some rank (no RCCL, no peer access), every rank falls
            # back to the callback transport over gloo — a slower data plane, named as such in the output line, rather than no number
            err = None
            try:
                comm = distributed.Comm.rccl(dist)
            except Exception as e:   # noqa: BLE001
                err = "%s: %s" % (type(e).__name__, e)
            errs = [None] * world
            dist.all_gather_object(errs, err)
            if any(errs):
                if comm is not None:
                    comm.close()
                comm = distributed.Comm.gloo(dist)
                backend = "gloo (RCCL communicator failed: %s)" % next(e for e in errs if e)
        else:
            comm = distributed.Comm.gloo(dist)
    rccl_info, degraded = (None, False) if world == 1 else comm_report(comm, dist, world, backend)

    w = synth.WORKLOADS[args.workload](segment_rows=args.segment_rows)
    total_segments = args.segments or {"C1": 10, "C2": 100, "C3": 1000, "C5t": 100, "C5": 100}[args.workload]
    # contiguous block of segments per rank; global row ids are preserved
    seg_lo, seg_hi = distributed.shard_segments(total_segments, rank, world)
    my_segments = seg_hi - seg_lo
    t_gen = time.time()
    table = synth.create_device_table(w, my_segments, w.segment_rows, row_base=seg_lo * w.segment_rows)
    table._row_base = seg_lo * w.segment_rows
    torch.cuda.synchronize()
    t_gen = time.time() - t_gen
    # (a count distinct over 32-bit ids is asked for as a uint32 column: a third less to deliver for C5's 35 M groups)
    plan = executor.AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics,
                            flags=args.flags | capi.PLAN_CARD32 | ((capi.PLAN_NO_PACK | capi.PLAN_NO_NARROW) if args.no_pack else 0), groups_hint=w.plan.groups_hint)

    table.prepare(plan)   # the plan's C structs are built once, like a prepared statement
    # ... and so is the payload projection of its group + metric columns (vh_table_pack): part of the resident mirror,
    # like the column arenas; the reference's analogue is the g++ compile it caches per query shape
    t_pack = time.time()
    if not args.no_pack:
        table.pack(table.gather_columns(plan))
        if args.no_predpack:
            table.narrow(table.filter_columns(plan))     # 8- / 16-bit copies of the predicate columns whose values fit (vh_table_narrow)
        else:
            table.predpack(table.filter_columns(plan))   # the predicate columns as bit fields of one word per row, bit-sliced (vh_table_predpack: C3 22 planes of one bit per row = 2.75 bytes)
    torch.cuda.synchronize()
    t_layout = time.time() - t_pack      # the derived layouts alone (two passes over the referenced columns); the compile below is the other one-time cost
    # first-use costs paid before anything is timed, as a database would at table-load time for its hot query shapes (vh_table_prepare:
    # the compile of the scan kernel for this shape, the derived layouts above if not asked for explicitly)
    warmed = 0 if args.no_warm else table.warm(plan)
    torch.cuda.synchronize()
    t_pack = time.time() - t_pack

    checked = None
    if args.full and not args.no_check:
        checked = parity_gate(table, w, plan, my_segments, executor)   # every rank checks its own shard; raises on any difference

    def step():
        # copy=False: result arrays alias the library's pinned staging buffer (no second host copy)
        if world == 1:
            return table.query_agg(plan, copy=False)
        return distributed.sharded_query(table, plan, comm, root=0, copy=False)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    last = None
    for _ in range(args.warmup):
        last = step()
    barrier()
    t0 = time.perf_counter()
    kernel_ms = []
    for _ in range(args.steps):
        last = step()
        if last is not None:
            kernel_ms.append(last.scan_kernel_ms)
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # now: `last` aliases the staging buffer that the queries below write into
        print("bench.py: --dump-outputs %s" % json.dumps(dump_outputs(last, w, plan, args.dump_outputs)), file=sys.stderr, flush=True)

    # The same query on the REFERENCE layout — the 4-byte column arenas only, no payload projection, no narrow predicate copies
    # (VH_PLAN_NO_PACK | VH_PLAN_NO_NARROW) — timed in the same run, after the headline loop: what the kernels do with the
    # bytes the reference's Segment holds, so that rounds stay comparable whatever the derived layouts buy.
    ref_layout = None
    if args.full and world == 1 and not args.no_pack and not args.no_reference_layout:
        rplan = executor.AggPlan(filter=plan.filter, groups=plan.groups, metrics=plan.metrics, groups_hint=plan.groups_hint,
                                 flags=args.flags | capi.PLAN_NO_PACK | capi.PLAN_NO_NARROW)
        table.prepare(rplan)
        rsteps = max(3, min(args.steps, 10))
        for _ in range(2):
            rlast = table.query_agg(rplan, copy=False)
        torch.cuda.synchronize()
        r0 = time.perf_counter()
        rk = []
        for _ in range(rsteps):
            rlast = table.query_agg(rplan, copy=False)
            rk.append(rlast.scan_kernel_ms)
        torch.cuda.synchronize()
        rel = time.perf_counter() - r0
        ref_layout = (rlast, rel / rsteps, sum(rk) / len(rk), rsteps)
        table.prepare(plan)
    # An UNPREPARED caller: a second table of the same rows that nobody calls vh_table_prepare / vh_table_pack / vh_table_predpack
    # on — the query simply arrives, eight times. The first one pays the kernel's compile (or its load from the disk cache), the first few read the
    # reference's layout, and the library builds the derived layouts unasked once the shape has been seen VH_AUTO_PACK / VH_AUTO_NARROW (3) times:
    # what every one of those queries costs is in the line, next to what the prepared table's cost.
    unprepared = None
    if args.full and world == 1 and not args.no_pack and not args.no_unprepared and not args.no_warm:
        try:
            t2 = synth.create_device_table(w, my_segments, w.segment_rows, row_base=seg_lo * w.segment_rows)
            torch.cuda.synchronize()
            uplan = executor.AggPlan(filter=plan.filter, groups=plan.groups, metrics=plan.metrics, flags=plan.flags, groups_hint=plan.groups_hint)
            per, kern, packed_at = [], [], None
            for i in range(10):
                q0 = time.perf_counter()
                ur = t2.query_agg(uplan, copy=False)
                per.append(round((time.perf_counter() - q0) * 1e3, 3))
                kern.append(round(ur.scan_kernel_ms, 3))
                if packed_at is None and ur.packed and ur.predpack:
                    packed_at = i
            unprepared = {"what": "a second table of the same rows, no vh_table_prepare / pack / predpack: the same query ten times from a caller that prepares nothing",
                          "per_query_ms": per, "kernel_ms": kern, "derived_layouts_in_use_from_query": packed_at, "steady_ms": sorted(per[-3:])[1],
                          "kernel": ur.kernel, "groups": ur.ngroups}
            t2.close()
        except Exception as e:   # noqa: BLE001 - a courtesy leg must not take the number down
            unprepared = {"failed": repr(e)[:300]}
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    total_rows = total_segments * w.segment_rows
    ms_per_step = elapsed / args.steps * 1e3
    value = total_rows / (elapsed / args.steps)
    if rank != 0:
        table.close()
        comm.close()
        dist.destroy_process_group()
        return
    avg_kernel_ms = sum(kernel_ms) / len(kernel_ms)
    rows_rank0 = my_segments * w.segment_rows
    # B_ref per launch on this rank: rows x referenced bytes/row (the library counts fixed-width columns; a bitset metric's CSR offsets and
    # ids — C5: 8 + 2 x 4 bytes per row — come from the workload's own figure)
    algo_bytes = max(last.algorithmic_bytes, rows_rank0 * w.bytes_per_row_referenced)
    # B_min of SURVEY 8(d): filter columns in full + the other referenced columns for passing rows only
    fcols = sorted({f[1] for f in w.plan.filter if f[0] in ("rel", "in")})
    fbytes = sum(capi.ELEM_SIZE[w.columns[c].elem] for c in fcols)
    b_min = rows_rank0 * fbytes + last.passed_recs * max(0, w.bytes_per_row_referenced - fbytes)
    traffic, traffic_src, traffic_head, traffic_write, traffic_why = measured_traffic(args.workload, my_segments * w.segment_rows, last.kernel, last.packed, last.narrow)
    # never credit more than was moved. Without a PMC pass of this very kernel and layout, credit B_min — what ANY
    # implementation must move (filter columns in full at their declared width + the passing rows' payload) — rather than B_ref:
    # with projections and narrow copies the query reads far less than it references, and B_ref / t can exceed the HBM peak
    credited = min(algo_bytes, traffic) if traffic else min(algo_bytes, b_min)
    achieved = credited / (avg_kernel_ms * 1e-3) / 1e9 if avg_kernel_ms > 0 else 0.0

    if rank == 0:
        out = {
            "metric": "rows/sec, filtered GROUP-BY SUM (+ achieved HBM GB/s in roofline)",
            "value": value, "unit": "rows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "strong",
            "degraded": bool(degraded),       # true = N > 1 but the data plane was NOT RCCL over distinct GPUs (see "rccl")
            "rccl": rccl_info,
            "full": bool(args.full),          # false = the headline alone: no parity gate, no reference_layout / unprepared / CPU legs
            "parity_checked": bool(checked), "parity": checked,
            "vs_baseline": None, "dtype": "u32 predicates (compared as bit fields of a packed word / u8 / u16 where such a copy exists) / int64 + u32 integer sums", "data": "synthetic",
            "config": {"workload": "%s: %s" % (w.name if world == 1 else w.name + " sharded (C4)", w.description),
                       "rows": total_rows, "segments": total_segments, "segment_rows": w.segment_rows,
                       "columns": len(w.columns), "table_bytes": total_rows * w.table_bytes_per_row,
                       "groups": last.ngroups, "passed_rows_rank0": last.passed_recs,
                       "table_path": last.path, "parallelism": ("segments sharded x%d, vh_query_agg_sharded: plan agreement + ncclReduce of the partial tables to rank 0 (%s transport)"
                                                                % (world, "RCCL" if backend == "nccl" else "callbacks over " + backend)) if world > 1 else "1 GPU",
                       "generate_seconds": round(t_gen, 3), "payload_projection": bool(last.packed), "narrow_predicates": bool(last.narrow), "predicate_projection": bool(last.predpack), "streamed_payload": bool(last.streamed_payload),
                       "compiled_kernel": bool(last.jit), "prepared": not args.no_warm,
                       "one_word_tuples": bool(warmed & 1024),
                       "pack_seconds": round(t_pack, 3), "device_bytes": table.info()[2]},
            # what the derived layouts cost, first class: built once (like the reference's per-query g++ compile, outside its steady
            # state), resident next to the table
            "unprepared": unprepared,
            "derived_layout": {"one_time_seconds": round(t_layout, 4),
                               # ... and the other first-use cost of the shape: the scan kernel's compile by hipRTC, or its load from the disk cache (vh_table_prepare)
                               # (vh_table_prepare: the compile or load, up to three settling runs of the query, and a place for the derived layouts found by
                               # measurement — up to VH_PREPARE_PLACE = 8 candidates, each a device-to-device copy of the layouts + three queries)
                               "kernel_compile_or_load_seconds": round(t_pack - t_layout, 4),
                               "prepare_seconds": round(t_pack - t_layout, 4),
                               "break_even_queries_with_prepare": (round(t_pack / max(1e-9, ref_layout[1] - elapsed / args.steps)) if ref_layout is not None and ref_layout[1] > elapsed / args.steps else None),
                               # queries of this shape after which building the derived layouts has paid for itself: one-time seconds / (what a query costs
                               # on the reference's layout - what it costs on the derived ones), both measured in this run
                               "break_even_queries": (round(t_layout / max(1e-9, ref_layout[1] - elapsed / args.steps)) if ref_layout is not None and ref_layout[1] > elapsed / args.steps else None), "extra_device_bytes": max(0, table.info()[2] - total_rows * w.table_bytes_per_row // max(1, world)),
                               "table_bytes": total_rows * w.table_bytes_per_row // max(1, world),
                               "what": ("payload projection of the group + metric columns (vh_table_pack) and " + ("8- / 16-bit copies of the predicate columns (vh_table_narrow)" if args.no_predpack else
                                        "the predicate columns as bit fields of one word per row, bit-sliced: one plane per bit, compared 32 rows per lane at a time (vh_table_predpack)")) if not args.no_pack else "none"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "kernel": last.kernel,
                         "kernel_ms": avg_kernel_ms,
                         "algorithmic_bytes_per_launch": algo_bytes, "b_min_bytes_per_launch": b_min,
                         "bref_over_t_GBs": algo_bytes / (avg_kernel_ms * 1e-3) / 1e9 if avg_kernel_ms > 0 else 0.0,
                         "frac_ref": algo_bytes / (avg_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if avg_kernel_ms > 0 else 0.0,
                         "traffic_write": traffic_write,
                         # every byte the kernels moved (fetched x2 + written) over their time: what the memory system did, whatever the min rule credits
                         "moved_GBs": (traffic + (traffic_write or 0)) / (avg_kernel_ms * 1e-3) / 1e9 if traffic and avg_kernel_ms > 0 else None,
                         "frac_moved": (traffic + (traffic_write or 0)) / (avg_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if traffic and avg_kernel_ms > 0 else None,
                         "traffic_source": traffic_src, "traffic_head": traffic_head, "traffic_refused": traffic_why,
                         "kernel_sources": kernel_sources_hash(),
                         "note": "achieved = min(B_ref, B_meas) / mean HIP-event time of the scan kernel(s) on rank 0 "
                                 "(SURVEY 8d: never more than was moved, never more than the algorithm references); B_ref = rows x "
                                 "referenced bytes/row; B_meas = rocprofv3 FETCH_SIZE x2 (gfx950 correction, MI355X_MICROARCH.md) from "
                                 "the committed PMC pass of this kernel (same payload source), scaled by rows; traffic_write = WRITE_SIZE of "
                                 "that pass, raw; traffic null = no pass of this kernel and layout committed (then B_min is credited); "
                                 "bref_over_t_GBs / frac_ref = B_ref / t, what round 1 and SURVEY's >= 60 % target were quoted on. The min rule credits bytes MOVED: "
                                 "a layout that avoids bytes (payload projection, narrow predicate copies) lowers frac while the query gets faster - "
                                 "compare kernel_ms / value across rounds (round 1: 5.03 ms, frac 0.66 with 26.5 GB moved)"},
        }
        if ref_layout is not None:
            rl, rsec, rkms, rsteps = ref_layout
            rtraffic, rsrc, rhead, rwrite, rwhy = measured_traffic(args.workload, my_segments * w.segment_rows, rl.kernel, rl.packed, rl.narrow)
            rcred = min(rl.algorithmic_bytes, rtraffic) if rtraffic else min(rl.algorithmic_bytes, b_min)
            out["reference_layout"] = {
                "what": "the same query with VH_PLAN_NO_PACK | VH_PLAN_NO_NARROW: every referenced column read from its 4-byte / 8-byte arena, as the reference's Segment lays them out",
                "value": total_rows / rsec, "unit": "rows/s", "ms_per_step": rsec * 1e3, "steps": rsteps, "kernel_ms": rkms, "kernel": rl.kernel, "table_path": rl.path,
                "compiled_kernel": bool(rl.jit),
                "roofline": {"achieved": rcred / (rkms * 1e-3) / 1e9, "frac": rcred / (rkms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": rtraffic, "traffic_write": rwrite,
                             "traffic_source": rsrc, "traffic_refused": rwhy,
                             "bref_over_t_GBs": rl.algorithmic_bytes / (rkms * 1e-3) / 1e9}}
        if args.full and world == 1 and not args.no_cpu:
            twin_state = None
            try:
                # (sparse groups: the twin's unordered_map grows with the sample — C5's 5 segments are ~4.5 M groups, ~10-20 s of CPU for the 8 runs)
                cpu_segs = min(args.cpu_segments, total_segments, 5 if w.name.startswith("C5") else args.cpu_segments)
                out["cpu_baseline"], twin_state = cpu_baseline(w, cpu_segs)
            except Exception as e:  # the CPU leg must never take the GPU number down with it
                out["cpu_baseline"] = {"value": None, "unit": "rows/s", "cores": 1, "kind": "port", "sample": "failed: %r" % (e,)}
            if twin_state is not None and not args.no_check:
                # the CPU leg's groups are the oracle's answer for the first cpu_segments segments: the GPU's answer over exactly those
                # rows (a size() snapshot that hides the rest) must be the same, group for group — a tenth of the table instead of the
                # two segments the numpy oracle checks before the timed loop. A difference is an error, not a line.
                from tests.parity import compare
                ns = cpu_segs
                snap = [w.segment_rows] * ns + [0] * (my_segments - ns)
                wres = table.query_agg(executor.AggPlan(filter=plan.filter, groups=plan.groups, metrics=plan.metrics, flags=plan.flags,
                                                        groups_hint=plan.groups_hint, seg_rows=snap))
                twin_state.scanned_recs, twin_state.scanned_segments = wres.scanned_recs, wres.scanned_segments
                if twin_state.passed_recs < 0:       # (the emitted loop keeps no such counter; the groups below are the check)
                    twin_state.passed_recs = wres.passed_recs
                compare(wres, twin_state, "bench parity gate (CPU twin window)")
                out["parity"]["cpu_twin_window_rows"] = ns * w.segment_rows
                out["parity"]["cpu_twin_groups"] = twin_state.ngroups
            if not args.no_cpu_parallel:
                try:
                    out["cpu_baseline_all_cores"] = cpu_baseline_parallel(w)
                except Exception as e:
                    out["cpu_baseline_all_cores"] = {"value": None, "sample": "failed: %r" % (e,)}
        print(json.dumps(out), flush=True)
    table.close()
    if world > 1:
        comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
