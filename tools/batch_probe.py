#!/usr/bin/env python3
"""What a fused batch (vh_query_agg_batch: scan_agg_planes_batch_kernel) gains or loses against the same plans asked one by one, A/B inside ONE
process and on one table (boxes and processes differ by more than the variants do). C3 is generated on the device (vh_segment_generate), 125
segments of 1 M rows, m4 drawn from 50 000 values so that V fits 32 planes; F = [d2, d3, d4] and V = [d2, m0, count, m4] are built explicitly. Batches of K = 2, 4 and 8 in three shapes, all under
VH_PLAN_NO_JIT | VH_PLAN2_PLANE_AGG:
  1. totals_k_literals   K totals, SUM(m0) + COUNT, under C3's filter with K different literals for d3
  2. by_d2_k_filters     K GROUP BY d2 under the same K filters
  3. totals_k_metrics    K totals without a filter over K different selections of V's metrics
Each batch is measured two ways, rounds interleaved after a warm-up, each round the median of 5:
  a. fused       one vh_query_agg_batch call
  b. sequential  K vh_query_agg calls of the same plans (the path every caller has without the batch entry point)
and two figures each: wall time of the batch (host clock around the calls, results delivered) and kernel time — fused_kernel_ms against the sum
of the K scan_kernel_ms. The members of a must all be fused and must return what b returns. One JSON line per (shape, K) with min / median /
max over the rounds and the ratios b / a of the minima (> 1: the batch is faster); then the same as a Markdown table.
usage: batch_probe.py [segments] [rounds]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
executor.init(0)
w = synth.c3()
w.columns[11] = synth.SynthColumn("m4", capi.METRIC_MIN, capi.U32, (synth.U, 50_000, 0, 1.0), "uint_min")      # 16 bits instead of 20: V's four fields take 30 of a projection's 32 planes
t = synth.create_device_table(w, seg)
D2, D3, D4, M0, COUNT, M4 = 2, 3, 4, 7, 9, 11
F, V = [D2, D3, D4], [D2, M0, COUNT, M4]
t.predpack(F, sliced=True)
t.predpack(V, sliced=True)
FL, F2 = capi.PLAN_NO_JIT, capi.PLAN2_PLANE_AGG


def c3_with(k):
    return [("rel", D2, capi.OP_EQ, 1), ("rel", D3, capi.OP_LT, 447 - 25 * k), ("rel", D4, capi.OP_GE, 553), ("and", 3)]


METRICS = [[M0, COUNT], [M0], [COUNT], [M4], [M0, M4], [COUNT, M4], [M0, COUNT, M4], [M4, M0]]


def shapes(K):
    yield "totals_k_literals", [AggPlan(filter=c3_with(k), groups=[], metrics=[M0, COUNT], flags=FL, flags2=F2) for k in range(K)]
    yield "by_d2_k_filters", [AggPlan(filter=c3_with(k), groups=[GroupSpec(D2)], metrics=[M0, COUNT], flags=FL, flags2=F2) for k in range(K)]
    yield "totals_k_metrics", [AggPlan(filter=[], groups=[], metrics=METRICS[k], flags=FL, flags2=F2) for k in range(K)]


def fused(plans):
    t0 = time.perf_counter()
    res, info = t.query_agg_batch(plans, copy=False)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, info.fused_kernel_ms, res, info


def sequential(plans):
    t0 = time.perf_counter()
    res = [t.query_agg(p, copy=False) for p in plans]
    wall = (time.perf_counter() - t0) * 1e3
    return wall, sum(r.scan_kernel_ms for r in res), res, None


def stat(v):
    return {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)}


status, table = 0, []
for K in (2, 4, 8):
    for name, plans in shapes(K):
        for _ in range(3):
            fused(plans)
            sequential(plans)
        va, vb = t.query_agg_batch(plans)[0], [t.query_agg(p) for p in plans]      # (private copies: a view outlives only the next query of its context)
        same = all((a.ngroups, a.passed_recs, a.path, [int(x) for s in a.states for x in s]) == (b.ngroups, b.passed_recs, b.path, [int(x) for s in b.states for x in s])
                   for a, b in zip(va, vb))
        wall, kern, last = {"fused": [], "sequential": []}, {"fused": [], "sequential": []}, {}
        for _ in range(rounds):
            for leg, run in (("fused", fused), ("sequential", sequential)):
                ws, ks = [], []
                for _ in range(5):
                    wl, kn, res, info = run(plans)
                    ws.append(wl)
                    ks.append(kn)
                wall[leg].append(sorted(ws)[2])
                kern[leg].append(sorted(ks)[2])
                last[leg] = (res, info)
        (fr, fi), (sr, _) = last["fused"], last["sequential"]
        all_fused = fi.fused_groups == 1 and fi.fused_members == K and all(r.batch_fused for r in fr) and all(r.plane_agg and not r.batch_fused for r in sr)
        same = same and all((a.ngroups, a.passed_recs) == (b.ngroups, b.passed_recs) for a, b in zip(fr, sr))
        sw, sk = {l: stat(v) for l, v in wall.items()}, {l: stat(v) for l, v in kern.items()}
        rw = round(sw["sequential"]["min"] / max(sw["fused"]["min"], 1e-9), 2)
        rk = round(sk["sequential"]["min"] / max(sk["fused"]["min"], 1e-9), 2)
        print(json.dumps({"shape": name, "K": K, "segments": seg, "all_fused": all_fused, "legs_agree": same, "passed_recs": [r.passed_recs for r in fr],
                          "wall_ms": sw, "kernel_ms": sk, "wall_ratio_sequential_over_fused": rw, "kernel_ratio_sequential_over_fused": rk,
                          "kernel": fr[0].kernel}), flush=True)
        table.append((name, K, sw, sk, rw, rk))
        if not (all_fused and same):
            status = 1
print("\n| shape | K | fused wall (min / median / max ms) | sequential wall | wall ratio | fused kernel | sum of sequential kernels | kernel ratio |")
print("|---|---|---|---|---|---|---|---|")
cell = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"
for name, K, sw, sk, rw, rk in table:
    print(f"| {name} | {K} | {cell(sw['fused'])} | {cell(sw['sequential'])} | {rw} | {cell(sk['fused'])} | {cell(sk['sequential'])} | {rk} |")
t.close()
sys.exit(status)
