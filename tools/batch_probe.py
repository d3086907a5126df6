#!/usr/bin/env python3
"""What a fused batch (vh_query_agg_batch: scan_agg_planes_batch_kernel) gains or loses against the same plans asked one by one, and what the
sharing of pass masks inside a fused launch (vh_batch.h: vh_batch_share) gains on top, A/B inside ONE process and on one table (boxes and
processes differ by more than the variants do). C3 is generated on the device (vh_segment_generate), 125 segments of 1 M rows, m4 drawn from
50 000 values so that V fits 32 planes; F = [d2, d3, d4] and V = [d2, m0, count, m4] are built explicitly. Batches of K = 2, 4 and 8 in four
shapes, all under VH_PLAN_NO_JIT | VH_PLAN2_PLANE_AGG:
  1. totals_k_literals      K totals, SUM(m0) + COUNT, under C3's filter with K different literals for d3 (K mask classes)
  2. by_d2_k_filters        K GROUP BY d2 under the same K filters (K mask classes)
  3. totals_k_metrics       K totals without a filter over K different selections of V's metrics (one mask class: equal snapshots)
  4. breakdowns_one_filter  K different breakdowns — totals and GROUP BY d2 over K selections of V's metrics — under C3's ONE filter
                            d2 == 1 & d3 < 447 & d4 >= 553 (one mask class: the dashboard's shape)
Each batch is measured three ways, rounds interleaved after a warm-up, each round the median of 5:
  a. fused       one vh_query_agg_batch call, as shipped
  b. noshare     the same call under VH_TEST_NO_BATCH_SHARE=1: the fused launch with every member evaluating its own mask
  c. sequential  K vh_query_agg calls of the same plans (the path every caller has without the batch entry point)
and two figures each: wall time of the batch (host clock around the calls, results delivered) and kernel time — fused_kernel_ms against the sum
of the K scan_kernel_ms. The members of a and b must all be fused, all three legs must return the same rows, and mask_classes must be what
the shape says: as listed above for a, K for b. One JSON line per (shape, K) with min / median / max over the rounds, the ratios c / a and
b / a of the minima (> 1: a is faster) and whether a's kernel-time range lies wholly below b's; then the same as a Markdown table.
usage: batch_probe.py [segments] [rounds] [shape ...]"""
import json, os, sys, time
os.environ["VH_TEST_HOOKS"] = "1"      # (read once when the library loads: VH_TEST_NO_BATCH_SHARE is then read per call)
os.environ.pop("VH_TEST_NO_BATCH_SHARE", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    yield "breakdowns_one_filter", [AggPlan(filter=c3_with(0), groups=[GroupSpec(D2)] if k % 2 else [], metrics=METRICS[k], flags=FL, flags2=F2) for k in range(K)]


CLASSES = {"totals_k_literals": lambda K: K, "by_d2_k_filters": lambda K: K, "totals_k_metrics": lambda K: 1, "breakdowns_one_filter": lambda K: 1}


def fused(plans):
    t0 = time.perf_counter()
    res, info = t.query_agg_batch(plans, copy=False)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, info.fused_kernel_ms, res, info


def noshare(plans):
    os.environ["VH_TEST_NO_BATCH_SHARE"] = "1"
    try:
        return fused(plans)
    finally:
        del os.environ["VH_TEST_NO_BATCH_SHARE"]


def rows(r):
    return (r.ngroups, r.passed_recs, r.path, [int(x) for k in r.keys for x in k], [int(x) for s in r.states for x in s])


def sequential(plans):
    t0 = time.perf_counter()
    res = [t.query_agg(p, copy=False) for p in plans]
    wall = (time.perf_counter() - t0) * 1e3
    return wall, sum(r.scan_kernel_ms for r in res), res, None


def stat(v):
    return {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)}


status, table = 0, []
LEGS = (("fused", fused), ("noshare", noshare), ("sequential", sequential))
for K in (2, 4, 8):
    for name, plans in shapes(K):
        if only and name not in only:
            continue
        for _ in range(3):
            for _, run in LEGS:
                run(plans)
        # (private copies: a view outlives only the next query of its context)
        os.environ["VH_TEST_NO_BATCH_SHARE"] = "1"
        vn = t.query_agg_batch(plans)[0]
        del os.environ["VH_TEST_NO_BATCH_SHARE"]
        va, vb = t.query_agg_batch(plans)[0], [t.query_agg(p) for p in plans]
        same = all(rows(a) == rows(b) == rows(c) for a, b, c in zip(va, vb, vn))
        classes = ([r.batch_member.mask_classes for r in va], [r.batch_member.mask_classes for r in vn])
        classes_ok = classes == ([CLASSES[name](K)] * K, [K] * K) and [r.batch_member.mask_of for r in vn] == list(range(K))
        wall, kern, last = {l: [] for l, _ in LEGS}, {l: [] for l, _ in LEGS}, {}
        for _ in range(rounds):
            for leg, run in LEGS:
                ws, ks = [], []
                for _ in range(5):
                    wl, kn, res, info = run(plans)
                    ws.append(wl)
                    ks.append(kn)
                wall[leg].append(sorted(ws)[2])
                kern[leg].append(sorted(ks)[2])
                last[leg] = (res, info)
        (fr, fi), (nr, ni), (sr, _) = last["fused"], last["noshare"], last["sequential"]
        all_fused = all(i.fused_groups == 1 and i.fused_members == K and all(r.batch_fused for r in rs) for rs, i in ((fr, fi), (nr, ni))) and \
            all(r.plane_agg and not r.batch_fused for r in sr)
        same = same and all((a.ngroups, a.passed_recs) == (b.ngroups, b.passed_recs) == (c.ngroups, c.passed_recs) for a, b, c in zip(fr, sr, nr))
        sw, sk = {l: stat(v) for l, v in wall.items()}, {l: stat(v) for l, v in kern.items()}
        ratio = lambda s, a, b: round(s[a]["min"] / max(s[b]["min"], 1e-9), 2)
        rw, rk, nw, nk = ratio(sw, "sequential", "fused"), ratio(sk, "sequential", "fused"), ratio(sw, "noshare", "fused"), ratio(sk, "noshare", "fused")
        below = sk["fused"]["max"] < sk["noshare"]["min"]
        print(json.dumps({"shape": name, "K": K, "segments": seg, "all_fused": all_fused, "legs_agree": same, "mask_classes": classes[0][0], "mask_classes_noshare": classes[1][0],
                          "mask_classes_ok": classes_ok, "passed_recs": [r.passed_recs for r in fr],
                          "wall_ms": sw, "kernel_ms": sk, "wall_ratio_sequential_over_fused": rw, "kernel_ratio_sequential_over_fused": rk,
                          "wall_ratio_noshare_over_fused": nw, "kernel_ratio_noshare_over_fused": nk, "fused_kernel_range_below_noshare": below,
                          "kernel": fr[0].kernel}), flush=True)
        table.append((name, K, sw, sk, rw, rk, nw, nk, below))
        if not (all_fused and same and classes_ok):
            status = 1
print("\n| shape | K | fused wall (min / median / max ms) | noshare wall | sequential wall | wall seq / fused | wall noshare / fused | fused kernel | noshare kernel | sum of sequential kernels | kernel seq / fused | kernel noshare / fused | fused range below noshare |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
cell = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"
for name, K, sw, sk, rw, rk, nw, nk, below in table:
    print(f"| {name} | {K} | {cell(sw['fused'])} | {cell(sw['noshare'])} | {cell(sw['sequential'])} | {rw} | {nw} | {cell(sk['fused'])} | {cell(sk['noshare'])} | {cell(sk['sequential'])} | {rk} | {nk} | {'yes' if below else 'no'} |")
t.close()
sys.exit(status)
