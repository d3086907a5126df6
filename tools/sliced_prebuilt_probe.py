#!/usr/bin/env python3
"""What the pre-built aggregate scan over the bit-sliced predicate planes (VH_PLAN_SLICED_PREBUILT: scan_agg_sliced_kernel) gains or loses
against the pre-built kernels on the 4-byte arenas, A/B inside ONE process and on one table (boxes and processes differ by more than the
variants do). C3 is generated on the device (vh_segment_generate), 125 segments of 1 M rows as tools/scale_proxy.py uses; the bit-sliced
projection of the filter's columns is built once; then three shapes are timed with and without the flag, rounds interleaved, after a warm-up:
  1. C3's own query under VH_PLAN_NO_JIT | VH_PLAN_NO_LANES          (the partitioned dense organisation)
  2. the same query GROUP BY d2                                      (the LDS table)
  3. the same query with VH_PLAN_FORCE_HASH                          (the hash table)
The leg without the flag runs code the flag does not touch. Both legs must return the same ngroups and passed_recs. One JSON line per shape:
scan_kernel_ms of both legs (min and median over the rounds, each round the median of 5 queries) and the ratio arenas / planes (> 1: the
planes are faster). usage: sliced_prebuilt_probe.py [segments] [rounds]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, seg)
p = w.plan
t.predpack(t.filter_columns(p), sliced=True)
BASE = capi.PLAN_NO_JIT | capi.PLAN_NO_LANES
shapes = [("c3", p.groups, BASE, p.groups_hint), ("c3_by_d2", [GroupSpec(2)], BASE, 0), ("c3_force_hash", p.groups, BASE | capi.PLAN_FORCE_HASH, p.groups_hint)]
status = 0
for name, groups, flags, hint in shapes:
    legs = {"arenas": AggPlan(filter=p.filter, groups=groups, metrics=p.metrics, groups_hint=hint, flags=flags),
            "planes": AggPlan(filter=p.filter, groups=groups, metrics=p.metrics, groups_hint=hint, flags=flags | capi.PLAN_SLICED_PREBUILT)}
    for plan in legs.values():
        t.prepare(plan)
        for _ in range(3):
            t.query_agg(plan, copy=False)
    ms = {n: [] for n in legs}
    wall = {n: [] for n in legs}
    last = {}
    for _ in range(rounds):
        for n, plan in legs.items():
            k = []
            t0 = time.perf_counter()
            for _ in range(5):
                r = t.query_agg(plan, copy=False)
                k.append(r.scan_kernel_ms)
            wall[n].append((time.perf_counter() - t0) / 5 * 1e3)
            ms[n].append(sorted(k)[2])
            last[n] = r
    a, b = last["arenas"], last["planes"]
    same = (a.ngroups, a.passed_recs, a.path) == (b.ngroups, b.passed_recs, b.path)
    on = b.sliced_prebuilt and not a.sliced_prebuilt
    med = {n: sorted(ms[n])[len(ms[n]) // 2] for n in legs}
    print(json.dumps({"shape": name, "segments": seg, "path": b.path, "ngroups": b.ngroups, "passed_recs": b.passed_recs, "legs_agree": same, "planes_read": on,
                      "arenas_ms": {"min": round(min(ms["arenas"]), 4), "median": round(med["arenas"], 4), "per_query": round(sorted(wall["arenas"])[rounds // 2], 4)},
                      "planes_ms": {"min": round(min(ms["planes"]), 4), "median": round(med["planes"], 4), "per_query": round(sorted(wall["planes"])[rounds // 2], 4)},
                      "ratio_min": round(min(ms["arenas"]) / max(min(ms["planes"]), 1e-9), 3), "ratio_median": round(med["arenas"] / max(med["planes"], 1e-9), 3),
                      "arenas_leg": {"kernel": a.kernel, "narrow": a.narrow, "packed": a.packed}, "planes_leg": {"kernel": b.kernel, "narrow": b.narrow, "packed": b.packed}}), flush=True)
    if not (same and on):
        status = 1
t.close()
sys.exit(status)
