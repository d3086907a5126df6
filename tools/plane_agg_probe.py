#!/usr/bin/env python3
"""What the aggregate ON the bit-sliced planes (VH_PLAN2_PLANE_AGG: scan_agg_planes_kernel) gains or loses, A/B inside ONE process and on one
table (boxes and processes differ by more than the variants do). C3 is generated on the device (vh_segment_generate), 125 segments of 1 M
rows, with d1 drawn from 16 values instead of 100 so that (d1, d2) is a 64-id GROUP BY; F = [d2, d3, d4] and V = [d1, d2, m0, count] are
built explicitly. Five shapes, SUM(m0) + COUNT each:
  1. scalar, no filter            2. scalar, C3's filter          3. GROUP BY d2, C3's filter (5 % pass)
  4. GROUP BY d2, every row passes (d3 != 1023)                   5. GROUP BY (d1, d2), 64 ids, C3's filter
in four configurations, rounds interleaved after a warm-up:
  a. VH_PLAN_NO_JIT with VH_PLAN2_PLANE_AGG        b. VH_PLAN_NO_JIT alone: the pre-built kernels the path stands in for
  c. the default path, compiled kernels allowed    d. VH_PLAN_NO_JIT with VH_PLAN_SLICED_PREBUILT
All four must return the same ngroups and passed_recs. One JSON line per shape: scan_kernel_ms of every configuration (min, median and max
over the rounds, each round the median of 5 queries), the ratios b / a, c / a and d / a of the minima (> 1: the planes are faster), the kernels
that ran and the bits per row of the planes configuration a reads. Then the same as a Markdown table.
usage: plane_agg_probe.py [segments] [rounds]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
executor.init(0)
w = synth.c3()
w.columns[1] = synth._dim("d1", 16)
t = synth.create_device_table(w, seg)
D1, D2, D3, D4, M0, COUNT = 1, 2, 3, 4, 7, 9
F, V = [D2, D3, D4], [D1, D2, M0, COUNT]
t.predpack(F, sliced=True)
t.predpack(V, sliced=True)
bits = {c: (w.columns[c].gen[1] + w.columns[c].gen[2] - 1).bit_length() for c in set(F + V)}      # values are add .. add + mod - 1
c3 = list(w.plan.filter)
every = [("rel", D3, capi.OP_NE, 1023)]
shapes = [("scalar_no_filter", [], [], []), ("scalar_c3", c3, [], F), ("by_d2_5pct", c3, [D2], F), ("by_d2_100pct", every, [D2], F),
          ("by_d1_d2_64ids", c3, [D1, D2], F)]
NOJ = capi.PLAN_NO_JIT
configs = [("a_planes", NOJ, capi.PLAN2_PLANE_AGG), ("b_prebuilt", NOJ, 0), ("c_default", 0, 0), ("d_sliced_prebuilt", NOJ | capi.PLAN_SLICED_PREBUILT, 0)]
status, table = 0, []
for name, flt, dims, fcols in shapes:
    legs = {c: AggPlan(filter=flt, groups=[GroupSpec(d) for d in dims], metrics=[M0, COUNT], flags=fl, flags2=f2) for c, fl, f2 in configs}
    for plan in legs.values():
        for _ in range(3):
            t.query_agg(plan, copy=False)
    ms, last = {n: [] for n in legs}, {}
    for _ in range(rounds):
        for n, plan in legs.items():
            k = []
            for _ in range(5):
                r = t.query_agg(plan, copy=False)
                k.append(r.scan_kernel_ms)
            ms[n].append(sorted(k)[2])
            last[n] = r
    a = last["a_planes"]
    same = all((r.ngroups, r.passed_recs, r.path) == (a.ngroups, a.passed_recs, a.path) for r in last.values())
    on = a.plane_agg and not any(r.plane_agg for n, r in last.items() if n != "a_planes")
    stat = {n: {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)} for n, v in ms.items()}
    ratio = {n: round(stat[n]["min"] / max(stat["a_planes"]["min"], 1e-9), 2) for n in legs if n != "a_planes"}
    plane_bits = sum(bits[c] for c in fcols) + sum(bits[c] for c in dims + [M0, COUNT])
    print(json.dumps({"shape": name, "segments": seg, "path": a.path, "ngroups": a.ngroups, "passed_recs": a.passed_recs, "legs_agree": same, "on_planes": on,
                      "plane_bits_per_row": plane_bits, "scan_kernel_ms": stat, "ratio_of_min_to_a": ratio, "kernel": {n: r.kernel for n, r in last.items()}}), flush=True)
    table.append((name, a.passed_recs, plane_bits, stat, ratio))
    if not (same and on):
        status = 1
print("\n| shape | passed rows | plane bits / row | a: on the planes (min / median / max ms) | b: pre-built | c: default | d: sliced pre-built | b / a | c / a | d / a |")
print("|---|---|---|---|---|---|---|---|---|---|")
for name, passed, pb, stat, ratio in table:
    cell = lambda n: f"{stat[n]['min']:.3f} / {stat[n]['median']:.3f} / {stat[n]['max']:.3f}"
    print(f"| {name} | {passed} | {pb} | {cell('a_planes')} | {cell('b_prebuilt')} | {cell('c_default')} | {cell('d_sliced_prebuilt')} | "
          f"{ratio['b_prebuilt']} | {ratio['c_default']} | {ratio['d_sliced_prebuilt']} |")
t.close()
sys.exit(status)
