#!/usr/bin/env python3
"""What the ROW SINK of the aggregate on the bit-sliced planes (VH_PLAN2_PLANE_ROWS: scan_agg_planes_rows_kernel, and a fused launch named
scan_agg_planes_batch_kernel<256, S, rows>) gains or loses, A/B inside ONE process and on one table (boxes and processes differ by more than
the variants do). C3 is generated on the device (vh_segment_generate), 125 segments of 1 M rows, with a thirteenth column d6 of 16 values so
that (d6, d2) is a 64-id GROUP BY; F = [d2, d3, d4], V = [d0, d1, d2, m0, count] (31 planes) and W = [d6, d2, m0, count] are built
explicitly. Everything runs under VH_PLAN_NO_JIT, SUM(m0) + COUNT each, rounds interleaved after a warm-up, each round the median of 5
queries, at least 7 rounds; scan_kernel_ms throughout.
  (a) single   GROUP BY d1 (100 ids), d0 (1000 ids) and (d0, d2) (4000 ids; SUM(m0) alone, so that the table fits the LDS organisation's
               40 KB), each under C3's filter (5 % pass), with every row passing
               (d3 != 1023) and with no filter: the plan with VH_PLAN2_PLANE_ROWS against the same plan without it — the pre-built kernel
               that answers it today.
  (b) sinks    GROUP BY d2 (4 ids) and (d6, d2) (64 ids) under C3's filter and with every row passing, through both sinks:
               VH_PLAN2_PLANE_ROWS under VH_TEST_PLANE_ROWS_MIN=1 (the row sink) against VH_PLAN2_PLANE_AGG (the loop over ids).
  (c) batch    K = 2 / 4 / 8 breakdowns under C3's ONE filter, member 0 GROUP BY d1 (a row member), the others totals and GROUP BY d2:
               one call with VH_PLAN2_PLANE_ROWS on every member (one fused launch, the row member in it) against one call with
               VH_PLAN2_PLANE_AGG (the row member single and off the planes, the rest fused: what the call did before the flag). Kernel
               time of a call: fused_kernel_ms plus the scan_kernel_ms of every member that was not fused.
Both legs of a comparison must return the same groups and passed rows. One JSON line per comparison with min / median / max over the rounds
and the ratio of the minima (> 1: the row sink is faster); then the same as Markdown tables.
usage: plane_rows_probe.py [segments] [rounds]"""
import json, os, sys
os.environ["VH_TEST_HOOKS"] = "1"      # (read once when the library loads: VH_TEST_PLANE_ROWS_MIN is then read per call)
os.environ.pop("VH_TEST_PLANE_ROWS_MIN", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
executor.init(0)
w = synth.c3()
w.columns.append(synth._dim("d6", 16))
t = synth.create_device_table(w, seg)
D0, D1, D2, D3, D4, M0, COUNT, D6 = 0, 1, 2, 3, 4, 7, 9, 12
for cols in ([D2, D3, D4], [D0, D1, D2, M0, COUNT], [D6, D2, M0, COUNT]):
    t.predpack(cols, sliced=True)
NOJ, AGG, ROWS = capi.PLAN_NO_JIT, capi.PLAN2_PLANE_AGG, capi.PLAN2_PLANE_ROWS
C3 = list(w.plan.filter)
FILTERS = [("c3_5pct", C3), ("every_row", [("rel", D3, capi.OP_NE, 1023)]), ("no_filter", [])]
HOOK = "VH_TEST_PLANE_ROWS_MIN"
status = 0


def plan(flt, dims, f2, metrics=(M0, COUNT)):
    return AggPlan(filter=flt, groups=[GroupSpec(d) for d in dims], metrics=list(metrics), flags=NOJ, flags2=f2)


def single(p, hook=None):
    def run():
        if hook is not None:
            os.environ[HOOK] = hook
        try:
            r = t.query_agg(p, copy=False)
        finally:
            os.environ.pop(HOOK, None)
        return r.scan_kernel_ms, [r]
    return run


def batch(plans):
    def run():
        res, info = t.query_agg_batch(plans, copy=False)
        return info.fused_kernel_ms + sum(r.scan_kernel_ms for r in res if not r.batch_fused), res
    return run


def stat(v):
    return {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)}


def measure(legs):
    """legs: {name: run}; -> {name: stat}, {name: the last round's results}"""
    for run in legs.values():
        for _ in range(3):
            run()
    ms, last = {n: [] for n in legs}, {}
    for _ in range(rounds):
        for n, run in legs.items():
            k = []
            for _ in range(5):
                v, res = run()
                k.append(v)
            ms[n].append(sorted(k)[2])
            last[n] = res
    return {n: stat(v) for n, v in ms.items()}, last


def report(part, name, st, last, checks, extra):
    global status
    a, b = last["rows"], last["base"]
    same = all((x.ngroups, x.passed_recs, x.path) == (y.ngroups, y.passed_recs, y.path) for x, y in zip(a, b))
    ratio = round(st["base"]["min"] / max(st["rows"]["min"], 1e-9), 2)
    ok = same and checks
    print(json.dumps({"part": part, "shape": name, "segments": seg, "ngroups": [r.ngroups for r in a], "passed_recs": a[0].passed_recs, "legs_agree": same, "as_expected": checks,
                      "kernel_ms": st, "ratio_base_over_rows": ratio, "kernel": {n: [r.kernel for r in rs] for n, rs in last.items()}, **extra}), flush=True)
    if not ok:
        status = 1
    return ratio


cell = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"
tab_a, tab_b, tab_c = [], [], []
# (a) single queries beyond 64 ids
# (4000 ids of SUM(m0) + COUNT are 52 KB, beyond the 40 KB of the dense LDS table: that shape sums m0 alone, 36 KB)
for dims, label, mets in (([D1], "by_d1_100ids", (M0, COUNT)), ([D0], "by_d0_1000ids", (M0, COUNT)), ([D0, D2], "by_d0_d2_4000ids_m0_alone", (M0,))):
    for fname, flt in FILTERS:
        st, last = measure({"rows": single(plan(flt, dims, ROWS, mets)), "base": single(plan(flt, dims, 0, mets))})
        r, b = last["rows"][0], last["base"][0]
        ratio = report("a", f"{label}/{fname}", st, last, r.plane_sink == 2 and b.plane_sink == 0, {})
        tab_a.append((label, fname, r.passed_recs, st, ratio, b.kernel))
# (b) the crossover: plans of at most 64 ids through both sinks
for dims, label in (([D2], "by_d2_4ids"), ([D6, D2], "by_d6_d2_64ids")):
    for fname, flt in FILTERS[:2]:
        st, last = measure({"rows": single(plan(flt, dims, ROWS), hook="1"), "base": single(plan(flt, dims, AGG))})
        r, b = last["rows"][0], last["base"][0]
        ratio = report("b", f"{label}/{fname}", st, last, r.plane_sink == 2 and b.plane_sink == 1, {})
        tab_b.append((label, fname, r.passed_recs, st, ratio))
# (c) batches with one row member
METRICS = [[M0, COUNT], [M0], [COUNT], [COUNT, M0]]
for K in (2, 4, 8):
    def members(f2):
        out = [plan(C3, [D1], f2)]
        for k in range(1, K):
            out.append(plan(C3, [D2] if k % 2 else [], f2, METRICS[(k // 2) % 4]))
        return out
    st, last = measure({"rows": batch(members(ROWS)), "base": batch(members(AGG))})
    a, b = last["rows"], last["base"]
    checks = all(r.batch_fused for r in a) and a[0].plane_sink == 2 and a[0].kernel.endswith(", rows>") and len({r.batch_member.mask_classes for r in a}) == 1 and \
        not b[0].batch_fused and b[0].plane_sink == 0 and (K == 2 or all(r.batch_fused for r in b[1:]))
    ratio = report("c", f"breakdowns_one_filter_K{K}", st, last, checks, {"K": K, "mask_classes": int(a[0].batch_member.mask_classes)})
    tab_c.append((K, st, ratio))
print("\n(a) single queries: the row sink against the same plan without the flag\n")
print("| GROUP BY | filter | passed rows | row sink (min / median / max ms) | without the flag | its kernel | without / with |")
print("|---|---|---|---|---|---|---|")
for label, fname, passed, st, ratio, kernel in tab_a:
    print(f"| {label} | {fname} | {passed} | {cell(st['rows'])} | {cell(st['base'])} | `{kernel}` | {ratio} |")
print("\n(b) both sinks on plans of at most 64 ids\n")
print("| GROUP BY | filter | passed rows | row sink (min / median / max ms) | loop over ids | loop / row sink |")
print("|---|---|---|---|---|---|")
for label, fname, passed, st, ratio in tab_b:
    print(f"| {label} | {fname} | {passed} | {cell(st['rows'])} | {cell(st['base'])} | {ratio} |")
print("\n(c) K breakdowns under one filter, one of them GROUP BY d1: kernel time of the call\n")
print("| K | all fused, row member included (min / median / max ms) | row member single, the rest fused | before / after |")
print("|---|---|---|---|")
for K, st, ratio in tab_c:
    print(f"| {K} | {cell(st['rows'])} | {cell(st['base'])} | {ratio} |")
t.close()
sys.exit(status)
