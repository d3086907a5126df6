#!/usr/bin/env python3
"""What the aggregate on the bit-sliced planes gains or loses when its kernel is COMPILED for the plan's shape (VH_PLAN2_PLANE_JIT), three legs
inside ONE process and on one table (boxes and processes differ by more than the legs do). C3 is generated on the device
(vh_segment_generate), 125 segments of 1 M rows, with a thirteenth column d6 of 16 values so that (d6, d2) is a 64-id GROUP BY; F = [d2, d3,
d4], V = [d0, d1, d2, m0, count] (31 planes) and W = [d6, d2, m0, count] are built explicitly. SUM(m0) + COUNT throughout. Per shape:
  (A) the plan with VH_PLAN2_PLANE_JIT (+ VH_PLAN2_PLANE_ROWS beyond 64 ids): the compiled plane aggregate;
  (B) VH_PLAN_NO_JIT + VH_PLAN2_PLANE_AGG (+ _ROWS): the pre-built plane kernel it is the compiled form of;
  (C) no flag at all: what the library does today for that plan, the compiled scan over rows.
B and C are the library's behaviour without the flag, measured in the same process. The three legs must return the same groups and passed
rows. Rounds are interleaved after a warm-up, a round's figure is the median of 5 queries, at least 7 rounds; scan_kernel_ms as min / median
/ max, ratios of the minima (> 1: A is faster). compile_ms is the build worker's own time for leg A's kernel, taken once per shape on the
table in background build mode with the disk cache off. The limit that ends a hung run is the CALLER's: run the probe under `timeout -k 10
<seconds>` — a query stuck inside the library never gives the interpreter control back. The per-shape SIGALRM here only catches a shape
that is slow between queries (status 3), so that a slow run says which shape it was.
usage: plane_jit_probe.py [segments] [rounds]"""
import json, os, signal, sys
os.environ["VH_JIT_NO_DISK_CACHE"] = "1"      # (read once: every kernel of this process is compiled here, so compile_ms is a compile's)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan, GroupSpec
seg = int(sys.argv[1]) if len(sys.argv) > 1 else 125
rounds = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
SHAPE_LIMIT_S = 100
executor.init(0)
w = synth.c3()
w.columns.append(synth._dim("d6", 16))
t = synth.create_device_table(w, seg)
D0, D1, D2, D3, D4, M0, COUNT, D6 = 0, 1, 2, 3, 4, 7, 9, 12
for cols in ([D2, D3, D4], [D0, D1, D2, M0, COUNT], [D6, D2, M0, COUNT]):
    t.predpack(cols, sliced=True)
NOJ, AGG, ROWS, JIT = capi.PLAN_NO_JIT, capi.PLAN2_PLANE_AGG, capi.PLAN2_PLANE_ROWS, capi.PLAN2_PLANE_JIT
C3 = list(w.plan.filter)
EVERY = [("rel", D3, capi.OP_NE, 1023)]
SHAPES = [("totals/no_filter", [], [], 0), ("totals/c3_5pct", C3, [], 0), ("by_d2/c3_5pct", C3, [D2], 0), ("by_d2/every_row", EVERY, [D2], 0),
          ("by_d6_d2_64ids/c3_5pct", C3, [D6, D2], 0), ("by_d1_100ids_rows/c3_5pct", C3, [D1], ROWS), ("by_d1_100ids_rows/every_row", EVERY, [D1], ROWS)]
status = 0


def overrun(signum, frame):
    print(json.dumps({"error": "a shape ran beyond its time limit", "limit_s": SHAPE_LIMIT_S}), flush=True)
    os._exit(3)


signal.signal(signal.SIGALRM, overrun)


def stat(v):
    return {"min": round(min(v), 4), "median": round(sorted(v)[len(v) // 2], 4), "max": round(max(v), 4)}


def measure(legs):
    for p in legs.values():
        for _ in range(3):
            t.query_agg(p, copy=False)
    ms, last = {n: [] for n in legs}, {}
    for _ in range(rounds):
        for n, p in legs.items():
            k = []
            for _ in range(5):
                last[n] = t.query_agg(p, copy=False)
                k.append(last[n].scan_kernel_ms)
            ms[n].append(sorted(k)[2])
    return {n: stat(v) for n, v in ms.items()}, last


rows_out = []
for name, flt, dims, rows2 in SHAPES:
    signal.alarm(SHAPE_LIMIT_S)
    legs = {"A": AggPlan(filter=flt, groups=[GroupSpec(d) for d in dims], metrics=[M0, COUNT], flags=0, flags2=JIT | rows2),
            "B": AggPlan(filter=flt, groups=[GroupSpec(d) for d in dims], metrics=[M0, COUNT], flags=NOJ, flags2=AGG | rows2),
            "C": AggPlan(filter=flt, groups=[GroupSpec(d) for d in dims], metrics=[M0, COUNT], flags=0, flags2=0)}
    # leg A's kernel, compiled by the build worker: its own time for it
    t.set_build_mode(True)
    before = t.build_info().compile_ms
    first = t.query_agg(legs["A"], copy=False)
    compile_ms = round(t.build_wait(120000).compile_ms - before, 1)
    t.set_build_mode(False)
    st, last = measure(legs)
    a, b, c = last["A"], last["B"], last["C"]
    same = len({(r.ngroups, r.passed_recs) for r in (a, b, c)}) == 1
    expected = a.plane_agg and a.jit and b.plane_agg and not b.jit and not c.plane_agg and a.plane_sink == b.plane_sink == (2 if rows2 else 1)
    spread_b = round(st["B"]["max"] - st["B"]["min"], 4)
    rec = {"shape": name, "segments": seg, "ngroups": a.ngroups, "passed_recs": a.passed_recs, "legs_agree": same, "as_expected": bool(expected),
           "pending_first": bool(first.flags & capi.INFO_BUILD_PENDING), "compile_ms": compile_ms, "kernel_ms": st,
           "B_over_A": round(st["B"]["min"] / max(st["A"]["min"], 1e-9), 2), "C_over_A": round(st["C"]["min"] / max(st["A"]["min"], 1e-9), 2),
           "B_spread_ms": spread_b, "A_slower_than_B_beyond_its_spread": bool(st["A"]["min"] - st["B"]["min"] > spread_b),
           "kernel": {n: r.kernel for n, r in last.items()}}
    print(json.dumps(rec), flush=True)
    if not (same and expected):
        status = 1
    rows_out.append(rec)
    signal.alarm(0)
cell = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"
print("\n| shape | passed rows | groups | A compiled plane aggregate (min / median / max ms) | B pre-built plane kernel | C compiled scan | B / A | C / A | compile ms |")
print("|---|---|---|---|---|---|---|---|---|")
for r in rows_out:
    k = r["kernel_ms"]
    print(f"| {r['shape']} | {r['passed_recs']} | {r['ngroups']} | {cell(k['A'])} | {cell(k['B'])} | {cell(k['C'])} | {r['B_over_A']} | {r['C_over_A']} | {r['compile_ms']} |")
t.close()
sys.exit(status)
