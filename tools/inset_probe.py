"""A long IN list three ways, one process, one table: C3's table and plan with the leaf on d3 (`d3 < 447`) replaced by
`d3 IN (N values)`, N in {8, 32, 33, 64, 600}, run as VH_F_IN (unchanged code: what the library did before set leaves existed), as a set
leaf in bitmap form and as a set leaf in sorted-array form (VH_PLAN_SET_SEARCH). Per leg: warm-up queries (the third builds the automatic
layouts of the shape), then the median kernel and wall time of up to 20 queries (fewer when a query takes long: 5 at least, ~4 s per leg).
One JSON line per leg, also appended to `out`.
usage: python tools/inset_probe.py [segments=200] [out=profiles/r07/inset.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07", "inset.json")
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
lines = []
for n in (8, 32, 33, 64, 600):
    members = [(k * 1000) // n for k in range(n)]          # spread over d3's 1000 values: n / 1000 of the rows pass this leaf
    for label, kind, flags in (("in", "in", 0), ("set_bitmap", "inset", 0), ("set_array", "inset", capi.PLAN_SET_SEARCH)):
        flt = [w.plan.filter[0], (kind, 3, True, members), w.plan.filter[2], ("and", 3)]
        plan = t.prepare(AggPlan(filter=flt, groups=w.plan.groups, metrics=w.plan.metrics, flags=flags, groups_hint=w.plan.groups_hint))
        for _ in range(5):
            r = t.query_agg(plan, copy=False)
        ks, ws, t0 = [], [], time.perf_counter()
        while len(ks) < 20 and (len(ks) < 5 or time.perf_counter() - t0 < 4.0):
            q0 = time.perf_counter(); r = t.query_agg(plan, copy=False); ws.append((time.perf_counter() - q0) * 1e3); ks.append(r.scan_kernel_ms)
        ks, ws = sorted(ks), sorted(ws)
        lines.append({"n": n, "leg": label, "rows": nseg * w.segment_rows, "kernel_ms": round(ks[len(ks) // 2], 4), "kernel_ms_min": round(ks[0], 4), "wall_ms": round(ws[len(ws) // 2], 4),
                      "queries": len(ks), "passed": r.passed_recs, "ngroups": r.ngroups, "jit": r.jit, "predpack": r.predpack, "sliced": r.sliced, "packed": r.packed,
                      "inset": r.inset, "inset_search": r.inset_search, "path": r.path, "kernel": r.kernel})
        print(json.dumps(lines[-1]), flush=True)
    assert len({l["passed"] for l in lines[-3:]}) == 1 and len({l["ngroups"] for l in lines[-3:]}) == 1, lines[-3:]      # the three legs answer alike
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for l in lines:
        f.write(json.dumps(l) + "\n")
