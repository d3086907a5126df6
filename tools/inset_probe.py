"""A long IN list four ways, one process, one table: C3's table and plan with the leaf on d3 (`d3 < 447`) replaced by
`d3 IN (N values)`, N in {8, 32, 33, 64, 600} and a dense set (every value the column holds: no empty word in the 10-bit truth table), run
  * as VH_F_IN (what the library did before set leaves existed; bit-serial up to 32 literals, the interpreting kernel beyond),
  * as a set leaf looked up per row in bitmap form and in sorted-array form (VH_PLAN_SET_SEARCH), both under VH_PLAN_NO_SLICED: byte planes,
    the path a set plan took before it could read bit planes,
  * as a set leaf evaluated from its truth table on the bit-sliced planes.
Every leg runs under VH_PLAN_NO_GROUPED (no grouped records, no clustered planes), so the legs differ in the leaf only; both predicate
projections are built up front. Per leg: warm-up queries, then the median kernel and wall time of up to 20 queries (fewer when a query
takes long: 5 at least, ~4 s per leg). One JSON line per leg, also written to `out`.
With `clustered` as the third argument: C3 itself and C3 with d3 as a 300-member set, both through the clustered planes (vh_table_prepare
builds them), nothing else.
usage: python tools/inset_probe.py [segments=200] [out=profiles/r12/inset.json] [clustered]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r12", "inset.json")
clustered = len(sys.argv) > 3 and sys.argv[3] == "clustered"
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
lines = []


def leg(n, label, flt, flags):
    plan = t.prepare(AggPlan(filter=flt, groups=w.plan.groups, metrics=w.plan.metrics, flags=flags, groups_hint=w.plan.groups_hint))
    for _ in range(5):
        r = t.query_agg(plan, copy=False)
    ks, ws, t0 = [], [], time.perf_counter()
    while len(ks) < 20 and (len(ks) < 5 or time.perf_counter() - t0 < 4.0):
        q0 = time.perf_counter(); r = t.query_agg(plan, copy=False); ws.append((time.perf_counter() - q0) * 1e3); ks.append(r.scan_kernel_ms)
    ks, ws = sorted(ks), sorted(ws)
    lines.append({"n": n, "leg": label, "rows": nseg * w.segment_rows, "kernel_ms": round(ks[len(ks) // 2], 4), "kernel_ms_min": round(ks[0], 4), "wall_ms": round(ws[len(ws) // 2], 4),
                  "queries": len(ks), "passed": r.passed_recs, "ngroups": r.ngroups, "jit": r.jit, "predpack": r.predpack, "sliced": r.sliced, "packed": r.packed,
                  "grouped_planes": r.grouped_planes, "inset": r.inset, "inset_search": r.inset_search, "inset_sliced": r.inset_sliced, "path": r.path, "kernel": r.kernel})
    print(json.dumps(lines[-1]), flush=True)


if clustered:
    leg(0, "c3_clustered", list(w.plan.filter), 0)
    leg(300, "set_clustered", [w.plan.filter[0], ("inset", 3, True, [(k * 1000) // 300 for k in range(300)]), w.plan.filter[2], ("and", 3)], 0)
    assert lines[-1]["grouped_planes"] and lines[-1]["inset_sliced"] and lines[-2]["grouped_planes"], lines[-2:]
else:
    t.predpack([2, 3, 4], sliced=False)
    t.predpack([2, 3, 4], sliced=True)
    G, S = capi.PLAN_NO_GROUPED, capi.PLAN_NO_SLICED
    for n in (8, 32, 33, 64, 600, 1000):
        members = [(k * 1000) // n for k in range(n)]          # spread over d3's 1000 values: n / 1000 of the rows pass this leaf
        for label, kind, flags in (("in", "in", G), ("set_bitmap", "inset", G | S), ("set_array", "inset", G | S | capi.PLAN_SET_SEARCH), ("set_sliced", "inset", G)):
            leg(n, label, [w.plan.filter[0], (kind, 3, True, members), w.plan.filter[2], ("and", 3)], flags)
        assert len({l["passed"] for l in lines[-4:]}) == 1 and len({l["ngroups"] for l in lines[-4:]}) == 1, lines[-4:]      # the four legs answer alike
        assert lines[-1]["inset_sliced"] and not lines[-2]["inset_sliced"] and not lines[-3]["inset_sliced"], lines[-3:]
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for l in lines:
        f.write(json.dumps(l) + "\n")
