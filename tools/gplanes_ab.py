"""C3 at bench size, one process, one table: the compiled scan reading the clustered planes beside the grouped records against the same plan
with VH_PLAN_NO_GPLANES (row-order bit planes over the grouped records), alternating, `rounds` times; per variant and round the median kernel
and wall time of 20 queries.
usage: python tools/gplanes_ab.py [segments=1000] [rounds=5]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
mk = lambda flags: AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, flags=flags, groups_hint=w.plan.groups_hint)
flags = t.warm(mk(0))
print(json.dumps({"prepared": hex(flags), "grouped_payload": bool(flags & capi.INFO_GROUPED_PAYLOAD), "grouped_planes": bool(flags & capi.INFO_GROUPED_PLANES)}), flush=True)
for rnd in range(rounds):
    for label, f in (("clustered", 0), ("row_order_planes", capi.PLAN_NO_GPLANES)):
        plan = t.prepare(mk(f))
        ks, ws = [], []
        for i in range(25):
            q0 = time.perf_counter(); r = t.query_agg(plan, copy=False); ws.append((time.perf_counter() - q0) * 1e3); ks.append(r.scan_kernel_ms)
        ks, ws = sorted(ks[5:]), sorted(ws[5:])
        print(json.dumps({"round": rnd, "variant": label, "grouped_planes": r.grouped_planes, "kernel_ms": round(ks[len(ks) // 2], 4), "kernel_ms_min": round(ks[0], 4),
                          "kernel_ms_max": round(ks[-1], 4), "wall_ms": round(ws[len(ws) // 2], 4), "passed": r.passed_recs, "ngroups": r.ngroups, "kernel": r.kernel}), flush=True)
