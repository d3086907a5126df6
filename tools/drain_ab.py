"""C3 at bench size, one process, one prepared table: the compiled scan's pipelined drain (survivor records in flight while the previous
group is sunk) against the same plan with VH_TEST_DRAIN_DEPTH=0 (one drain after another), alternating, `rounds` times; per leg and
round the median, min and max of the kernel time (scan + phase 2) of 20 queries. The legs must have run different code objects (the
kernel's name carries the shape's hash, and the depth is part of the shape): anything else is an error.
A second test knob can be swept the same way (the resident-block cap: `VH_TEST_BLOCKS_PER_CU 3,4,5`; the wave scans as shuffles:
`VH_JIT_FLAGS -DVH_WAVE_SCAN_SHFL=1,default`; the clustered scan's tile groups kept inside a segment: `VH_TEST_NO_GPSPAN 1,default`; longer
units: `VH_TEST_UNIT_ROWS 32768,131072,262144`); "default" leaves the knob unset.
usage: python tools/drain_ab.py [segments=1000] [rounds=3] [knob=VH_TEST_DRAIN_DEPTH] [values=0,default]"""
import json, os, sys, time
os.environ["VH_TEST_HOOKS"] = "1"            # the gate in front of the library's test hooks (viya_hip.hip test_env)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
knob = sys.argv[3] if len(sys.argv) > 3 else "VH_TEST_DRAIN_DEPTH"
values = (sys.argv[4] if len(sys.argv) > 4 else "0,default").split(",")
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
plan = AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, flags=0, groups_hint=w.plan.groups_hint)
flags = t.warm(plan)
print(json.dumps({"prepared": hex(flags), "grouped_payload": bool(flags & capi.INFO_GROUPED_PAYLOAD), "grouped_planes": bool(flags & capi.INFO_GROUPED_PLANES)}), flush=True)
kernels, med = {}, {v: [] for v in values}
for rnd in range(rounds):
    for v in values:
        if v == "default": os.environ.pop(knob, None)
        else: os.environ[knob] = v
        p = t.prepare(plan)
        ks, ws = [], []
        for i in range(25):
            q0 = time.perf_counter(); r = t.query_agg(p, copy=False); ws.append((time.perf_counter() - q0) * 1e3); ks.append(r.scan_kernel_ms)
        ks, ws = sorted(ks[5:]), sorted(ws[5:])
        kernels[v] = r.kernel
        med[v].append(ks[len(ks) // 2])
        print(json.dumps({"round": rnd, knob: v, "kernel_ms": round(ks[len(ks) // 2], 4), "kernel_ms_min": round(ks[0], 4), "kernel_ms_max": round(ks[-1], 4),
                          "spread": round(ks[-1] - ks[0], 4), "wall_ms": round(ws[len(ws) // 2], 4), "wall_ms_min": round(ws[0], 4), "wall_ms_max": round(ws[-1], 4), "passed": r.passed_recs, "ngroups": r.ngroups, "kernel": r.kernel}), flush=True)
os.environ.pop(knob, None)
print(json.dumps({"knob": knob, "kernels": kernels, "median_ms": {v: [round(x, 4) for x in med[v]] for v in values}}), flush=True)
if knob == "VH_TEST_DRAIN_DEPTH" and len(set(kernels.values())) != len(values):
    raise SystemExit("the legs ran the same code object: %r" % (kernels,))
