"""C3 at bench size, one process, one table: the grouped form SUB-SORTED by d3 (the scan trims every run to the words that can pass
`d3 < 447`) against the form in row order inside its runs (VH_TEST_SUBSORT=0), alternating, `rounds` times. Every leg calls warm()
(vh_table_prepare), which has the form built again for the leg's order — the time of that rebuild is reported with the leg — and then times
20 queries: per leg and round the median, min and max of the kernel time (scan + phase 2). The legs must report different path bits
(vh_result_info.reserved bit 28) and the same answer: anything else is an error.
usage: python tools/subsort_ab.py [segments=1000] [rounds=3] [values=0,default]"""
import json, os, sys, time
os.environ["VH_TEST_HOOKS"] = "1"            # the gate in front of the library's test hooks (viya_hip.hip test_env)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
from viyadb_amd.executor import AggPlan
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
values = (sys.argv[3] if len(sys.argv) > 3 else "0,default").split(",")
knob = "VH_TEST_SUBSORT"
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
plan = AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, flags=0, groups_hint=w.plan.groups_hint)
trimmed, answers, med = {}, {}, {v: [] for v in values}
for rnd in range(rounds):
    for v in values:
        if v == "default": os.environ.pop(knob, None)
        else: os.environ[knob] = v
        w0 = time.perf_counter(); flags = t.warm(plan); warm_s = time.perf_counter() - w0
        p = t.prepare(plan)
        ks, ws = [], []
        for i in range(25):
            q0 = time.perf_counter(); r = t.query_agg(p, copy=False); ws.append((time.perf_counter() - q0) * 1e3); ks.append(r.scan_kernel_ms)
        ks, ws = sorted(ks[5:]), sorted(ws[5:])
        trimmed[v] = bool(r.flags & capi.INFO_SUBTRIM)
        answers[v] = (r.passed_recs, r.ngroups)
        med[v].append(ks[len(ks) // 2])
        print(json.dumps({"round": rnd, knob: v, "warm_s": round(warm_s, 3), "prepared": hex(flags), "sub_trimmed": trimmed[v], "device_bytes": t.info()[2],
                          "kernel_ms": round(ks[len(ks) // 2], 4), "kernel_ms_min": round(ks[0], 4), "kernel_ms_max": round(ks[-1], 4), "spread": round(ks[-1] - ks[0], 4),
                          "wall_ms": round(ws[len(ws) // 2], 4), "wall_ms_min": round(ws[0], 4), "wall_ms_max": round(ws[-1], 4), "passed": r.passed_recs, "ngroups": r.ngroups, "kernel": r.kernel}), flush=True)
os.environ.pop(knob, None)
print(json.dumps({"knob": knob, "sub_trimmed": trimmed, "median_ms": {v: [round(x, 4) for x in med[v]] for v in values}}), flush=True)
if len(values) > 1 and (len(set(trimmed.values())) < 2 or len(set(answers.values())) != 1):
    raise SystemExit("the legs must differ in bit 28 and agree on the answer: %r %r" % (trimmed, answers))
