"""vh_query_select over C3's table, on the bit-sliced predicate planes and on the arenas: C3's filter (`d2 == 1 & d3 < 447 & d4 >= 553`),
selecting `id, m0`, with vh_table_predpack([d2, d3, d4], sliced) built up front. Four legs in one process: limit 0 (every passing row is
emitted) and limit 1000, each as the planner takes it (the planes, where the library reads them for a select) and under VH_PLAN_NO_SLICED
(the arenas), the two alternating query by query. Per leg: warm-up queries, then the median vh_rows_info.kernel_ms — count, scan and
emission kernels, the host's window arithmetic and the allocation of the output arrays between them included — and wall time of 20 queries. One JSON line per leg, appended to `out` under `tag`; lines of other tags
already there are kept, so a run of an older build of the library (which has no vh_rows_flags: `flags` is null there, and both of its legs
read the arenas) stands beside this one's.
usage: python tools/select_probe.py [segments=200] [out=profiles/r13/select.json] [tag=head]"""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viyadb_amd import capi, executor, synth
nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13", "select.json")
tag = sys.argv[3] if len(sys.argv) > 3 else "head"
executor.init(0)
w = synth.c3()
t = synth.create_device_table(w, nseg)
t.predpack([2, 3, 4], sliced=True)
lib = capi.load()
rows_flags = getattr(lib, "vh_rows_flags", None)      # (an older build has none)
if rows_flags is not None:
    rows_flags.restype, rows_flags.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]
cols = [w.col("id"), w.col("m0")]
lines = []


def select(sp):
    rows, info, flags = C.c_void_p(), capi.RowsInfo(), C.c_uint32()
    q0 = time.perf_counter()
    capi.check(lib.vh_query_select(t.handle, C.byref(sp), C.byref(rows)))
    wall = (time.perf_counter() - q0) * 1e3
    try:
        capi.check(lib.vh_rows_get_info(rows, C.byref(info)))
        if rows_flags is not None:
            capi.check(rows_flags(rows, C.byref(flags)))
    finally:
        lib.vh_rows_free(rows)
    return info, (int(flags.value) if rows_flags is not None else None), wall


def legs(limit):
    """The two legs of one limit, ALTERNATING query by query: what drifts between runs — the allocator's state above all, a limit-0 select
    allocates its 120 MB of output inside the timed window — drifts for both."""
    plans = [("planes", t._select_plan(w.plan.filter, cols, 0, limit, None, 0)), ("no_sliced", t._select_plan(w.plan.filter, cols, 0, limit, None, capi.PLAN_NO_SLICED))]
    ks, ws, last = {}, {}, {}
    for r in range(3 + 20):
        for label, (sp, keep) in plans:
            info, path, wall = select(sp)
            if r >= 3:
                ks.setdefault(label, []).append(info.kernel_ms); ws.setdefault(label, []).append(wall); last[label] = (info, path)
    for label, _ in plans:
        k, v, (info, path) = sorted(ks[label]), sorted(ws[label]), last[label]
        lines.append({"tag": tag, "leg": label, "limit": limit, "rows": nseg * w.segment_rows, "kernel_ms": round(k[len(k) // 2], 4), "kernel_ms_min": round(k[0], 4),
                      "wall_ms": round(v[len(v) // 2], 4), "queries": len(k), "nrows": info.nrows, "passed": info.passed_recs,
                      "flags": path, "sliced": None if path is None else bool(path & capi.INFO_SLICED)})
        print(json.dumps(lines[-1]), flush=True)


for limit in (0, 1000):
    legs(limit)
    assert lines[-1]["passed"] == lines[-2]["passed"] and lines[-1]["nrows"] == lines[-2]["nrows"], lines[-2:]
    assert not lines[-1]["sliced"], lines[-1]
kept = []
if os.path.exists(out):
    kept = [l for l in (json.loads(s) for s in open(out) if s.strip()) if l.get("tag") != tag]
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    for l in kept + lines:
        f.write(json.dumps(l) + "\n")
