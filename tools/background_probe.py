"""What a caller who prepares nothing pays per query, inline and with background builds (csrc/vhh_build.h).

Three legs, each in a fresh process with an empty JIT cache directory, each twelve queries of the C3 plan on a table nobody prepared:
  inline      the default: the queries compile and build themselves;
  background  vh_table_set_build_mode(VH_BUILD_BACKGROUND): the worker compiles and builds beside them;
  existing    VH_PLAN_NO_JIT | NO_PACK | NO_NARROW | NO_PREDPACK: the arenas through the pre-built kernels, i.e. what a query costs on
              "what exists" — code the background mode does not touch.
Writes profiles/r07/background.json: the per-query wall times (ms) of the three legs, the query index from which the background leg runs on the
compiled kernel and the layouts, vh_build_info of the background leg, and the size. `--rows N` (default: 1 000 M, falling back to 100 M when
the table does not fit)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUERIES = 12


def leg(name, rows):
    from viyadb_amd import capi, executor, synth
    from viyadb_amd.executor import AggPlan
    executor.init(0)
    seg = 1_000_000
    w = synth.c3(segment_rows=seg)
    dt = synth.create_device_table(w, rows // seg, seg)
    flags = 0
    if name == "existing":
        flags = capi.PLAN_NO_JIT | capi.PLAN_NO_PACK | capi.PLAN_NO_NARROW | capi.PLAN_NO_PREDPACK
    if name == "background":
        dt.set_build_mode(True)
    plan = AggPlan(filter=w.plan.filter, groups=w.plan.groups, metrics=w.plan.metrics, flags=flags, groups_hint=w.plan.groups_hint)
    ms, kernel_ms, info_flags = [], [], []
    for _ in range(QUERIES):
        t0 = time.perf_counter()
        res = dt.query_agg(plan)
        ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(res.scan_kernel_ms)
        info_flags.append(res.flags)
    out = {"per_query_ms": ms, "scan_kernel_ms": kernel_ms, "flags": info_flags}
    if name == "background":
        bi = dt.build_wait(120_000)
        out["build_info_after_wait"] = {k: getattr(bi, k) for k, _ in capi.BuildInfo._fields_}
        steady = []
        for _ in range(QUERIES):
            t0 = time.perf_counter()
            res = dt.query_agg(plan)
            steady.append((time.perf_counter() - t0) * 1e3)
        out["after_wait_per_query_ms"] = steady
        out["after_wait_flags"] = res.flags
        ready = [i for i, f in enumerate(info_flags) if f & capi.INFO_JIT and f & capi.INFO_PACKED and not f & capi.INFO_BUILD_PENDING]
        out["first_query_on_kernel_and_layouts"] = ready[0] if ready else None
    dt.close()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "background.json"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.rows)
    result = {"rows": a.rows, "queries": QUERIES, "workload": "C3, unprepared"}
    for name in ("inline", "background", "existing"):
        with tempfile.TemporaryDirectory() as cache:
            env = dict(os.environ, VH_JIT_CACHE_DIR=cache, VH_TIMES="")
            env.pop("VH_TIMES")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--rows", str(a.rows)], env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit(f"leg {name} failed with exit {p.returncode}")      # (nothing more is started on the device)
        result[name] = json.loads(lines[-1][4:])
    bg, ex, inl = result["background"], result["existing"], result["inline"]
    result["summary"] = {
        "background_slowest_ms": max(bg["per_query_ms"]), "existing_slowest_ms": max(ex["per_query_ms"]), "existing_fastest_ms": min(ex["per_query_ms"]),
        "inline_slowest_ms": max(inl["per_query_ms"]),
        "background_steady_ms": min(bg["after_wait_per_query_ms"]), "inline_steady_ms": min(inl["per_query_ms"][-4:]),
        "worker_lock_ms": bg["build_info_after_wait"]["lock_ms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["summary"]))


if __name__ == "__main__":
    main()
