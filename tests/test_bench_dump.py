"""`bench.py --dump-outputs DIR` (no GPU: a result of the timed path's shape, made up): the arrays as float64 .npy files, groups sorted
by their keys, at most 64 MB in all with a fixed seeded sample above that; and `--steps` below 1 is refused before anything runs."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

import bench
from viyadb_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(ng, seed=1):
    rng = np.random.default_rng(seed)
    k0 = rng.permutation(ng).astype(np.uint32)
    k1 = (k0 % 13).astype(np.uint32)
    return SimpleNamespace(keys=[k1, k0], states=[k0.astype(np.int64) * 3 - 7, (k0 % 5 + 1).astype(np.uint32)], hidden_count=None)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_sorted_float64_and_complete(tmp_path):
    w = synth.WORKLOADS["C3"](segment_rows=1000)
    res = _result(5000)
    info = bench.dump_outputs(res, w, w.plan, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["key0_d0", "key1_d1", "state0_m0", "state1_count"] and not info["sampled"]
    assert all(a.dtype == np.float64 and a.shape == (5000,) for a in got.values())
    order = np.lexsort([res.keys[1], res.keys[0]])
    for name, src in (("key0_d0", res.keys[0]), ("key1_d1", res.keys[1]), ("state0_m0", res.states[0]), ("state1_count", res.states[1])):
        assert np.array_equal(got[name], src[order].astype(np.float64)), name


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    w = synth.WORKLOADS["C3"](segment_rows=1000)
    full = tmp_path / "full"
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 30)
    bench.dump_outputs(_result(50_000), w, w.plan, str(full))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    a, b = tmp_path / "a", tmp_path / "b"
    ia = bench.dump_outputs(_result(50_000), w, w.plan, str(a))
    bench.dump_outputs(_result(50_000, seed=2), w, w.plan, str(b))       # the same groups in another order
    assert ia["sampled"] and ia["written_groups"] < 50_000
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 200_000
    ga, gb, gf = _load(a), _load(b), _load(full)
    assert sorted(ga) == sorted(gb) and "group_index" in ga
    for name in ga:
        assert np.array_equal(ga[name], gb[name]), name
        if name != "group_index":
            assert np.array_equal(ga[name], gf[name][ga["group_index"].astype(np.int64)]), name


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
