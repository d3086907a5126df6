"""`bench.py` plain and `--full` on a small C3 table: a plain run prints the headline line and runs none of the other legs (no parity
gate, no reference layout, no unprepared caller, no CPU baselines); `--full` runs them all as before. The timed path is the same in both:
their --dump-outputs arrays agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--segments", "4", "--segment-rows", "200000", "--steps", "3", "--warmup", "1"]


def _bench(extra, dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra + ["--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_full_runs_every_leg(tmp_path):
    plain = _bench([], tmp_path / "plain")
    assert plain["full"] is False and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "rows/s" and plain["higher_is_better"] is True
    assert plain["config"]["rows"] == 800_000 and plain["roofline"]["kernel_ms"] > 0
    assert not plain["parity_checked"] and plain["parity"] is None and plain["unprepared"] is None
    assert "reference_layout" not in plain and "cpu_baseline" not in plain and "cpu_baseline_all_cores" not in plain

    full = _bench(["--full", "--cpu-segments", "2", "--no-cpu-parallel"], tmp_path / "full")
    assert full["full"] is True and full["parity_checked"] and full["parity"]["cpu_twin_window_rows"] == 2 * 200_000
    assert full["reference_layout"]["value"] > 0 and full["unprepared"]["groups"] == plain["config"]["groups"]
    assert full["cpu_baseline"]["value"] > 0 and "cpu_baseline_all_cores" not in full
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k], k

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
