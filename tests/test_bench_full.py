"""bench.py plain and with --full: a plain run carries the headline and nothing that takes work of its own (no CPU baseline,
no parity sample, no search timed by itself); --full carries all of them -- and both run the very same steps on the very
same inputs: what --dump-outputs writes is equal bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import ROOT

BENCH = os.path.join(ROOT, "bench.py")
MOVED = ("cpu_baseline", "cpu_baseline_reference", "parity_sample_max_rel", "parity_lists", "search_ms")


def test_full_is_an_option_off_by_default():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "[--full]" in out.stdout        # (a flag: it takes no value)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """One plain and one --full run of the same small workload, each with its dump."""
    got = {}
    for name, extra in (("plain", []), ("full", ["--full", "--cpu-seconds", "0.5"])):
        d = str(tmp_path_factory.mktemp(name))
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "C2-mini", "--steps", "1", "--warmup", "1",
                              "--dump-outputs", d, *extra], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1
        got[name] = (json.loads(js[0]), d)
    return got


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only(lines):
    d, _ = lines["plain"]
    assert d["full"] is False
    assert d["metric"] == "grid-point LETKF solves/sec" and d["unit"] == "solves/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 1 and d["warmup"] == 1
    assert abs(d["value"] - d["config"]["points_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["nonzero_status_points"] == 0 and d["roofline"]["kernel_ms"] > 0
    for key in MOVED:
        assert key in d and d[key] is None, key


@pytest.mark.gpu
def test_full_run_carries_baseline_parity_and_search_time(lines):
    d, _ = lines["full"]
    assert d["full"] is True and d["value"] > 0 and d["nonzero_status_points"] == 0
    assert d["parity_sample_max_rel"] is not None and d["parity_sample_max_rel"] <= d["parity_tolerance"] == 1e-10
    assert d["parity_lists"]["points"] > 0 and "oracle" in d["parity_lists"]["lists"]
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    assert d["search_ms"] > 0


@pytest.mark.gpu
def test_both_run_the_same_steps_on_the_same_inputs(lines):
    (p, dp), (f, df) = lines["plain"], lines["full"]
    assert p["config"] == f["config"] and p["warm_runs"] == f["warm_runs"] and p["obs_spread"] == f["obs_spread"]
    assert p["jacobi_sweeps_mean"] == f["jacobi_sweeps_mean"] and p["roofline"]["kernel"] == f["roofline"]["kernel"]
    assert sorted(os.listdir(dp)) == sorted(os.listdir(df)) == ["anal.npy", "nobs.npy", "points.npy", "status.npy"]
    for name in os.listdir(dp):
        a, b = np.load(os.path.join(dp, name)), np.load(os.path.join(df, name))
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
