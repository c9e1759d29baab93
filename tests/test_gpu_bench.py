"""bench.py end to end at a small size (one GPU): the JSON line carries the contract's fields,
with --full the CPU baseline's answers equal the GPU's bit for bit and recall is a fraction, and
--dump-outputs writes the timed path's answer, the same from a plain and from a --full run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, K = 2000, 10
SMALL = ["--n", "300000", "--nlist", "64", "--nprobe", "8", "--nq", str(NQ), "--steps", "3", "--warmup", "1",
         "--block-rows", "40000", "--add-rows", "100000"]


def run_bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return run_bench(["--dump-outputs", str(d)]), d


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("full")
    return run_bench(["--full", "--recall-queries", "200", "--cpu-seconds", "1", "--dump-outputs", str(d)]), d


def test_bench_small_json_line(full_run):
    out = full_run[0]
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]:
        assert key in out
    assert out["n_gpus"] == 1 and out["value"] > 0
    assert 0.0 < out["recall_at_10"] <= 1.0
    cpu = out["cpu_baseline"]
    assert cpu["parity"]["ids_equal"] and cpu["parity"]["scores_bit_identical"]
    assert cpu["cores"] >= 1 and "host" in cpu
    assert 0 < out["roofline"]["frac"] < 1.5
    assert out["graph_check"]["last_replay_equals_direct_search"]


def test_bench_plain_run_is_lean(plain_run, full_run):
    out, full = plain_run[0], full_run[0]
    for key in ["metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"]:
        assert out[key] == full[key]
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(NQ / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ["roofline", "cpu_baseline", "recall_at_10", "graph_check", "phases_ms"]:
        assert key not in out


def test_bench_dump_outputs(plain_run, full_run):
    d = plain_run[1]
    assert sorted(os.listdir(d)) == ["labels.npy", "scores.npy"]
    s, lab = np.load(d / "scores.npy"), np.load(d / "labels.npy")
    assert s.dtype == np.float32 and lab.dtype == np.float64
    assert s.shape == lab.shape == (NQ, K)
    step = np.diff(s, axis=1)
    assert np.all(step >= 0) or np.all(step <= 0)  # best first, in the metric's order
    assert np.all((lab >= 0) & (lab < 300000) & (lab == np.floor(lab)))
    # the same seeded inputs: the --full run's timed path returned the same bits
    f = full_run[1]
    assert np.array_equal(np.load(f / "scores.npy").view(np.uint32), s.view(np.uint32))
    assert np.array_equal(np.load(f / "labels.npy"), lab)
