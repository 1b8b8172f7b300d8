"""bench.py's comparison contract on a GPU (small config, fresh child processes): --dump-outputs writes what the last timed decision
returned (names, float dtypes, shapes), two runs with the same arguments write the same arrays, a plain run's line holds the headline
only, and --full adds the measurement objects without changing what the timed decisions compute."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
MOVED = ("roofline", "roofline_mfma", "end_to_end", "cpu_baseline", "fp8_vs_bf16")


def _bench(out_dir, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--small", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(out_dir)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return line, {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(str(out_dir), "*.npy"))}


@pytest.fixture(scope="module")
def bench_runs(dev, tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    return [_bench(d / "plain0"), _bench(d / "plain1"), _bench(d / "full", ["--full"])]


def test_bench_plain_line_and_dumped_outputs(bench_runs):
    line, out = bench_runs[0]
    assert all(k in line for k in HEADLINE) and not any(k in line for k in MOVED)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    N = line["config"]["candidates_total"]
    assert sorted(out) == ["scores", "tokens", "winner_index"]
    assert out["scores"].dtype == np.float32 and out["scores"].shape == (N,) and np.isfinite(out["scores"]).all()
    assert out["tokens"].dtype == np.float64 and out["tokens"].shape == (N, 7) and np.array_equal(out["tokens"], np.round(out["tokens"]))
    assert out["winner_index"].dtype == np.float64 and out["winner_index"].shape == (1,) and 0 <= out["winner_index"][0] < N


def test_bench_dumped_outputs_reproducible_and_unchanged_by_full(bench_runs):
    (_, a), (_, b), (full, c) = bench_runs
    assert sorted(a) == sorted(b) == sorted(c)
    for k in a:
        assert np.array_equal(a[k], b[k]), k          # same arguments, same inputs -> same outputs
        assert np.array_equal(a[k], c[k]), k          # --full measures more after the timed steps, computes the same
    assert all(k in full for k in HEADLINE) and "roofline_mfma" in full and full["steps"] == 2
