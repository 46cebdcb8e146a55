"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only (what
--full adds stays out of it), --steps is the number of timed steps, and --dump-outputs DIR
writes what the last timed step left a caller (parameters, gradient, logits, values) as float32
.npy files under a fixed size budget, cut to a seeded sample where an array would exceed it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("sustained", "roofline", "roofline_vtrace", "step_roofline", "kernel_ms_per_step", "phase_ms",
             "final_loss", "cpu_baseline")


class _FakeLearner:
    """stands in for DeviceLearner: four arrays of known contents"""

    def __init__(self, sizes):
        self.a = {k: np.arange(n, dtype=np.float32) + i for i, (k, n) in enumerate(sizes.items())}

    def get_params(self):
        return self.a["params"]

    def tensor(self, name):
        return self.a[name]


def test_dump_outputs_whole_arrays_under_the_budget(tmp_path):
    L = _FakeLearner({"params": 1000, "grads": 1000, "logits": 5000, "values": 300})
    bench.dump_outputs(L, str(tmp_path / "d"), budget_bytes=4 * 8000)
    for k, want in L.a.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)


def test_dump_outputs_samples_what_exceeds_the_budget(tmp_path):
    sizes = {"params": 1000, "grads": 1000, "logits": 50000, "values": 300}
    budget = 4 * 6000
    outs = []
    for run in ("a", "b"):
        bench.dump_outputs(_FakeLearner(sizes), str(tmp_path / run), budget_bytes=budget)
        outs.append({k: np.load(tmp_path / run / f"{k}.npy") for k in sizes})
    a, b = outs
    assert sum(v.nbytes for v in a.values()) <= budget
    for k in ("params", "grads", "values"):  # the small arrays stay whole
        assert a[k].size == sizes[k]
    # logits: what the others left, a strictly increasing (so duplicate-free) sample of the
    # original (arange + 2: the value tells the index), the same in both runs
    assert a["logits"].size == 6000 - 2300
    assert np.all(np.diff(a["logits"]) > 0) and a["logits"].min() >= 2 and a["logits"].max() < 50002
    for k in sizes:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    T, B, A, D, H, steps = 8, 64, 18, 128, 256, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "LOCAL_RANK", "RANK",
                                                               "TORCHELASTIC_RUN_ID")}
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--arch", "mlp",
                            "--seq-len", str(T), "--batch", str(B), "--steps", str(steps), "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)],
                           env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
    d = lines[0]
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    # value is T * B * steps / elapsed and ms_per_step is elapsed / steps: the step count cancels
    # only if --steps really is the number of timed steps
    np.testing.assert_allclose(d["value"], T * B / (d["ms_per_step"] * 1e-3), rtol=1e-3)
    n_params = D * H + H + H * H + H + H * (A + 1) + (A + 1)
    shapes = {"params": n_params, "grads": n_params, "logits": (T + 1) * B * A, "values": (T + 1) * B}
    a, b = ({k: np.load(tmp_path / run / f"{k}.npy") for k in shapes} for run in ("a", "b"))
    for k, n in shapes.items():
        assert a[k].dtype == np.float32 and a[k].shape == (n,), k
        assert np.isfinite(a[k]).all(), k
        # the same seeded inputs and initial parameters in both runs. The only run-to-run
        # difference is the summation order of fp32 atomics in the gradient (~1e-6 relative);
        # Adam's normalised update can amplify it for the few elements whose gradient is at that
        # noise level, by at most 2 * lr per step each. Another batch or other parameters would
        # differ by O(1) in relative L2, so 1e-2 tells the two apart.
        rel = np.linalg.norm(a[k].astype(np.float64) - b[k]) / max(1e-30, np.linalg.norm(a[k].astype(np.float64)))
        assert rel <= 1e-2, (k, rel)
    assert np.abs(a["grads"]).max() > 0 and np.abs(a["logits"]).max() > 0
