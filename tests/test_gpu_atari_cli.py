"""cmd/freeimpala-shaped binaries with --learner-arch atari: synthetic actors write Atari records
(28 elements per step), the learner steps the conv policy on them. Every step of the run is
replayed bit-exactly by a Python DeviceLearner from the dumped batch and parameters (the step is
deterministic across processes, tests/test_gpu_atari.py), and one step goes through the oracle.
"""
import json
import os

import numpy as np
import pytest

from test_dropin import _make, run
from test_mpi import MPIEXEC, mpirun

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_EXE = os.path.join(ROOT, "build", "fi_freeimpala_mpi")
T, B, A, REC = 2, 4, 18, 28672
ARGS = ["--learner-arch", "atari", "--players", "1", "--seq-length", "2", "--entry-size", "84", "--game-steps", "3",
        "--batch-size", "4", "--buffer-capacity", "8", "--agents", "2", "--iterations", "8", "--agent-time", "0",
        "--optimizer", "sgd", "--lr", "1e-3", "--max-grad-norm", "0", "--publish", "fp32", "--seed", "7"]


def replica():
    from freeimpala_amd.learner import DeviceLearner
    return DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, optimizer="sgd", lr=1e-3, max_grad_norm=0.0)


def entries_of(dump, k):
    batch = np.fromfile(dump / f"batch_0_{k}.bin", np.uint8)
    assert batch.size == B * (T + 1) * REC
    return [e.tobytes() for e in batch.reshape(B, (T + 1) * REC)]


def replay(dump, k, L):
    """Step k of the run on the replica: from params_0_k and batch_0_k to params_0_{k+1} and
    grads_0_k, bit for bit."""
    L.set_params(np.fromfile(dump / f"params_0_{k}.bin", np.float32), version=k)
    st = L.step(entries_of(dump, k))
    np.testing.assert_array_equal(L.tensor("grads"), np.fromfile(dump / f"grads_0_{k}.bin", np.float32))
    np.testing.assert_array_equal(L.get_params(), np.fromfile(dump / f"params_0_{k + 1}.bin", np.float32))
    want = json.loads((dump / f"stats_0_{k}.json").read_text())
    for key in ("pg_loss", "baseline_loss", "entropy_loss", "total_loss", "grad_norm", "version"):
        assert st[key] == want[key], (k, key)


def oracle_step(orc, dump, k, monkeypatch):
    from test_gpu_atari import _check_step_against_oracle
    monkeypatch.setenv("FI_KEEP_DA1", "1")
    monkeypatch.setenv("FI_A1_NHWC", "1")
    L = replica()
    p = np.fromfile(dump / f"params_0_{k}.bin", np.float32)
    L.set_params(p)
    L.step(entries_of(dump, k))  # leaves the batch resident
    L.set_params(p)
    _check_step_against_oracle(orc, L, T, B, A)
    L.close()


def test_cli_atari_end_to_end_replayed_bit_exactly(orc, tmp_path, monkeypatch):
    from freeimpala_amd.learner import unpack_atari_records
    dump = tmp_path / "dump"
    r = run(ARGS + ["--checkpoint-freq", "0", "--checkpoint-location", str(tmp_path / "ck"), "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["learner_iterations"] == [4] and out["expected_iterations"] == 2 * 8 // 4
    m = out["metrics"]
    assert m["learner_env_steps"] == 4 * T * B and m["rejected_batches"] == 0
    assert m["learner_model_updates"] == 4 and m["data_transfers"] == 2 * 8
    for k in range(4):
        assert (dump / f"batch_0_{k}.bin").stat().st_size == 4 * 3 * 28672
        act = unpack_atari_records(np.fromfile(dump / f"batch_0_{k}.bin", np.uint8), T, B, A)[2]
        assert ((act >= 0) & (act < A)).all()
    L = replica()
    for k in range(4):
        replay(dump, k, L)
    L.close()
    oracle_step(orc, dump, 1, monkeypatch)


@pytest.mark.skipif(MPIEXEC is None, reason="no mpiexec (MPICH) in this image")
def test_mpi_cli_atari_end_to_end(tmp_path):
    """Two MPI actor ranks send 84 KiB Atari trajectories (tag 100 + p) to the rank-0 learner."""
    dump = tmp_path / "dump"
    exe = _make("build/fi_freeimpala_mpi", MPI_EXE)
    r = mpirun(3, [exe] + ARGS + ["--checkpoint-freq", "0", "--checkpoint-location", str(tmp_path / "ck"),
                                  "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["learner_iterations"] == [4] and out["expected_iterations"] == 4
    mm = out["mpi"]
    assert mm["actors"] == 2 and mm["trajectories"] == 2 * 8
    assert mm["trajectory_bytes"] == mm["trajectories"] * 84 * 1024 and mm["bad_messages"] == 0
    assert out["metrics"]["learner_env_steps"] == 4 * T * B and out["metrics"]["rejected_batches"] == 0
    L = replica()
    replay(dump, 0, L)
    L.close()
