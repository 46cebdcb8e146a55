"""cmd/freeimpala-shaped binaries with --learner-arch atari --atari-records planes: synthetic
actors write single-plane records (7 elements per step and a 21-element history block), the
learner rebuilds the 4-frame stacks on the device. Every dumped batch is unpacked and stacked on
the host, every step of the run is replayed bit-exactly by a Python planes handle and checked
stage by stage against the oracle on the host-stacked frames.
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
T, B, A = 2, 4, 18
ENTRY = 1024 * (7 * T + 28)  # 42 elements: 3 records of 7 and the history block of 21
# --seed 1: the 16 entries of this run hold starts on record 0 and one after a discount of 0
ARGS = ["--learner-arch", "atari", "--atari-records", "planes", "--players", "1", "--seq-length", "2",
        "--entry-size", "42", "--game-steps", "3", "--batch-size", "4", "--buffer-capacity", "8", "--agents", "2",
        "--iterations", "8", "--agent-time", "0", "--optimizer", "sgd", "--lr", "1e-3", "--max-grad-norm", "0",
        "--publish", "fp32", "--seed", "1"]


def replica():
    from freeimpala_amd.learner import DeviceLearner
    return DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, optimizer="sgd", lr=1e-3, max_grad_norm=0.0,
                         records="planes")


def batch_of(dump, k):
    batch = np.fromfile(dump / f"batch_0_{k}.bin", np.uint8)
    assert batch.size == B * ENTRY
    return batch


def replay(dump, k, L):
    """Step k of the run on the replica: from params_0_k and batch_0_k to params_0_{k+1} and
    grads_0_k, bit for bit; the frames it leaves resident are stack_planes of the dumped batch.
    Returns the batch's episode_start flags."""
    from freeimpala_amd.learner import stack_planes, unpack_atari_plane_records
    batch = batch_of(dump, k)
    planes, history, start, mu, act, rew, disc = unpack_atari_plane_records(batch, T, B, A)
    assert ((act >= 0) & (act < A)).all()
    L.set_params(np.fromfile(dump / f"params_0_{k}.bin", np.float32), version=k)
    st = L.step([e.tobytes() for e in batch.reshape(B, ENTRY)])
    np.testing.assert_array_equal(L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4)),
                                  stack_planes(planes, history, start))
    np.testing.assert_array_equal(L.tensor("mu", shape=(T, B, A)), mu)
    np.testing.assert_array_equal(L.tensor("discounts", shape=(T, B)), disc)
    np.testing.assert_array_equal(L.tensor("grads"), np.fromfile(dump / f"grads_0_{k}.bin", np.float32))
    np.testing.assert_array_equal(L.get_params(), np.fromfile(dump / f"params_0_{k + 1}.bin", np.float32))
    want = json.loads((dump / f"stats_0_{k}.json").read_text())
    for key in ("pg_loss", "baseline_loss", "entropy_loss", "total_loss", "grad_norm", "version"):
        assert st[key] == want[key], (k, key)
    # the writer's rule: a record follows a discount of 0 exactly when it starts an episode
    np.testing.assert_array_equal(start[1:], disc == 0)
    return start


def test_cli_atari_planes_end_to_end_replayed_bit_exactly(orc, tmp_path, monkeypatch):
    from test_gpu_atari import _check_step_against_oracle
    dump = tmp_path / "dump"
    r = run(ARGS + ["--checkpoint-freq", "0", "--checkpoint-location", str(tmp_path / "ck"), "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["learner_iterations"] == [4] and out["expected_iterations"] == 2 * 8 // 4
    m = out["metrics"]
    assert m["learner_env_steps"] == 4 * T * B and m["rejected_batches"] == 0
    assert m["learner_model_updates"] == 4 and m["data_transfers"] == 2 * 8
    monkeypatch.setenv("FI_KEEP_DA1", "1")
    monkeypatch.setenv("FI_A1_NHWC", "1")
    L = replica()
    starts = []
    for k in range(4):
        starts.append(replay(dump, k, L))
        # the same step against the oracle: the batch is resident, back to the step's parameters
        L.set_params(np.fromfile(dump / f"params_0_{k}.bin", np.float32))
        _check_step_against_oracle(orc, L, T, B, A)
    L.close()
    starts = np.stack(starts)
    assert starts.any(), "the run holds no episode_start"
    assert starts[:, 0].any() and not starts[:, 0].all()


@pytest.mark.skipif(MPIEXEC is None, reason="no mpiexec (MPICH) in this image")
def test_mpi_cli_atari_planes_end_to_end(tmp_path):
    """Two MPI actor ranks send 42 KiB plane trajectories (tag 100 + p) to the rank-0 learner."""
    dump = tmp_path / "dump"
    exe = _make("build/fi_freeimpala_mpi", MPI_EXE)
    r = mpirun(3, [exe] + ARGS + ["--checkpoint-freq", "0", "--checkpoint-location", str(tmp_path / "ck"),
                                  "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["learner_iterations"] == [4] and out["expected_iterations"] == 4
    mm = out["mpi"]
    assert mm["actors"] == 2 and mm["trajectories"] == 2 * 8
    assert mm["trajectory_bytes"] == mm["trajectories"] * 42 * 1024 and mm["bad_messages"] == 0
    assert out["metrics"]["learner_env_steps"] == 4 * T * B and out["metrics"]["rejected_batches"] == 0
    L = replica()
    replay(dump, 0, L)
    L.close()


def test_cli_refuses_a_small_entry_and_a_wrong_arch():
    r = run(ARGS[:ARGS.index("--entry-size")] + ["--entry-size", "41"] + ARGS[ARGS.index("--entry-size") + 2:])
    assert r.returncode != 0
    assert "42 = 7 * (seq_length + 1) + 21" in r.stderr, r.stderr
    r = run(["--learner-arch", "mlp", "--atari-records", "planes"])
    assert r.returncode != 0 and "--atari-records" in r.stderr
    r = run(ARGS + ["--num-actions", "19"])
    assert r.returncode != 0 and "mu[18]" in r.stderr
    r = run(["--learner-arch", "atari", "--atari-records", "rows"])
    assert r.returncode != 0 and "stacked|planes" in r.stderr
