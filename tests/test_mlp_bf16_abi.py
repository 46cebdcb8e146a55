"""The MLP precision header (include/fi_mlp.h) without a device: the exports, the enum against the C compiler, the
Python methods, and the inputs of tests/test_gpu_mlp_bf16.py checked with mlp_bf16_reference alone: at most 5 % of a
stored tensor's derived intervals may hold more than four bf16 values (tests/atari_ref.py, CAP)."""
import os
import subprocess

import numpy as np
import pytest

import atari_ref as R
from test_gpu_mlp_bf16 import CASES, IDS, case_inputs, terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_enum_and_methods(tmp_path):
    from freeimpala_amd import _abi, mlp_bf16
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert set(mlp_bf16.SIGNATURES) <= exported and len(mlp_bf16.SIGNATURES) == 3
    mlp_bf16.lib()
    (tmp_path / "t.c").write_text('#include <stdio.h>\n#include "fi_mlp.h"\nint main(){printf("%d %d %zu", (int)FI_MLP_FP32, '
                                  '(int)FI_MLP_BF16, sizeof(fi_learner_config));return 0;}')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    import ctypes
    assert [int(x) for x in got] == [mlp_bf16.FP32, mlp_bf16.BF16, ctypes.sizeof(_abi.LearnerConfig)] and got[:2] == ["0", "1"]
    assert callable(DeviceLearner.set_mlp_precision) and isinstance(DeviceLearner.mlp_precision, property)
    assert callable(Actor.set_mlp_precision)
    assert mlp_bf16.lib().fi_learner_mlp_precision(None) == -1 and mlp_bf16.lib().fi_learner_set_mlp_precision(None, 1) == -1
    assert mlp_bf16.supported(128, 256, 18) and not mlp_bf16.supported(128, 48, 18) and not mlp_bf16.supported(128, 288, 18)
    with pytest.raises(ValueError):
        mlp_bf16.precision("fp16")


@pytest.mark.parametrize("D,H,A,T,B", CASES, ids=IDS)
def test_gpu_case_inputs_keep_the_intervals_narrow(D, H, A, T, B):
    """dout here is a stand-in of the step's (softmax-minus-one-hot rows times an advantage, a value error): the GPU
    test asserts the same cap on the real one."""
    from freeimpala_amd import mlp_bf16 as M
    p0, obs = case_inputs(D, H, A, T, B)
    rs, N = np.random.RandomState(3), (T + 1) * B
    ref = M.mlp_bf16_reference(obs, p0, D, H, A)
    pi = np.exp(ref["logits"] - ref["logits"].max(1, keepdims=True))
    dout = np.concatenate([pi / pi.sum(1, keepdims=True) - np.eye(A)[rs.randint(0, A, N)], rs.standard_normal((N, 1))], 1)
    dout = (dout * rs.standard_normal((N, 1))).astype(np.float32)
    dout[T * B:, :A] = 0
    ref = M.mlp_bf16_reference(obs, p0, D, H, A, dout)
    P = M.split_params(p0, D, H, A)
    W1, W2, Wh = (M.rne(P[k]) for k in ("W1", "W2", "Wh"))
    d = M.rne(dout)
    wide = {"h1": R.bf16_interval_stats(*terms(M.rne(obs), W1, P["b1"]), D, 1, True)[2],
            "h2": R.bf16_interval_stats(*terms(ref["h1"], W2, P["b2"]), H, 1, True)[2],
            "out": R.bf16_interval_stats(*terms(ref["h2"], Wh, P["bh"]), H, 1)[2],
            "dz2": R.bf16_interval_stats(*[t * (ref["h2"] > 0) for t in terms(d, Wh.T)], A + 1, 0)[2],
            "dz1": R.bf16_interval_stats(*[t * (ref["h1"] > 0) for t in terms(ref["dz2"], W2.T)], H, 0)[2]}
    assert max(wide.values()) <= R.CAP, wide
    assert ref["grads"].size == p0.size and np.isfinite(ref["grads"]).all()
