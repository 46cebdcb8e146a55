"""The MLP policy's bf16 mode (include/fi_mlp.h, csrc/mlp_bf16.hip) on the device: every kernel on its own against
fp64 from the tensors one resident step leaves behind, with the derived bounds and helpers of
tests/test_gpu_atari_kernels.py and tests/atari_ref.py and no other tolerance; run-to-run equality; actor == learner
bit for bit; the setter's rules; the target network's image swap."""
import numpy as np
import pytest

import atari_ref as R
from test_gpu_atari_kernels import check_bf16, check_f32, check_wgrad

pytestmark = pytest.mark.gpu

# (D, H, A, T, B). The first four are the issue's. The last two stand on either side of the edges of the kernels
# as built that those miss: 2046 rows are one weight-gradient slice and 2200 rows two (splits = rows / 1024) of 18
# and 17 chunks of 64 rows, the last one partial; A + 1 = 32 fills one 32-column head tile and two k-steps and
# A + 1 = 33 opens the next of each; D = 16 is one k-step of layer 1 and D = 17 two.
CASES = [(128, 256, 18, 2, 100), (24, 32, 2, 1, 3), (1, 64, 64, 3, 43), (128, 256, 5, 1, 256),
         (16, 32, 31, 1, 1023), (17, 32, 32, 1, 1100)]
IDS = ["config2_tail", "narrowest", "d1_a64", "exact_tiles", "one_slice_a31_d16", "two_slices_a32_d17"]


def structured_mlp(D, H, A, seed):
    """atari_ref.structured_params' cousin for the MLP slab: observations in [0, 1); an output channel's weights share
    one sign (+-50 % in magnitude, pre-activations O(1)); of 8 channels 5 are on (bias -0.05), 1 is off, 2 switch from
    row to row (a bias of the other sign near the channel's mean); heads of both signs, +-10 % per output."""
    rs = np.random.RandomState(seed)
    parts, xm = [], 0.5
    for K in (D, H):
        mag = (0.5 + rs.random_sample((K, H))) / (K * xm)
        kind = rs.permutation(np.arange(H) % 8)
        sign = np.where((kind < 5) | (kind == 6), 1.0, -1.0)
        f = 1.0 + 0.3 * (2.0 * rs.random_sample(H) - 1.0)
        parts += [(mag * sign).ravel(), np.where(kind < 5, -0.05, np.where(kind == 5, f, np.where(kind == 6, -f, 0.0)))]
        xm = 0.65
    mag = (0.9 + 0.2 * rs.random_sample((H, A + 1))) / (H * xm) * (0.3 + 1.5 * rs.random_sample(A + 1))
    parts += [(mag * np.where(rs.random_sample(A + 1) < 0.5, 1.0, -1.0)).ravel(), 0.1 * rs.standard_normal(A + 1)]
    return np.concatenate(parts).astype(np.float32)


def case_inputs(D, H, A, T, B):
    p0 = structured_mlp(D, H, A, 900 + D + H + A)
    obs = np.random.RandomState(77 + T + B).random_sample(((T + 1) * B, D)).astype(np.float32)
    return p0, obs


def mk(D, H, A, T, B, prec="bf16", **kw):
    from freeimpala_amd.learner import DeviceLearner
    L = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, obs_dim=D, hidden=H, optimizer="sgd", lr=1e-3,
                      max_grad_norm=0.0, **kw)
    if prec:
        L.set_mlp_precision(prec)
    p0, obs = case_inputs(D, H, A, T, B)
    L.synth(seed=5)
    L.set_params(p0)
    L.upload("obs", obs)
    return L, p0, obs


def terms(x, w, b=0.0):
    """(r, S) of x . w + b in fp64: the result and the sum of the terms' absolute values."""
    return x @ w + b, np.abs(x) @ np.abs(w) + np.abs(b)


@pytest.mark.parametrize("D,H,A,T,B", CASES, ids=IDS)
def test_every_kernel_vs_fp64(D, H, A, T, B):
    """One step; then each kernel from the GPU's own stored inputs. K = D, H, H, A + 1, H; c = 1 where a bias is added,
    0 in the data gradients."""
    from freeimpala_amd import mlp_bf16 as M
    L, p0, obs = mk(D, H, A, T, B)
    assert L.mlp_precision == "bf16"
    L.step_resident()
    N, TB = (T + 1) * B, T * B
    assert L.tensor_ptr("h1")[1] == N * H * 2 and L.tensor_ptr("dz1")[1] == N * H * 2
    b = {nm: L.tensor(nm, np.uint16, (N, H)) for nm in ("h1", "h2", "dz1", "dz2")}
    v = {nm: R.bf16_bits_to_f64(x) for nm, x in b.items()}
    logits, values = L.tensor("logits", shape=(N, A)), L.tensor("values", shape=(N,))
    dout = np.zeros((N, A + 1), np.float32)
    dout[:TB, :A] = L.tensor("dlogits", shape=(TB, A))
    dout[:, A] = L.tensor("dvalue", shape=(N,))
    np.testing.assert_array_equal(L.tensor("obs", shape=(N, D)), obs)
    grads = M.split_params(L.tensor("grads"), D, H, A)
    L.close()

    P = M.split_params(p0, D, H, A)
    W1, W2, Wh = (M.rne(P[k]) for k in ("W1", "W2", "Wh"))
    x, d = M.rne(obs), M.rne(dout)
    out = dict(fails=[], stats={})
    check_bf16(out, "h1", b["h1"], terms(x, W1, P["b1"]), D, 1, relu=True)
    check_bf16(out, "h2", b["h2"], terms(v["h1"], W2, P["b2"]), H, 1, relu=True)
    r, S = terms(v["h2"], Wh, P["bh"])
    check_f32(out, "logits", logits, (r[:, :A], S[:, :A]), H, 1)
    check_f32(out, "values", values, (r[:, A], S[:, A]), H, 1)
    check_bf16(out, "dz2", b["dz2"], [t * (v["h2"] > 0) for t in terms(d, Wh.T)], A + 1, 0)
    check_bf16(out, "dz1", b["dz1"], [t * (v["h1"] > 0) for t in terms(v["dz2"], W2.T)], H, 0)
    for nm, X, dY in (("W1", x, v["dz1"]), ("W2", v["h1"], v["dz2"]), ("Wh", v["h2"], d)):
        check_wgrad(out, "g" + nm, grads[nm], terms(X.T, dY))
        check_wgrad(out, "gb" + nm[1], grads["b" + nm[1]].reshape(1, -1), (dY.sum(0, keepdims=True), None))
    for nm, s in out["stats"].items():
        print(f"  {nm}: {s}")
    assert not out["fails"], "\n".join(out["fails"])


def test_two_runs_give_equal_bits():
    got = []
    for _ in range(2):
        L, _, _ = mk(*CASES[0])
        L.step_resident()
        got.append((L.tensor("grads").view(np.uint32), L.get_params().view(np.uint32)))
        L.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("N", [7, 300])
@pytest.mark.parametrize("blob", ["fp32", "bf16"])
def test_actor_equals_learner(N, blob):
    """Row independence: N rows in an actor's tiles give the bits the same rows give among the learner's 300. The
    parameters are bf16 values, so both blobs carry the same numbers (the bf16 blob rounds the fp32 biases too)."""
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.publish import round_params
    D, H, A, T, B = CASES[0]
    L, p0, obs = mk(D, H, A, T, B)
    p0 = round_params(p0, "bf16")
    L.set_params(p0)
    L.step_resident()
    logits, values = L.tensor("logits", shape=((T + 1) * B, A))[:N], L.tensor("values", shape=((T + 1) * B,))[:N]
    L.close()
    a = Actor("mlp", num_envs=N, num_actions=A, obs_dim=D, hidden=H, mode="greedy")
    a.set_mlp_precision("bf16")
    a.set_params(p0 if blob == "fp32" else (p0.view(np.uint32) >> 16).astype(np.uint16).tobytes())
    got = a.act_obs(obs[:N])
    a.close()
    np.testing.assert_array_equal(got["logits"].view(np.uint32), logits.view(np.uint32))
    np.testing.assert_array_equal(got["values"].view(np.uint32), values.view(np.uint32))


def test_setter_rules():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import DeviceLearner
    L, p0, _ = mk(*CASES[1])
    L.step_resident()
    with pytest.raises(FiError, match="rc=-4:"):
        L.set_mlp_precision("fp32")
    # a batch with an out-of-range action is still refused and skips the update
    before = L.get_params()
    acts = L.tensor("actions", np.int32)
    acts[0] = CASES[1][2]
    L.upload("actions", acts)
    with pytest.raises(FiError, match="rc=-1:"):
        L.step_resident()
    np.testing.assert_array_equal(L.get_params().view(np.uint32), before.view(np.uint32))
    L.close()
    X = DeviceLearner("atari", seq_len=1, batch=2, num_actions=4)
    with pytest.raises(FiError, match="rc=-1:"):
        X.set_mlp_precision("bf16")
    X.close()
    for H in (48, 288):
        X = DeviceLearner("mlp", seq_len=1, batch=3, num_actions=2, obs_dim=24, hidden=H, optimizer="sgd", lr=1e-3)
        with pytest.raises(FiError, match=f"rc=-6:.*hidden {H}"):
            X.set_mlp_precision("bf16")
        X.synth(seed=5)
        assert X.mlp_precision == "fp32" and np.isfinite(X.step_resident()["total_loss"])
        assert X.tensor_ptr("h1")[1] == 6 * H * 4
        X.close()


def test_target_network_swaps_the_images():
    """theta- differs from the parameters: tlogits follow theta-'s images, the step's own logits the parameters'."""
    from freeimpala_amd import hip, mlp_bf16 as M
    D, H, A, T, B = CASES[1]
    L, p0, obs = mk(D, H, A, T, B)
    L.set_objective("surrogate")
    L.enable_target(period=1)
    theta = (p0 * np.float32(1.25)).astype(np.float32)
    L.set_target_params(theta)
    L.step_resident()
    N = (T + 1) * B
    tlogits = hip.download_ptr(L.target_logits_dev(), np.float32, (N, A))
    logits = L.tensor("logits", shape=(N, A))
    L.close()
    out = dict(fails=[], stats={})
    for nm, got, p in (("tlogits", tlogits, theta), ("logits", logits, p0)):
        ref, P = M.mlp_bf16_reference(obs, p, D, H, A), M.split_params(p, D, H, A)
        r, S = terms(ref["h2"], M.rne(P["Wh"]), P["bh"])
        np.testing.assert_array_equal(r[:, :A], ref["logits"])
        check_f32(out, nm, got, (r[:, :A], S[:, :A]), H, 1)
    assert not out["fails"], "\n".join(out["fails"])
    assert np.abs(tlogits - logits).max() > 1e-3
