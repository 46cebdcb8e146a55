"""CPU-side checks of actor exploration (include/fi_explore.h): the in-tree libfi_learner.so exports
exactly the functions the header declares and freeimpala_amd.explore binds exactly that set, in a
header of its own; behaviour_reference -- the host form of the rule -- against the definitions it
must satisfy and against the plain sampling rule; epsilon_ladder."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h", "fi_train.h", "fi_breakout.h", "fi_publish.h")
FUNCTIONS = ("fi_explore_set", "fi_explore_clear", "fi_explore_get", "fi_explore_behaviour_dev",
             "fi_explore_read_behaviour", "fi_sample_behaviour")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_explore_header():
    from freeimpala_amd import (_abi, actor, breakout, env, explore, farmer, gather, prio, publish, ring, rollout, train,
                                weights)
    lib = explore.lib()
    names = header_functions("fi_explore.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(explore.SIGNATURES), set(names) ^ set(explore.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_explore_")} == {n for n in names if n.startswith("fi_explore_")}
    assert set(names) <= exported
    # a header of its own: no older header and no older table gains a function
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for mod in (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish):
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(actor.SIGNATURES) == 17 and len(publish.SIGNATURES) == 8
    assert lib.fi_abi_version() == 1


def case(N=64, A=18, scale=3.0, seed=1):
    rs = np.random.RandomState(seed)
    logits = (scale * rs.standard_normal((N, A))).astype(np.float32)
    from freeimpala_amd.explore import epsilon_ladder
    eps = epsilon_ladder(N)
    eps[::5] = 0.0
    eps[3] = eps[N - 2] = 1.0
    return logits, eps


@pytest.mark.parametrize("tau", [0.25, 1.0, 4.0])
def test_reference_mu_is_the_log_of_w_over_W(tau):
    """softmax(mu) sums to 1 and equals w / W, w built here from the header's definitions."""
    from freeimpala_amd.explore import behaviour_reference
    logits, eps = case()
    N, A = logits.shape
    act, near, mu = behaviour_reference(logits, tau, eps, seed=9, draw=4)
    assert mu.dtype == np.float64 and mu.shape == (N, A) and act.dtype == np.int32 and near.dtype == bool
    assert np.isfinite(mu).all()
    sm = np.exp(mu - mu.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    np.testing.assert_allclose(np.exp(mu).sum(1), 1.0, rtol=0, atol=1e-12)
    l = logits.astype(np.float64)
    p = np.exp((l - l.max(1, keepdims=True)) / tau)
    Z = p.sum(1, keepdims=True)
    e = eps.astype(np.float64)[:, None]
    w = (1 - e) * p + e * Z / A
    np.testing.assert_allclose(sm, w / w.sum(1, keepdims=True), rtol=1e-12, atol=1e-300)
    # the action is the first index whose running sum of w exceeds u W
    from freeimpala_amd.explore import uniforms
    u = uniforms(9, 4, N)
    c = np.cumsum(w, 1)
    for i in range(N):
        over = np.nonzero(c[i] > u[i] * c[i, -1])[0]
        assert act[i] == (over[0] if over.size else A - 1)


def test_reference_mu_stays_finite_where_p_underflows():
    from freeimpala_amd.explore import behaviour_reference
    logits = np.zeros((2, 4), np.float32)
    logits[:, 1] = -2000.0  # exp(-2000 / 0.5) is 0 in fp64 as well
    _, _, mu = behaviour_reference(logits, 0.5, np.array([0.0, 0.25], np.float32), 0, 0)
    assert np.isfinite(mu).all()
    assert mu[0, 1] == -4000.0 - np.log(3.0)              # eps = 0: z - log Z
    np.testing.assert_allclose(mu[1, 1], np.log(0.25 / 4), rtol=1e-15)  # eps > 0: the uniform floor


def test_reference_epsilon_one_is_uniform_and_depends_on_u_alone():
    from freeimpala_amd.explore import behaviour_reference, uniforms
    logits, _ = case(N=200, A=9)
    other = np.random.RandomState(77).standard_normal(logits.shape).astype(np.float32) * 5
    for tau in (0.25, 1.0, 4.0):
        act, _, mu = behaviour_reference(logits, tau, 1.0, seed=3, draw=11)
        act2, _, mu2 = behaviour_reference(other, tau, 1.0, seed=3, draw=11)
        np.testing.assert_allclose(mu, -np.log(9.0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(mu2, -np.log(9.0), rtol=0, atol=1e-12)
        # u is a multiple of 2^-24 and the boundaries are k / 9: no tie, the action is floor(9 u)
        want = np.minimum(np.floor(uniforms(3, 11, 200) * 9), 8).astype(np.int32)
        np.testing.assert_array_equal(act, want)
        np.testing.assert_array_equal(act2, want)


def test_reference_at_tau_one_epsilon_zero_is_the_plain_rule(orc):
    """The actions of the existing fp64 sampling reference (tests/test_gpu_actor.py, built on the
    oracle's Philox) on the same inputs, and mu = log softmax(logits)."""
    from test_gpu_actor import ref_sample
    from freeimpala_amd.explore import behaviour_reference
    for (N, A, seed, draw) in ((64, 6, 5, 0), (257, 18, 0x5EED0101, 7), (100, 64, 2 ** 40 + 3, 2 ** 33)):
        logits = (2.0 * np.random.RandomState(N + A).standard_normal((N, A))).astype(np.float32)
        want, want_near = ref_sample(orc, logits, seed, draw)
        for eps in (None, 0.0, np.zeros(N, np.float32)):
            act, near, mu = behaviour_reference(logits, 1.0, eps, seed, draw)
            np.testing.assert_array_equal(act, want)
            np.testing.assert_array_equal(near, want_near)
        l = logits.astype(np.float64)
        lse = np.log(np.exp(l - l.max(1, keepdims=True)).sum(1, keepdims=True)) + l.max(1, keepdims=True)
        np.testing.assert_allclose(mu, l - lse, rtol=0, atol=1e-12)


def test_epsilon_ladder():
    from freeimpala_amd.explore import epsilon_ladder
    e = epsilon_ladder(8)
    assert e.dtype == np.float32 and e.shape == (8,)
    assert e[0] == np.float32(0.4) and e[-1] == np.float32(0.4 ** 8)
    assert (np.diff(e) < 0).all()
    np.testing.assert_allclose(e, 0.4 ** (1 + 7 * np.arange(8) / 7), rtol=1e-7)
    assert epsilon_ladder(1).tolist() == [np.float32(0.4)]
    np.testing.assert_allclose(epsilon_ladder(3, base=0.5, alpha=2.0), [0.5, 0.25, 0.125], rtol=1e-7)
    with pytest.raises(ValueError):
        epsilon_ladder(0)
