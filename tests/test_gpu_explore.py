"""Actor exploration on the device (include/fi_explore.h, freeimpala_amd/explore.py): the kernel
alone against behaviour_reference (fp64 on the fp32 inputs), its tau = 1 / epsilon = 0 case against
the plain sampler bit for bit, non-finite rows, the handle on host and device calls, the behaviour
logits all the way into the learner's own mu tensor, a change in the middle of an unroll, the
refusals and the C++ check program.

Actions: exact away from every boundary, within one index where the threshold u W lies within
1e-5 W of a running sum (explore.NEAR; the logic of tests/test_gpu_actor.py's check_sampled).

Behaviour logits: the absolute bound of DESIGN.md section 2.2 (exploration), derived from the
operation count with u = 2^-24 (a correctly rounded +, -, *, /, fma: relative error u; OCML's expf
and logf: 1 ulp, relative error 2 u):
    |mu_a - reference| <= 3 (A + 19) u + 5 u max(1, |mu_a|).
The bar is that bound; the worst measured fraction of it is printed."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_actor import check_sampled
from test_gpu_ring import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PLANE = 84 * 84


def mu_bound(A, mu):
    return 3 * (A + 19) * U + 5 * U * np.maximum(1.0, np.abs(mu))


def log_softmax(x):
    x = np.asarray(x, np.float64)
    s = x - x.max(-1, keepdims=True)
    return s - np.log(np.exp(s).sum(-1, keepdims=True))


def marked_ladder(N):
    """The ladder, every 5th row 0 and a few rows 1."""
    from freeimpala_amd.explore import epsilon_ladder
    eps = epsilon_ladder(N)
    eps[::5] = 0.0
    eps[[1, 2, N - 2]] = 1.0
    return eps


# ------------------------------------------------------------------ 1. the kernel alone
_cases = {}


def kernel_case(N, A, tau, sigma):
    """fp32 logits N(0, sigma^2), the epsilons and the reference's (actions, near, mu); shared, read-only."""
    key = (N, A, tau, sigma)
    if key not in _cases:
        from freeimpala_amd.explore import behaviour_reference
        rs = np.random.RandomState(7919 * A + N)
        logits = (sigma * rs.standard_normal((N, A))).astype(np.float32)
        eps = marked_ladder(N)
        seed, draw = 0xC0FFEE00 + N, 3
        ref = behaviour_reference(logits, tau, eps, seed, draw)
        for x in (logits, eps) + ref:
            x.setflags(write=False)
        _cases[key] = (logits, eps, seed, draw, ref)
    return _cases[key]


def device_behaviour(logits, tau, eps, seed, draw, count=True):
    """fi_sample_behaviour with the outputs between guards: (actions, mu, non-finite rows)."""
    from freeimpala_amd import explore, hip
    N, A = logits.shape
    dl = hip.DeviceBuffer.from_array(np.ascontiguousarray(logits, np.float32))
    de = hip.DeviceBuffer.from_array(np.ascontiguousarray(eps, np.float32)) if eps is not None else None
    dc = hip.DeviceBuffer.from_array(np.zeros(1, np.int32))
    g = Guarded([(N, np.int32), (N * A, np.float32)])
    explore.sample_behaviour(dl.ptr, N, A, tau, de.ptr if de else None, seed, draw, g.ptr[0], g.ptr[1],
                             dc.ptr if count else None)
    hip.synchronize()
    out = g.read(("actions", "mu"))  # asserts the guards
    bad = int(dc.download(np.int32, (1,))[0])
    for b in (dl, de, dc):
        if b is not None:
            b.free()
    g.free()
    return out["actions"], out["mu"].reshape(N, A), bad


KERNEL_CASES = [(N, A, tau, 3.0) for N in (5, 257, 4096) for A in (2, 8, 9, 18, 19, 32, 33, 64) for tau in (0.25, 1.0, 4.0)]
KERNEL_CASES += [(N, 64, 0.5, 8.0) for N in (5, 257, 4096)]  # p underflows on epsilon = 0 rows


@pytest.mark.parametrize("N,A,tau,sigma", KERNEL_CASES)
def test_kernel_matches_the_reference(N, A, tau, sigma):
    logits, eps, seed, draw, (want, near, mu_ref) = kernel_case(N, A, tau, sigma)
    if N == 4096:  # the reference alone: enough draws for a fraction
        assert near.mean() <= 0.01, near.mean()
        if sigma == 8.0:
            z = (logits.astype(np.float64) - logits.max(1, keepdims=True)) / tau
            assert (z[eps == 0].min(1) < np.log(2.0 ** -126)).any(), "no p underflows on an epsilon = 0 row"
    act, mu, bad = device_behaviour(logits, tau, eps, seed, draw)
    assert bad == 0 and act.min() >= 0 and act.max() < A
    err = np.abs(mu.astype(np.float64) - mu_ref)
    frac = (err / mu_bound(A, mu_ref)).max()
    print(f"behaviour N={N} A={A} tau={tau} sigma={sigma}: near {int(near.sum())}, differing "
          f"{int((act != want).sum())}, worst mu error {err.max():.3e} = {frac:.3f} of the bound")
    check_sampled(act, want, near, f"N={N} A={A} tau={tau}")
    assert np.isfinite(mu).all()
    assert frac <= 1.0, frac
    ones = eps == 1.0
    assert (mu[ones] == mu[ones][:, :1]).all(), "epsilon = 1: every mu of the row is equal"


def test_an_epsilon_whose_floor_rounds_to_zero_is_epsilon_zero():
    """eps = 2^-149: (eps Z) / A is 0 in fp32, so the row is drawn and recorded as with eps = 0, and mu
    stays finite where p underflows; eps = 2^-126 has a floor and keeps the other formula."""
    logits, _, seed, draw, _ = kernel_case(257, 64, 0.5, 8.0)
    logits = logits.copy()
    logits[:, 5] = logits.max(1) - 120.0  # expf(-240) is 0 in fp32
    N = logits.shape[0]
    act0, mu0, _ = device_behaviour(logits, 0.5, np.zeros(N, np.float32), seed, draw)
    act, mu, bad = device_behaviour(logits, 0.5, np.full(N, 2.0 ** -149, np.float32), seed, draw)
    assert bad == 0 and np.isfinite(mu).all()
    np.testing.assert_array_equal(act, act0)
    np.testing.assert_array_equal(mu.view(np.uint32), mu0.view(np.uint32))
    _, mu2, _ = device_behaviour(logits, 0.5, np.full(N, 2.0 ** -126, np.float32), seed, draw)
    assert np.isfinite(mu2).all() and (mu2[:, 5] > mu0[:, 5] + 100).all()


# ------------------------------------------------------------------ 2. tau = 1, epsilon NULL
@pytest.mark.parametrize("N,A", [(5, 2), (257, 18), (100, 64), (4096, 9)])
def test_tau_one_without_epsilon_draws_what_the_plain_sampler_draws(N, A):
    from test_gpu_actor import device_sample
    logits = (2.0 * np.random.RandomState(10 * N + A).standard_normal((N, A))).astype(np.float32)
    logits[0, (A - 1) // 2] = logits[0, A - 1] = logits[0].max() + 1.0  # a tie of the maximum
    seed = 0x5EED0000 + N
    for draw in (0, 5, 2 ** 40):
        want, _ = device_sample(logits, "sample", seed, draw)
        act, mu, bad = device_behaviour(logits, 1.0, None, seed, draw, count=draw != 5)
        assert bad == 0
        np.testing.assert_array_equal(act, want, err_msg=f"draw {draw}")
        act0, mu0, _ = device_behaviour(logits, 1.0, np.zeros(N, np.float32), seed, draw)
        np.testing.assert_array_equal(act0, want, err_msg=f"draw {draw}, epsilons of 0")
        np.testing.assert_array_equal(mu0.view(np.uint32), mu.view(np.uint32))
    ref = log_softmax(logits)  # softmax(mu) = softmax(logits): mu is a log-softmax already
    frac = (np.abs(mu - ref) / mu_bound(A, ref)).max()
    print(f"tau = 1, no epsilon, N={N} A={A}: worst mu error {frac:.3f} of the bound")
    assert frac <= 1.0
    assert (np.abs(log_softmax(mu) - ref) <= mu_bound(A, ref)).all()


# ------------------------------------------------------------------ 3. non-finite rows
def test_nonfinite_rows_copy_the_logits_through():
    logits, eps, seed, draw, _ = kernel_case(257, 18, 0.25, 3.0)
    l = logits.copy()
    l[9, 4] = np.nan
    l[40, 2] = np.inf
    l[256, 17] = -np.inf
    e = np.minimum(eps, 0.4 ** 4).astype(np.float32)
    act, mu, bad = device_behaviour(l, 0.25, e, seed, draw)
    assert bad == 3 and act[9] == 0 and act[40] == 0 and act[256] == 0
    for r in (9, 40, 256):
        np.testing.assert_array_equal(mu[r].view(np.uint32), l[r].view(np.uint32), err_msg=f"row {r}")
    # the neighbours are what they are without the bad rows
    fine = l.copy()
    fine[[9, 40, 256]] = logits[[9, 40, 256]]
    act2, mu2, bad2 = device_behaviour(fine, 0.25, e, seed, draw)
    rest = np.ones(257, bool)
    rest[[9, 40, 256]] = False
    assert bad2 == 0
    np.testing.assert_array_equal(act[rest], act2[rest])
    np.testing.assert_array_equal(mu[rest].view(np.uint32), mu2[rest].view(np.uint32))
    assert np.isfinite(mu[rest]).all()
    act3, mu3, _ = device_behaviour(l, 0.25, e, seed, draw, count=False)  # the counter is optional
    np.testing.assert_array_equal(act3, act)
    np.testing.assert_array_equal(mu3.view(np.uint32), mu.view(np.uint32))


# ------------------------------------------------------------------ 4. the handle
HN = 4
MLP_D, MLP_H = 7, 16
_params = {}


def params(arch, A, T=3):
    if (arch, A) not in _params:
        from freeimpala_amd.learner import DeviceLearner
        if arch == "atari":
            L = DeviceLearner("atari", seq_len=T, batch=HN, num_actions=A, records="planes", seed=11)
        else:
            L = DeviceLearner("mlp", seq_len=T, batch=HN, num_actions=A, obs_dim=MLP_D, hidden=MLP_H, seed=11)
        p = L.get_params()
        L.close()
        p.setflags(write=False)
        _params[(arch, A)] = p
    return _params[(arch, A)]


def make_actor(arch, A, seed, mode="sample"):
    from freeimpala_amd.actor import Actor
    a = Actor("atari", HN, num_actions=A, seed=seed, mode=mode) if arch == "atari" else \
        Actor("mlp", HN, num_actions=A, obs_dim=MLP_D, hidden=MLP_H, seed=seed, mode=mode)
    a.set_params(params(arch, A))
    return a


class Feeder:
    """One act call of an actor on given inputs, through the host call or the device call."""

    def __init__(self, arch, device):
        self.arch, self.device = arch, device
        self.g = Guarded([(HN * PLANE, np.uint8), (HN, np.uint8)] if arch == "atari" else [(HN * MLP_D, np.float32)])

    def inputs(self, rs, first):
        if self.arch == "atari":
            return rs.randint(0, 256, (HN, 84, 84)).astype(np.uint8), np.full(HN, first, np.uint8)
        return (3.0 * rs.standard_normal((HN, MLP_D))).astype(np.float32),

    def act(self, a, inp):
        from freeimpala_amd import hip
        if not self.device:
            return a.act_planes(*inp) if self.arch == "atari" else a.act_obs(*inp)
        for p, x in zip(self.g.ptr, inp):
            hip.upload_ptr(p, x)
        if self.arch == "atari":
            a.act_planes_dev(self.g.ptr[0], self.g.ptr[1])
        else:
            a.act_obs_dev(self.g.ptr[0])
        return a.read_outputs()

    def free(self):
        self.g.free()


def bits_equal(got, want, what):
    assert got.keys() == want.keys(), (what, got.keys(), want.keys())
    for nm in want:
        assert got[nm].dtype == want[nm].dtype
        np.testing.assert_array_equal(got[nm].view(np.uint32), want[nm].view(np.uint32), err_msg=f"{what}: {nm}")


def inactive(a):
    st = a.exploration()
    return not st["active"] and st["temperature"] == 1.0 and st["epsilon"].dtype == np.float32 and not st["epsilon"].any()


def check_explored(out, plain, tau, eps, seed, draw, what):
    """An exploring call against the reference on the policy logits it returned, and its policy
    logits and values against the plain actor's."""
    from freeimpala_amd.explore import behaviour_reference
    A = out["logits"].shape[1]
    for nm in ("logits", "values"):
        np.testing.assert_array_equal(out[nm].view(np.uint32), plain[nm].view(np.uint32), err_msg=f"{what}: {nm}")
    assert "behaviour_logits" in out and "behaviour_logits" not in plain
    want, near, mu_ref = behaviour_reference(out["logits"], tau, eps, seed, draw)
    check_sampled(out["actions"], want, near, what)
    beh = out["behaviour_logits"]
    assert beh.dtype == np.float32 and beh.shape == out["logits"].shape
    frac = (np.abs(beh - mu_ref) / mu_bound(A, mu_ref)).max()
    assert frac <= 1.0, (what, frac)
    assert (beh != out["logits"]).any(), what
    return frac


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("arch,A", [("mlp", 5), ("atari", 3), ("atari", 18)])
def test_handle_explores_and_goes_back_to_the_plain_draw(arch, A, device):
    seed = 23
    ex, plain = make_actor(arch, A, seed), make_actor(arch, A, seed)
    f = Feeder(arch, device)
    rs = np.random.RandomState(90 + A)
    eps = np.array([0.0, 0.3, 1.0, 0.4 ** 8], np.float32)
    assert inactive(ex)
    worst, draw = 0.0, 0

    def both():
        nonlocal draw
        inp = f.inputs(rs, draw == 0)
        o, p = f.act(ex, inp), f.act(plain, inp)
        draw += 1
        return o, p

    ex.set_exploration(2.0, eps)
    st = ex.exploration()
    assert st["active"] and st["temperature"] == 2.0 and (st["epsilon"] == eps).all()
    for _ in range(2):
        o, p = both()
        worst = max(worst, check_explored(o, p, 2.0, eps, seed, draw - 1, f"call {draw - 1}"))
    ex.clear_exploration()
    assert inactive(ex)
    o, p = both()
    bits_equal(o, p, "after clear_exploration")  # the draw has stayed in step
    ex.set_exploration(0.5, 0.25)  # a scalar epsilon
    assert (ex.exploration()["epsilon"] == np.float32(0.25)).all()
    o, p = both()
    worst = max(worst, check_explored(o, p, 0.5, np.full(HN, 0.25, np.float32), seed, draw - 1, f"call {draw - 1}"))
    ex.set_exploration(1.0, np.zeros(HN, np.float32))  # the same as clear
    assert inactive(ex)
    o, p = both()
    bits_equal(o, p, "after set_exploration(1, zeros)")
    ex.set_exploration(1.0)  # no epsilon either: inactive as well
    assert inactive(ex)
    # greedy mode ignores the exploration
    ex.set_exploration(2.0, eps)
    ex.set_mode("greedy")
    plain.set_mode("greedy")
    o, p = both()
    bits_equal(o, p, "greedy")
    np.testing.assert_array_equal(o["actions"], o["logits"].argmax(1))
    ex.set_mode("sample")
    plain.set_mode("sample")
    o, p = both()
    worst = max(worst, check_explored(o, p, 2.0, eps, seed, draw - 1, "sample mode again"))
    print(f"handle {arch} A={A} {'dev' if device else 'host'}: worst mu error {worst:.3f} of the bound")
    f.free()
    ex.close()
    plain.close()


def test_a_cleared_handle_reports_nonfinite_rows_as_a_plain_one():
    """The act call's own message survives the look for behaviour logits, and the outputs ride on it."""
    from freeimpala_amd._abi import FiError
    p = params("mlp", 5).copy()
    p[-6:] = np.nan  # the heads' biases: every logit and value
    obs = np.zeros((HN, MLP_D), np.float32)
    a = make_actor("mlp", 5, 3)
    a.set_params(p)
    for state in ("explored", "cleared", "greedy"):
        if state == "explored":
            a.set_exploration(2.0, 0.25)
        elif state == "cleared":
            a.clear_exploration()
        else:
            a.set_exploration(2.0, 0.25)
            a.set_mode("greedy")
        with pytest.raises(FiError, match=rf"rc=-7: .*{HN} of {HN} rows") as ei:
            a.act_obs(obs)
        out = ei.value.outputs
        assert (out["actions"] == 0).all() and np.isnan(out["logits"]).all()
        assert ("behaviour_logits" in out) == (state == "explored")
        if state == "explored":  # a non-finite row's mu is the policy's logits
            assert np.isnan(out["behaviour_logits"]).all()
    a.close()


# ------------------------------------------------------------------ 5. mu reaches the learner
T, A5, GAMMA, ENV_SEED, ACTOR_SEED = 3, 3, 0.99, 5, 17


def drive(actor, e, steps, change=None):
    """`steps` steps of device Catch under the actor's device calls, one at a time, so that every
    step's tensors can be read: what fi_env_rollout enqueues. change: {step: call before it}."""
    from freeimpala_amd import hip
    t = e.tensors()
    out = dict(planes=[], start=[], logits=[], values=[], act=[], rew=[], disc=[], beh=[])
    for j in range(steps):
        if change and j in change:
            change[j]()
        obs = e.read()
        out["planes"].append(obs["planes"])
        out["start"].append(obs["episode_start"])
        actor.act_planes_dev(t["planes"], t["episode_start"], e.stepped_event)
        o = actor.read_outputs()
        e.step(actor.outputs_dev()["actions"], None, actor.stream)
        if actor.rollout_entry_bytes:
            actor.outcome_dev(t["rewards"], t["discounts"])
        after = e.read()
        out["logits"].append(o["logits"])
        out["values"].append(o["values"])
        out["act"].append(o["actions"])
        out["beh"].append(o.get("behaviour_logits", o["logits"]))
        out["rew"].append(after["rewards"])
        out["disc"].append(after["discounts"])
    return {k: np.stack(v) for k, v in out.items()}


def packed(h, mu):
    from freeimpala_amd.learner import pack_atari_plane_records
    from freeimpala_amd.rollout import split_unrolls
    (u,) = split_unrolls(h["planes"], h["start"], mu, h["act"], h["rew"], h["disc"], T)
    return np.stack([np.frombuffer(x, np.uint8) for x in pack_atari_plane_records(*u)])


def catch_setup(explore):
    from freeimpala_amd import env
    from freeimpala_amd.explore import epsilon_ladder
    a = make_actor("atari", A5, ACTOR_SEED)
    if explore:
        a.set_exploration(2.0, epsilon_ladder(HN))
    a.begin_rollout(T)
    return a, env.CatchEnv(HN, GAMMA, ENV_SEED)


def learner5():
    from freeimpala_amd.learner import DeviceLearner
    L = DeviceLearner("atari", seq_len=T, batch=HN, num_actions=A5, records="planes", optimizer="sgd", lr=1e-3)
    L.set_params(params("atari", A5))
    return L


def learner_tensors(L):
    return dict(logits=L.tensor("logits", shape=(T + 1, HN, A5)), mu=L.tensor("mu", shape=(T, HN, A5)),
                actions=L.tensor("actions", np.int32, (T, HN)), rewards=L.tensor("rewards", shape=(T, HN)),
                discounts=L.tensor("discounts", shape=(T, HN)), values=L.tensor("values", shape=(T + 1, HN)))


def test_behaviour_logits_reach_the_learner(orc):
    from freeimpala_amd.explore import behaviour_reference, epsilon_ladder
    from freeimpala_amd.ring import EntryRing
    eps = epsilon_ladder(HN)
    a, e = catch_setup(True)
    h = drive(a, e, T + 1)
    assert a.rollout_ready()
    entries = a.read_rollout()
    np.testing.assert_array_equal(entries, packed(h, h["beh"]), err_msg="the records hold the behaviour logits")
    assert (entries != packed(h, h["logits"])).any()
    L = learner5()
    st = L.step_rollout(a)
    got = learner_tensors(L)
    # the learner recomputes the policy's logits and ingests the behaviour logits, bit for bit
    np.testing.assert_array_equal(got["logits"].view(np.uint32), h["logits"].view(np.uint32))
    np.testing.assert_array_equal(got["values"].view(np.uint32), h["values"].view(np.uint32))
    np.testing.assert_array_equal(got["mu"].view(np.uint32), h["beh"][:T].view(np.uint32))
    np.testing.assert_array_equal(got["actions"], h["act"][:T])
    np.testing.assert_array_equal(got["rewards"], h["rew"][:T])
    # log pi(a) - log mu(a) from the learner's two tensors against the reference's
    idx = got["actions"][..., None].astype(np.int64)
    log_rho = np.take_along_axis(log_softmax(got["logits"][:T]) - log_softmax(got["mu"]), idx, -1)[..., 0]
    worst = 0.0
    for t in range(T):
        want, near, mu_ref = behaviour_reference(h["logits"][t], 2.0, eps, ACTOR_SEED, t)
        check_sampled(h["act"][t], want, near, f"step {t}")
        ref = np.take_along_axis(log_softmax(h["logits"][t]) - mu_ref, idx[t], -1)[..., 0]
        bound = 2 * np.take_along_axis(mu_bound(A5, mu_ref), idx[t], -1)[..., 0]
        worst = max(worst, (np.abs(log_rho[t] - ref) / bound).max())
        assert (np.abs(log_rho[t] - ref) <= bound).all(), (t, log_rho[t], ref)
    print(f"log rho from the learner's tensors: worst error {worst:.3f} of twice the bound")
    assert (log_rho != 0).all(), "every epsilon of the ladder is > 0"
    # the three losses against the oracle on the tensors the learner ingested
    vt = orc.vtrace_loss(got["logits"][:T], got["mu"], got["actions"], got["rewards"], got["discounts"], got["values"])
    for i, nm in enumerate(("pg_loss", "baseline_loss", "entropy_loss")):
        assert abs(st[nm] - vt["losses"][i]) <= 1e-5 * max(1.0, abs(vt["losses"][i])), (nm, st[nm], vt["losses"][i])
    for nm in ("vs", "pg_adv"):
        err = np.abs(L.tensor(nm, shape=(T, HN)) - vt[nm]).max() / max(1.0, np.abs(vt[nm]).max())
        assert err <= 1e-5, (nm, err)
    first = {k: v.copy() for k, v in got.items()}
    for x in (a, e, L):
        x.close()

    # once more through fi_env_rollout, a ring and step_ring: the same bytes arrive
    a, e = catch_setup(True)
    assert e.rollout(a, T + 1) == T + 1
    np.testing.assert_array_equal(a.read_rollout(), entries, err_msg="fi_env_rollout against the steps one by one")
    ring = EntryRing(a.rollout_entry_bytes, 8, seed=1)
    ring.push_rollout(a)
    L = learner5()
    st2 = L.step_ring(ring)
    got = learner_tensors(L)
    for nm in first:
        np.testing.assert_array_equal(got[nm].view(np.uint32), first[nm].view(np.uint32), err_msg=f"step_ring: {nm}")
    assert st2["total_loss"] == st["total_loss"]
    for x in (a, e, L, ring):
        x.close()

    # the same unroll without exploration: mu is the policy's logits, as ever
    a, e = catch_setup(False)
    assert e.rollout(a, T + 1) == T + 1
    L = learner5()
    L.step_rollout(a)
    got = learner_tensors(L)
    np.testing.assert_array_equal(got["mu"].view(np.uint32), got["logits"][:T].view(np.uint32))
    np.testing.assert_array_equal(got["logits"][0].view(np.uint32), first["logits"][0].view(np.uint32))
    for x in (a, e, L):
        x.close()


# ------------------------------------------------------------------ 6. a change in the middle of an unroll
def test_set_exploration_between_two_steps_of_an_unroll():
    from freeimpala_amd.explore import behaviour_reference, epsilon_ladder
    from freeimpala_amd.learner import unpack_atari_plane_records
    eps = epsilon_ladder(HN)
    a, e = catch_setup(True)  # tau = 2 and the ladder for steps 0 and 1
    h = drive(a, e, T + 1, change={2: lambda: a.set_exploration(0.5, 0.25)})
    entries = a.read_rollout()
    np.testing.assert_array_equal(entries, packed(h, h["beh"]))
    mu = unpack_atari_plane_records(entries, T, HN, A5)[3]
    rules = [(2.0, eps), (2.0, eps), (0.5, np.full(HN, 0.25, np.float32))]
    for t, (tau, ep) in enumerate(rules):
        _, _, mu_ref = behaviour_reference(h["logits"][t], tau, ep, ACTOR_SEED, t)
        assert (np.abs(mu[t] - mu_ref) <= mu_bound(A5, mu_ref)).all(), f"record {t}: its own rule"
        other_tau, other_ep = rules[2] if t < 2 else rules[0]
        _, _, mu_other = behaviour_reference(h["logits"][t], other_tau, other_ep, ACTOR_SEED, t)
        assert (np.abs(mu[t] - mu_other) > mu_bound(A5, mu_other)).any(), f"record {t}: not the other rule"
    a.close()
    e.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_store_nothing():
    from freeimpala_amd import explore, hip
    from freeimpala_amd._abi import FiError
    a = make_actor("mlp", 5, 1)
    eps = np.array([0.1, 0.2, 0.3, 0.4], np.float32)

    def refused(pattern, tau, ep):
        before = a.exploration()
        with pytest.raises(FiError, match=pattern):
            a.set_exploration(tau, ep)
        after = a.exploration()
        assert after["temperature"] == before["temperature"] and after["active"] == before["active"]
        np.testing.assert_array_equal(after["epsilon"], before["epsilon"])

    for state in ("never set", "set"):
        for tau in (0.0, -1.0, float("nan"), 1.0 / 128, 128.0, float("inf")):
            refused(r"rc=-1: .*temperature", tau, eps)
        for i, bad in ((0, -0.1), (2, 1.5), (3, float("nan"))):
            ep = eps.copy()
            ep[i] = bad
            refused(rf"rc=-1: .*epsilon\[{i}\]", 2.0, ep)
        with pytest.raises(ValueError):
            a.set_exploration(2.0, eps[:3])
        a.set_exploration(1.0 / 64, eps)  # the ends of the range are taken
        a.set_exploration(64.0, np.array([0, 1, 0, 1], np.float32))
        a.set_exploration(4.0, eps)
    assert a.exploration()["temperature"] == 4.0
    with pytest.raises(FiError, match=r"rc=-4: .*did not draw"):
        a.behaviour_ptr()
    a.close()

    L = explore.lib()
    for call in (lambda: L.fi_explore_set(None, 1.0, None), lambda: L.fi_explore_clear(None),
                 lambda: L.fi_explore_get(None, None, None, None), lambda: L.fi_explore_read_behaviour(None, None, 0)):
        assert call() == -1

    d = hip.DeviceBuffer(4096)
    mu, act = d.ptr + 1024, d.ptr + 2048
    for A in (1, 65):
        with pytest.raises(FiError, match=r"rc=-1: .*2 <= A <= 64"):
            explore.sample_behaviour(d.ptr, 1, A, 1.0, None, 0, 0, act, mu)
    with pytest.raises(FiError, match=r"rc=-1: .*N must be >= 1"):
        explore.sample_behaviour(d.ptr, 0, 6, 1.0, None, 0, 0, act, mu)
    with pytest.raises(FiError, match=r"rc=-1: .*temperature"):
        explore.sample_behaviour(d.ptr, 1, 6, 0.0, None, 0, 0, act, mu)
    with pytest.raises(FiError, match=r"rc=-1: .*null"):
        explore.sample_behaviour(d.ptr, 1, 6, 1.0, None, 0, 0, act, None)
    for args in ((d.ptr + 2, None, act, mu), (d.ptr, d.ptr + 513, act, mu), (d.ptr, None, act + 1, mu),
                 (d.ptr, None, act, mu + 2)):
        with pytest.raises(FiError, match=r"rc=-1: .*4-byte aligned"):
            explore.sample_behaviour(args[0], 1, 6, 1.0, args[1], 0, 0, args[2], args[3])
    d.free()


# ------------------------------------------------------------------ 8. C++ wrapper
EXE = os.path.join(ROOT, "build", "host_explore_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_explore_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("explore atari:")]
    assert len(lines) == 1 and "mu != logits in" in lines[0]
    assert int(lines[0].split(" in ")[1].split()[0]) > 0
