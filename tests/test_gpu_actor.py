"""Acting on the device (include/fi_actor.h, freeimpala_amd/actor.py): the stack push and the
sampler alone against host references built here (stack_planes; Philox + fp64 numpy), the
forward through an actor handle against the learner's own logits (bit for bit: the same kernels)
and the oracle, the closed loop actor -> plane records -> learner, and the refusals.

Sampling reference: the rule of fi_actor.h in fp64 on the same fp32 logits. The device sums
fp32 expf values, so a draw whose threshold u Z lies within 1e-5 Z of a running sum c_a may land
one index away (fp32 expf plus an 18- to 64-term fp32 running sum is off by about 1e-6 Z; the
margin is roughly 8x that). Every other draw must match exactly, and at most 1 % of a case's
draws may be near (the expectation is about 2e-5 A per draw)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE, FRAME = 84 * 84, 84 * 84 * 4
ST_SAMPLE = 6
NEAR = 1e-5


# ------------------------------------------------------------------ references
def uniforms(orc, seed, draw, N):
    return np.array([(int(orc.philox4(seed, draw * N + i, ST_SAMPLE)[0]) >> 8) * 2.0 ** -24 for i in range(N)])


def ref_sample(orc, logits, seed, draw):
    """(actions, near) of the sampling rule in fp64 on fp32 logits."""
    logits = np.asarray(logits, np.float32)
    N, A = logits.shape
    l = logits.astype(np.float64)
    p = np.exp(l - l.max(1, keepdims=True))
    c = np.cumsum(p, 1)
    Z = c[:, -1]
    thr = uniforms(orc, seed, draw, N) * Z
    over = c > thr[:, None]
    act = np.where(over.any(1), over.argmax(1), A - 1).astype(np.int32)
    near = (np.abs(thr[:, None] - c) <= NEAR * Z[:, None]).any(1)
    return act, near


def check_sampled(got, want, near, what=""):
    """Exact away from every boundary; a near draw may land one index away. (The cap on the
    fraction of near draws is asserted per case, where there are enough draws for a fraction.)"""
    np.testing.assert_array_equal(got[~near], want[~near], err_msg=f"{what}: draws away from every boundary")
    assert (np.abs(got[near].astype(int) - want[near]) <= 1).all(), (what, got[near], want[near])


def rel_l2(got, want):
    return np.linalg.norm(got.astype(np.float64) - want) / max(1e-30, np.linalg.norm(want))


def start_pattern(N, pushes=7):
    """Every env starts at push 0; env 0 restarts at push 2; env N-1 at pushes 4 and 5 (two in a
    row); with N >= 3 the envs between never restart."""
    s = np.zeros((pushes, N), bool)
    s[0] = True
    s[2, 0] = True
    s[4, N - 1] = s[5, N - 1] = True
    return s


# ------------------------------------------------------------------ 1. stack push, standalone
def run_pushes(planes, start, flag_offset=0):
    """fi_push_planes once per step on zeroed stacks between guard bytes; the stacks after every
    push. flag_offset: the flags' device pointer is moved off 4-byte alignment."""
    from freeimpala_amd import actor, hip
    P, N = start.shape
    G = 256
    buf = hip.DeviceBuffer(N * FRAME + 2 * G)
    init = np.zeros(N * FRAME + 2 * G, np.uint8)
    init[:G] = init[G + N * FRAME:] = 0xA5
    buf.upload(init)
    dpl = hip.DeviceBuffer(N * PLANE)
    dfl = hip.DeviceBuffer(N + 8)
    out = []
    for t in range(P):
        dpl.upload(planes[t])
        fl = np.full(N + 8, 0xFF, np.uint8)  # the bytes around the flags are not flags
        fl[flag_offset:flag_offset + N] = start[t]
        dfl.upload(fl)
        actor.push_planes(buf.ptr + G, dpl.ptr, dfl.ptr + flag_offset, N)
        hip.synchronize()
        got = buf.download(np.uint8, (N * FRAME + 2 * G,))
        assert (got[:G] == 0xA5).all() and (got[G + N * FRAME:] == 0xA5).all(), f"push {t}: guard overwritten"
        out.append(got[G:G + N * FRAME].reshape(N, 84, 84, 4))
    for b in (buf, dpl, dfl):
        b.free()
    return out


@pytest.mark.parametrize("N,flag_offset", [(1, 0), (3, 1), (65, 0), (65, 3)])
def test_push_planes_equals_stack_planes(N, flag_offset):
    from freeimpala_amd.learner import stack_planes
    rs = np.random.RandomState(100 + N)
    start = start_pattern(N)
    planes = rs.randint(0, 256, (7, N, 84, 84)).astype(np.uint8)
    want = stack_planes(planes, np.zeros((3, N, 84, 84), np.uint8), start)
    for t, got in enumerate(run_pushes(planes, start, flag_offset)):
        np.testing.assert_array_equal(got, want[t], err_msg=f"push {t}")


def test_push_planes_without_a_start_reads_zero_history():
    from freeimpala_amd.learner import stack_planes
    N = 3
    rs = np.random.RandomState(7)
    start = np.zeros((5, N), bool)
    start[3, 1] = True
    planes = rs.randint(0, 256, (5, N, 84, 84)).astype(np.uint8)
    want = stack_planes(planes, np.zeros((3, N, 84, 84), np.uint8), start)
    got = run_pushes(planes, start)
    assert (got[0][..., :3] == 0).all() and (got[0][..., 3] == planes[0]).all()
    for t in range(5):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"push {t}")


# ------------------------------------------------------------------ 2. sampler, standalone
SAMPLER_SHAPES = [(1, 2), (64, 6), (257, 18), (100, 64)]
DRAW0 = 5  # 4 consecutive draws from here
_sampler_cases = {}


def sampler_case(orc, N, A):
    """fp32 logits N(0, 2^2) from a fixed seed (row 0 of each case holds an exact tie of its
    maximum) and the reference's actions and near flags for 4 consecutive draws; shared."""
    if (N, A) not in _sampler_cases:
        rs = np.random.RandomState(1000 * N + A)
        logits = (2.0 * rs.standard_normal((N, A))).astype(np.float32)
        top = np.float32(logits[0].max() + 1.0)
        logits[0, (A - 1) // 2] = logits[0, A - 1] = top
        seed = 0x5EED0000 + N
        ref = [ref_sample(orc, logits, seed, DRAW0 + k) for k in range(4)]
        logits.setflags(write=False)
        _sampler_cases[(N, A)] = (logits, seed, ref)
    return _sampler_cases[(N, A)]


def device_sample(logits, mode, seed, draw, count=True):
    from freeimpala_amd import actor, hip
    N, A = logits.shape
    dl = hip.DeviceBuffer.from_array(np.ascontiguousarray(logits, np.float32))
    da = hip.DeviceBuffer.from_array(np.full(N + 2, -77, np.int32))  # one guard word on each side
    dc = hip.DeviceBuffer.from_array(np.zeros(1, np.int32))
    actor.sample_actions(dl.ptr, N, A, mode, seed, draw, da.ptr + 4, dc.ptr if count else None)
    hip.synchronize()
    a = da.download(np.int32, (N + 2,))
    bad = int(dc.download(np.int32, (1,))[0])
    for b in (dl, da, dc):
        b.free()
    assert a[0] == -77 and a[-1] == -77, "guard overwritten"
    return a[1:-1], bad


@pytest.mark.parametrize("N,A", SAMPLER_SHAPES)
def test_sampler_matches_the_reference(orc, N, A):
    logits, seed, ref = sampler_case(orc, N, A)
    # the reference alone: the chosen seeds stay under the cap of near draws
    assert np.mean([near for _, near in ref]) <= 0.01
    got = []
    for k, (want, near) in enumerate(ref):
        a, bad = device_sample(logits, "sample", seed, DRAW0 + k)
        assert bad == 0 and a.min() >= 0 and a.max() < A
        print(f"sampler N={N} A={A} draw {DRAW0 + k}: near {int(near.sum())}, differing {int((a != want).sum())}")
        check_sampled(a, want, near, f"N={N} A={A} draw {DRAW0 + k}")
        got.append(a)
    again, _ = device_sample(logits, "sample", seed, DRAW0, count=False)
    np.testing.assert_array_equal(again, got[0])
    if N == 257:
        assert (got[0] != got[1]).any(), "draw + 1 gives another vector"
        other, _ = device_sample(logits, "sample", seed + 1, DRAW0)
        assert (other != got[0]).any(), "another seed gives another vector"


@pytest.mark.parametrize("N,A", SAMPLER_SHAPES)
def test_greedy_is_first_index_argmax(orc, N, A):
    logits, seed, _ = sampler_case(orc, N, A)
    a, bad = device_sample(logits, "greedy", seed, DRAW0)
    np.testing.assert_array_equal(a, logits.argmax(1))
    assert a[0] == (A - 1) // 2 and logits[0, (A - 1) // 2] == logits[0, A - 1] and bad == 0  # the tie: its first index


@pytest.mark.parametrize("mode", ["sample", "greedy"])
def test_nonfinite_rows_get_action_zero_and_are_counted(orc, mode):
    logits, seed, ref = sampler_case(orc, 64, 6)
    l = logits.copy()
    l[:, 0] -= 50.0  # action 0 is not what a finite row draws
    l[9, 4] = np.nan
    l[40, 2] = np.inf
    a, bad = device_sample(l, mode, seed, DRAW0)
    assert bad == 2 and a[9] == 0 and a[40] == 0
    rest = np.ones(64, bool)
    rest[[9, 40]] = False
    assert (a[rest] != 0).all()
    a2, _ = device_sample(l, mode, seed, DRAW0, count=False)  # the counter is optional
    np.testing.assert_array_equal(a2, a)


# ------------------------------------------------------------------ 3. Atari forward through the handle
_atari = {}


def atari_learner_run():
    """One Atari learner step at 16 rows (T = 1, B = 8, A = 18) from synthetic frames: p0, the
    frames and the logits / values the step computed with p0. Shared, read-only."""
    if not _atari:
        from freeimpala_amd.learner import DeviceLearner
        L = DeviceLearner("atari", seq_len=1, batch=8, optimizer="sgd")
        L.synth(seed=5)
        p0 = L.get_params()
        frames = L.tensor("frames", np.uint8, (16, 84, 84, 4))
        L.step_resident()
        out = dict(p0=p0, frames=frames, logits=L.tensor("logits", shape=(16, 18)), values=L.tensor("values", shape=(16,)))
        L.close()
        for v in out.values():
            v.setflags(write=False)
        _atari.update(out)
    return _atari


def oracle_rows(orc):
    """The oracle's bf16-emulating forward on 257 random frames with p0, once."""
    if "ref" not in _atari:
        run = atari_learner_run()
        frames = np.random.RandomState(31).randint(0, 256, (257, 84, 84, 4)).astype(np.uint8)
        ref = orc.atari_forward(frames, run["p0"], A=18, bf16_emul=True)["out"]
        frames.setflags(write=False)
        ref.setflags(write=False)
        _atari["ref_frames"], _atari["ref"] = frames, ref
    return _atari["ref_frames"], _atari["ref"]


def test_atari_actor_logits_equal_the_learners(orc):
    from freeimpala_amd.actor import Actor
    run = atari_learner_run()
    a = Actor("atari", 16, seed=3)
    assert a.param_count == run["p0"].size
    a.set_params(run["p0"], version=4)
    assert a.version == 4
    a.seed(3, draw=9)
    out = a.act_frames(run["frames"])
    np.testing.assert_array_equal(out["logits"], run["logits"])
    np.testing.assert_array_equal(out["values"], run["values"])
    want, near = ref_sample(orc, out["logits"], 3, 9)
    check_sampled(out["actions"], want, near, "act_frames")
    out2 = a.act_frames(run["frames"])  # the next call: draw 10
    np.testing.assert_array_equal(out2["logits"], out["logits"])
    want2, near2 = ref_sample(orc, out["logits"], 3, 10)
    check_sampled(out2["actions"], want2, near2, "act_frames, next draw")
    a.set_mode("greedy")
    np.testing.assert_array_equal(a.act_frames(run["frames"])["actions"], out["logits"].argmax(1))
    a.close()


@pytest.mark.parametrize("N", [1, 3, 257])  # 257: one more frame than the 256 persistent workgroups
def test_atari_actor_against_the_oracle(orc, N):
    from freeimpala_amd.actor import Actor
    run = atari_learner_run()
    frames, ref = oracle_rows(orc)
    a = Actor("atari", N, seed=21)
    a.set_params(run["p0"])
    out = a.act_frames(frames[:N])
    e_l, e_v = rel_l2(out["logits"], ref[:N, :18]), rel_l2(out["values"], ref[:N, 18])
    print(f"atari actor N={N}: rel L2 logits {e_l:.2e} values {e_v:.2e}")
    assert e_l <= 2e-3 and e_v <= 2e-3
    want, near = ref_sample(orc, out["logits"], 21, 0)
    if N >= 100:
        assert near.mean() <= 0.01
    check_sampled(out["actions"], want, near, f"N={N}")
    a.close()


# ------------------------------------------------------------------ 4. bf16 blob
def test_bf16_blob_matches_a_learner_that_loaded_it():
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    P = DeviceLearner("atari", seq_len=1, batch=8, optimizer="sgd", publish="bf16", seed=13)
    blob, _ = P.get_blob()
    assert len(blob) == 2 * P.param_count
    P.close()
    L = DeviceLearner("atari", seq_len=1, batch=8, optimizer="sgd", lr=0.0)
    L.set_params(blob, version=7)
    L.synth(seed=6)
    frames = L.tensor("frames", np.uint8, (16, 84, 84, 4))
    L.step_resident()
    a = Actor("atari", 16)
    a.set_params(blob, version=7)
    assert a.version == 7
    out = a.act_frames(frames)
    np.testing.assert_array_equal(out["logits"], L.tensor("logits", shape=(16, 18)))
    np.testing.assert_array_equal(out["values"], L.tensor("values", shape=(16,)))
    a.close()
    L.close()


# ------------------------------------------------------------------ 5. closed loop with plane records
def test_closed_loop_actor_records_learner(orc):
    """An actor acts T+1 times on planes; its own logits and actions go into plane records; the
    learner that ingests them rebuilds the actor's stacks and recomputes its logits bit for bit
    (4 rows in the actor, 16 in the learner: no forward kernel's row depends on the row count),
    so pi = mu exactly and the V-trace targets are the oracle's at pi = mu."""
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner, pack_atari_plane_records, stack_planes
    A, T, B = 6, 3, 4
    L = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, records="planes", optimizer="sgd", lr=0.0)
    p0 = L.get_params()
    actor = Actor("atari", B, num_actions=A, seed=17)
    actor.set_params(p0)
    rs = np.random.RandomState(55)
    planes = rs.randint(0, 256, (T + 1, B, 84, 84)).astype(np.uint8)
    start = np.zeros((T + 1, B), bool)
    start[0] = True
    start[2, 2] = True
    history = np.zeros((3, B, 84, 84), np.uint8)
    want_frames = stack_planes(planes, history, start)
    outs = []
    for t in range(T + 1):
        outs.append(actor.act_planes(planes[t], start[t]))
        np.testing.assert_array_equal(actor.stacks(), want_frames[t], err_msg=f"stacks after call {t}")
        want, near = ref_sample(orc, outs[t]["logits"], 17, t)
        check_sampled(outs[t]["actions"], want, near, f"call {t}")
    mu = np.stack([o["logits"] for o in outs[:T]])
    act = np.stack([o["actions"] for o in outs[:T]])
    rew = rs.randint(-1, 2, (T, B)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.2)).astype(np.float32)
    L.set_params(p0)
    L.step(pack_atari_plane_records(planes, history, start, mu, act, rew, disc))
    np.testing.assert_array_equal(L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4)), want_frames)
    logits = L.tensor("logits", shape=(T + 1, B, A))
    values = L.tensor("values", shape=(T + 1, B))
    for t in range(T + 1):
        np.testing.assert_array_equal(logits[t], outs[t]["logits"], err_msg=f"logits of call {t}")
        np.testing.assert_array_equal(values[t], outs[t]["values"], err_msg=f"values of call {t}")
    np.testing.assert_array_equal(L.tensor("mu", shape=(T, B, A)), logits[:T])
    vt = orc.vtrace_loss(logits[:T], mu, act, rew, disc, values)
    for nm in ("vs", "pg_adv"):
        got = L.tensor(nm, shape=(T, B))
        err = np.abs(got - vt[nm]).max() / max(1.0, np.abs(vt[nm]).max())
        assert err <= 1e-5, (nm, err)
    actor.close()
    L.close()


# ------------------------------------------------------------------ 6. MLP
def test_mlp_actor_equals_the_learner_and_the_oracle(orc):
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    T, B, A, D, H = 1, 5, 64, 128, 256
    L = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, obs_dim=D, hidden=H, optimizer="sgd")
    L.synth(seed=8)
    p0 = L.get_params()
    obs = L.tensor("obs", shape=(10, D))
    L.step_resident()
    a = Actor("mlp", 10, num_actions=A, obs_dim=D, hidden=H, seed=2)
    a.set_params(p0)
    out = a.act_obs(obs)
    np.testing.assert_array_equal(out["logits"], L.tensor("logits", shape=(10, A)))
    np.testing.assert_array_equal(out["values"], L.tensor("values", shape=(10,)))
    want, near = ref_sample(orc, out["logits"], 2, 0)
    check_sampled(out["actions"], want, near, "act_obs")
    a.close()
    L.close()
    one = Actor("mlp", 1, num_actions=A, obs_dim=D, hidden=H, mode="greedy")
    one.set_params(p0)
    o1 = one.act_obs(obs[3:4])
    ref = orc.mlp_forward(obs[3:4], p0, H=H, A=A)[2]
    assert np.abs(o1["logits"] - ref[:, :A]).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(o1["values"] - ref[:, A]).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert o1["actions"][0] == o1["logits"][0].argmax()
    one.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    from freeimpala_amd import actor, hip
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.actor import Actor
    run = atari_learner_run()
    at = Actor("atari", 2)
    obs = np.zeros((2, 128), np.float32)
    frames = np.zeros((2, 84, 84, 4), np.uint8)
    with pytest.raises(FiError, match=r"rc=-4: .*no parameters"):  # before set_params
        at.act_frames(frames)
    with pytest.raises(FiError, match=r"rc=-4: .*no parameters"):
        at.act_planes(frames[..., 0], [1, 1])
    with pytest.raises(FiError, match=r"rc=-1: .*Atari handle"):
        at.act_obs(obs)
    with pytest.raises(FiError, match=rf"rc=-1: .*{4 * run['p0'].size}.*{2 * run['p0'].size}"):
        at.set_params(run["p0"][:-1])
    assert at.version == 0
    at.set_params(run["p0"], version=1)
    with pytest.raises(FiError, match=r"rc=-1: .*Atari handle"):
        at.act_obs(obs)
    with pytest.raises(FiError, match=r"rc=-1: .*unknown mode"):
        at.set_mode(2)
    with pytest.raises(ValueError):
        at.act_frames(frames[:1])
    at.act_frames(frames)  # and the handle still works
    at.close()

    ml = Actor("mlp", 2, num_actions=6, obs_dim=8, hidden=16)
    with pytest.raises(FiError, match=r"rc=-4: .*no parameters"):
        ml.act_obs(np.zeros((2, 8), np.float32))
    with pytest.raises(FiError, match=r"rc=-1: .*MLP handle"):
        ml.act_planes(frames[..., 0], [0, 0])
    with pytest.raises(FiError, match=r"rc=-1: .*MLP handle"):
        ml.act_frames(frames)
    with pytest.raises(FiError, match=r"rc=-1: .*Atari handle has stacks"):
        ml.stacks()
    ml.close()

    with pytest.raises(FiError, match=r"rc=-1: .*num_envs"):
        Actor("atari", 0)
    with pytest.raises(FiError, match=r"rc=-1: .*num_envs"):
        Actor("mlp", 0)
    with pytest.raises(FiError, match=r"rc=-1: .*18"):
        Actor("atari", 2, num_actions=19)
    with pytest.raises(FiError, match=r"rc=-1: .*64"):
        Actor("mlp", 2, num_actions=65)
    with pytest.raises(ValueError):
        Actor("atari", 2, mode="epsilon")

    d = hip.DeviceBuffer(FRAME + PLANE + 16)
    with pytest.raises(FiError, match=r"rc=-1: .*N must be >= 1"):
        actor.push_planes(d.ptr, d.ptr + FRAME, d.ptr + FRAME + PLANE, 0)
    with pytest.raises(FiError, match=r"rc=-1: .*aligned"):
        actor.push_planes(d.ptr + 4, d.ptr + FRAME, d.ptr + FRAME + PLANE, 1)
    with pytest.raises(FiError, match=r"rc=-1: .*null"):
        actor.push_planes(d.ptr, None, d.ptr + FRAME + PLANE, 1)
    with pytest.raises(FiError, match=r"rc=-1: .*2 <= A <= 64"):
        actor.sample_actions(d.ptr, 1, 65, "sample", 0, 0, d.ptr + 1024)
    with pytest.raises(FiError, match=r"rc=-1: .*N must be >= 1"):
        actor.sample_actions(d.ptr, 0, 6, "sample", 0, 0, d.ptr + 1024)
    d.free()


def test_nonfinite_params_report_and_still_fill_the_outputs():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.actor import Actor
    run = atari_learner_run()
    p = run["p0"].copy()
    p[-19:] = np.nan  # the heads' biases: every logit and value
    a = Actor("atari", 16)
    a.set_params(p)
    with pytest.raises(FiError, match=r"rc=-7: .*16 of 16 rows") as ei:
        a.act_frames(run["frames"])
    out = ei.value.outputs
    assert (out["actions"] == 0).all() and np.isnan(out["logits"]).all() and np.isnan(out["values"]).all()
    a.set_params(run["p0"])  # a good blob repairs the handle
    np.testing.assert_array_equal(a.act_frames(run["frames"])["logits"], run["logits"])
    a.close()


# ------------------------------------------------------------------ 8. C++ wrapper
EXE = os.path.join(ROOT, "build", "host_actor_check")
_cpp_runs = []


def run_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_actor_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("actions ")]
    _cpp_runs.append(lines)
    return lines


def test_cpp_wrapper_acts():
    lines = run_check_program()
    assert len(lines) == 2 and lines[0].startswith("actions mlp:") and lines[1].startswith("actions atari:")
    mlp = [[int(x) for x in part.split()] for part in lines[0].split(":")[1].split("|")]
    atari = [[int(x) for x in part.split()] for part in lines[1].split(":")[1].split("|")]
    assert [len(x) for x in mlp] == [5, 5] and all(0 <= v < 18 for x in mlp for v in x)
    assert [len(x) for x in atari] == [3, 3] and all(0 <= v < 6 for x in atari for v in x)


def test_cpp_wrapper_is_deterministic():
    first = _cpp_runs[0] if _cpp_runs else run_check_program()
    assert run_check_program() == first
