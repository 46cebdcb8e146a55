"""Device-resident environments (include/fi_env.h): the built-in Catch environment against
catch_reference byte for byte (the handle, and its two kernels alone between guard bands), device
act calls against host act calls on the same bytes, a recording actor driven by fi_env_rollout
against the packer on the host's rebuild of the same steps, a learner that steps from such an
unroll against one that steps from the host-packed entries, two unrolls enqueued without a host
wait against the same steps waited for one by one, and the refusals.

No comparison has a tolerance: everything compared is integer data, or the output of the same
kernel on the same bytes."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_ring import Guarded, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, A, T, GAMMA = 5, 4, 3, 0.99  # N: odd and below a wave; A = 4: a mod 3 wraps
PLANE = 84 * 84
MLP_N, MLP_D, MLP_H, MLP_A = 3, 7, 16, 4
ENV_SEED, ACTOR_SEED = 5, 17


def dev(a):
    from freeimpala_amd import hip
    return hip.DeviceBuffer.from_array(np.ascontiguousarray(a))


# ------------------------------------------------------------------ 1. environment parity
def test_environment_equals_catch_reference_for_45_steps():
    from freeimpala_amd import env, hip
    ref = env.catch_reference(N, GAMMA, ENV_SEED)
    e = env.CatchEnv(N, GAMMA, ENV_SEED)
    # the two kernels alone, on buffers between guards: state, planes, episode_start, rewards, discounts, totals
    g = Guarded([(4 * N, np.uint32), (N * PLANE, np.uint8), (N, np.uint8), (N, np.float32), (N, np.float32),
                 (2, np.uint64)])
    names = ("state", "planes", "episode_start", "rewards", "discounts", "totals")
    s0 = ref.state()
    hip.upload_ptr(g.ptr[0], np.stack([s0["r"], s0["c"], s0["p"], s0["k"].astype(np.int32)], 1).astype(np.uint32))
    hip.upload_ptr(g.ptr[5], np.zeros(2, np.uint64))
    actions = np.random.RandomState(1).randint(0, A, (45, N)).astype(np.int32)
    d_act = hip.DeviceBuffer(N * 4)

    def check_handle(t):
        got, st = e.read(), e.state()
        for nm in ("planes", "episode_start", "rewards", "discounts"):
            np.testing.assert_array_equal(got[nm], getattr(ref, nm), err_msg=f"step {t}: {nm}")
        for nm, want in ref.state().items():
            np.testing.assert_array_equal(st[nm], want, err_msg=f"step {t}: {nm}")
            assert st[nm].dtype == want.dtype
        assert e.stats() == dict(episodes=ref.episodes, return_sum=ref.return_sum), t

    check_handle(-1)  # the first observation: Reset(i, 0), episode_start = 1
    assert (e.read()["episode_start"] == 1).all()
    for t in range(45):
        d_act.upload(actions[t])
        e.step(d_act.ptr)
        env.env_update(g.ptr[0], d_act.ptr, N, GAMMA, ENV_SEED, g.ptr[2], g.ptr[3], g.ptr[4], g.ptr[5])
        env.env_render(g.ptr[0], g.ptr[1], N)
        hip.synchronize()
        ref.step(actions[t])
        check_handle(t)
        got = g.read(names)  # asserts the guards
        want = ref.state()
        np.testing.assert_array_equal(got["state"].reshape(N, 4),
                                      np.stack([want["r"], want["c"], want["p"], want["k"].astype(np.int32)], 1).astype(np.uint32))
        np.testing.assert_array_equal(got["planes"].reshape(N, 84, 84), ref.planes, err_msg=f"step {t}")
        np.testing.assert_array_equal(got["episode_start"], ref.episode_start)
        np.testing.assert_array_equal(got["rewards"], ref.rewards)
        np.testing.assert_array_equal(got["discounts"], ref.discounts)
        assert int(got["totals"][0]) == ref.episodes and int(got["totals"].view(np.int64)[1]) == ref.return_sum
    assert ref.episodes == 2 * N and (ref.k == 2).all(), "two resets per environment"
    g.free()
    d_act.free()
    e.close()


def test_render_fills_more_than_one_block():
    """N = 300: 132,300 pieces, 517 workgroups, the last one's lanes 204 .. 255 idle; states at the
    corners of the grid."""
    from freeimpala_amd import env, hip
    n = 300
    ref = env.catch_reference(n, GAMMA, 9)
    rs = np.random.RandomState(2)
    ref.r[:] = rs.randint(0, 20, n)
    ref.c[:] = rs.randint(0, 21, n)
    ref.p[:] = rs.randint(1, 20, n)
    ref.r[:4], ref.c[:4], ref.p[:4] = (0, 0, 19, 19), (0, 20, 0, 20), (1, 19, 1, 19)
    g = Guarded([(4 * n, np.uint32), (n * PLANE, np.uint8)])
    hip.upload_ptr(g.ptr[0], np.stack([ref.r, ref.c, ref.p, np.zeros(n, np.int32)], 1).astype(np.uint32))
    env.env_render(g.ptr[0], g.ptr[1], n)
    hip.synchronize()
    np.testing.assert_array_equal(g.read(("state", "planes"))["planes"].reshape(n, 84, 84), ref.render())
    g.free()


# ------------------------------------------------------------------ 2. act parity
def atari_params():
    from freeimpala_amd.learner import DeviceLearner
    L = DeviceLearner("atari", seq_len=T, batch=N, num_actions=A, records="planes")
    p0 = L.get_params()
    L.close()
    return p0


_p0 = {}


def p0_atari():
    if "p" not in _p0:
        _p0["p"] = atari_params()
    return _p0["p"]


def outputs_equal(got, want, what):
    for nm in ("actions", "logits", "values"):
        assert got[nm].dtype == want[nm].dtype
        np.testing.assert_array_equal(got[nm].view(np.uint32), want[nm].view(np.uint32), err_msg=f"{what}: {nm}")


def test_device_act_calls_equal_host_act_calls_atari():
    from freeimpala_amd.actor import Actor
    calls = 6
    rs = np.random.RandomState(3)
    planes = rs.randint(0, 256, (calls, N, 84, 84)).astype(np.uint8)
    start = np.zeros((calls, N), np.uint8)
    start[0] = 1
    start[3, 1] = start[3, 4] = 1  # an episode start in the middle
    host, devc, mixed = (Actor("atari", N, num_actions=A, seed=ACTOR_SEED) for _ in range(3))
    for a in (host, devc, mixed):
        a.set_params(p0_atari())
    assert devc.outputs_dev()["done_event"] is None
    d_planes, d_start = Guarded([(N * PLANE, np.uint8)]), Guarded([(N, np.uint8)])
    from freeimpala_amd import hip
    for j in range(calls):
        want = host.act_planes(planes[j], start[j])
        hip.upload_ptr(d_planes.ptr[0], planes[j])
        hip.upload_ptr(d_start.ptr[0], start[j])
        devc.act_planes_dev(d_planes.ptr[0], d_start.ptr[0])
        assert devc.outputs_dev()["done_event"] is not None
        outputs_equal(devc.read_outputs(), want, f"call {j}")
        np.testing.assert_array_equal(devc.stacks(), host.stacks(), err_msg=f"call {j}")
        if j % 2:  # host and device calls alternate on one handle
            got = mixed.act_planes(planes[j], start[j])
        else:
            mixed.act_planes_dev(d_planes.ptr[0], d_start.ptr[0])
            got = mixed.read_outputs()
        outputs_equal(got, want, f"alternating, call {j}")
        np.testing.assert_array_equal(mixed.stacks(), host.stacks(), err_msg=f"alternating, call {j}")
        # the caller's buffers are read only
        np.testing.assert_array_equal(d_planes.read(("planes",))["planes"], planes[j].reshape(-1))
        np.testing.assert_array_equal(d_start.read(("start",))["start"], start[j])
    assert len({tuple(host.act_planes(planes[0], start[0])["actions"]) for _ in range(4)}) > 1, "draw advances"
    for h in (host, devc, mixed):
        h.close()
    d_planes.free()
    d_start.free()


def test_device_act_calls_equal_host_act_calls_mlp():
    from freeimpala_amd import hip
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    L = DeviceLearner("mlp", seq_len=T, batch=MLP_N, num_actions=MLP_A, obs_dim=MLP_D, hidden=MLP_H)
    p0 = L.get_params()
    L.close()
    host, devc, mixed = (Actor("mlp", MLP_N, num_actions=MLP_A, obs_dim=MLP_D, hidden=MLP_H, seed=ACTOR_SEED)
                         for _ in range(3))
    for a in (host, devc, mixed):
        a.set_params(p0)
    rs = np.random.RandomState(4)
    d_obs = Guarded([(MLP_N * MLP_D, np.float32)])
    for j in range(6):
        obs = rs.standard_normal((MLP_N, MLP_D)).astype(np.float32)
        want = host.act_obs(obs)
        hip.upload_ptr(d_obs.ptr[0], obs)
        devc.act_obs_dev(d_obs.ptr[0])
        outputs_equal(devc.read_outputs(), want, f"call {j}")
        if j % 2:
            got = mixed.act_obs(obs)
        else:
            mixed.act_obs_dev(d_obs.ptr[0])
            got = mixed.read_outputs()
        outputs_equal(got, want, f"alternating, call {j}")
        np.testing.assert_array_equal(d_obs.read(("obs",))["obs"], obs.reshape(-1))
    for h in (host, devc, mixed):
        h.close()
    d_obs.free()


# ------------------------------------------------------------------ the shared run of tests 3 and 4
STEPS, PRE_STEPS = 3 * T + 1, 15
_run = {}

LEARNER_TENSORS = (("frames", np.uint8), ("mu", np.float32), ("actions", np.int32), ("rewards", np.float32),
                   ("discounts", np.float32), ("logits", np.float32), ("vs", np.float32), ("grads", np.float32))


def snapshot(L, stats):
    d = {nm: L.tensor(nm, dt) for nm, dt in LEARNER_TENSORS}
    d["params"] = L.get_params()
    d["stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    return d


def make_learner():
    from freeimpala_amd.learner import DeviceLearner
    return DeviceLearner("atari", seq_len=T, batch=N, num_actions=A, records="planes", optimizer="adam", lr=1e-3)


def host_steps(actor, ref, steps):
    """`steps` steps of a host-driven actor on catch_reference: what every step held."""
    out = dict(planes=[], start=[], mu=[], act=[], rew=[], disc=[])
    for _ in range(steps):
        out["planes"].append(ref.planes.copy())
        out["start"].append(ref.episode_start.copy())
        o = actor.act_planes(ref.planes, ref.episode_start)
        ref.step(o["actions"])
        if actor.rollout_entry_bytes:
            actor.outcome(ref.rewards, ref.discounts)
        out["mu"].append(o["logits"])
        out["act"].append(o["actions"])
        out["rew"].append(ref.rewards.copy())
        out["disc"].append(ref.discounts.copy())
    return {k: np.stack(v) for k, v in out.items()}


def env_run():
    """A recording actor driven by fi_env_rollout for 3 T + 1 steps, released between the unrolls;
    beside it a plain actor of the same parameters and seed driven through the host calls on
    catch_reference. After unroll 0: one learner through step_rollout, one through step() on the
    host-packed entries. Computed once."""
    if _run:
        return _run
    from freeimpala_amd import env, hip
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import pack_atari_plane_records
    from freeimpala_amd.rollout import split_unrolls
    p0 = p0_atari()
    on_dev, on_host = make_learner(), make_learner()
    on_dev.set_params(p0)
    on_host.set_params(p0)
    rec, plain = (Actor("atari", N, num_actions=A, seed=ACTOR_SEED) for _ in range(2))
    rec.set_params(p0)
    plain.set_params(p0)
    rec.begin_rollout(T)
    e = env.CatchEnv(N, GAMMA, ENV_SEED)
    ref = env.catch_reference(N, GAMMA, ENV_SEED)
    # 15 steps before the recording starts, so that the reset falls on recorded step 5, mid-unroll
    d_act = hip.DeviceBuffer(N * 4)
    for j in range(PRE_STEPS):
        pre = ((np.arange(N) + j) % A).astype(np.int32)
        d_act.upload(pre)
        e.step(d_act.ptr)
        hip.synchronize()
        ref.step(pre)
    d_act.free()
    h = host_steps(plain, ref, STEPS)
    packed = [np.stack([np.frombuffer(x, np.uint8) for x in pack_atari_plane_records(*u)])
              for u in split_unrolls(h["planes"], h["start"], h["mu"], h["act"], h["rew"], h["disc"], T)]
    entries, counts, snaps = [], [], {}
    for k in range(3):
        counts.append(e.rollout(rec, T + 1 if k == 0 else T))
        assert rec.rollout_ready()
        entries.append(rec.read_rollout())
        if k == 0:
            snaps["dev"] = snapshot(on_dev, on_dev.step_rollout(rec))
            snaps["host"] = snapshot(on_host, on_host.step([row for row in packed[0]]))
            staging = dict(dev=on_dev.staging_bytes, host=on_host.staging_bytes)
        else:
            rec.release_rollout()
        assert not rec.rollout_ready()
    _run.update(p0=p0, host=h, packed=packed, entries=entries, counts=counts, snaps=snaps, staging=staging,
                final=dict(env=e.read(), state=e.state(), stats=e.stats(), stacks=rec.stacks(), out=rec.read_outputs()),
                want=dict(ref=ref, stacks=plain.stacks()))
    rec.end_rollout()
    for x in (rec, plain, e, on_dev, on_host):
        x.close()
    return _run


# ------------------------------------------------------------------ 3. recording parity
def test_rollout_records_equal_the_packed_host_rebuild():
    r = env_run()
    assert r["counts"] == [T + 1, T, T]
    assert len(r["entries"]) == 3
    for k in range(3):
        assert r["entries"][k].shape == r["packed"][k].shape == (N, (T + 1) * 7168 + 21504)
        np.testing.assert_array_equal(r["entries"][k], r["packed"][k], err_msg=f"unroll {k}")
    # the run crossed a reset in the middle of unroll 1, and the actions vary
    start = r["host"]["start"]
    assert start[20 - PRE_STEPS].all() and start.sum() == N and T < 20 - PRE_STEPS < 2 * T
    assert len(np.unique(r["host"]["act"])) > 1 and np.abs(r["host"]["rew"]).sum() == N
    # where the device loop ended is where the host loop ended
    ref = r["want"]["ref"]
    for nm in ("planes", "episode_start", "rewards", "discounts"):
        np.testing.assert_array_equal(r["final"]["env"][nm], getattr(ref, nm), err_msg=nm)
    for nm, want in ref.state().items():
        np.testing.assert_array_equal(r["final"]["state"][nm], want, err_msg=nm)
    assert r["final"]["stats"] == dict(episodes=ref.episodes, return_sum=ref.return_sum)
    np.testing.assert_array_equal(r["final"]["stacks"], r["want"]["stacks"])
    np.testing.assert_array_equal(r["final"]["out"]["actions"], r["host"]["act"][-1])
    np.testing.assert_array_equal(r["final"]["out"]["logits"].view(np.uint32), r["host"]["mu"][-1].view(np.uint32))


# ------------------------------------------------------------------ 4. learner parity
def test_learner_steps_from_the_rollout_as_from_the_packed_entries():
    r = env_run()
    same(r["snaps"]["dev"], r["snaps"]["host"], "step_rollout against step() on the packed entries")
    assert r["snaps"]["dev"]["stats"]["version"] == 1 and (r["snaps"]["dev"]["params"] != r["p0"]).any()
    assert np.isfinite(r["snaps"]["dev"]["grads"]).all() and r["snaps"]["dev"]["grads"].any()
    assert r["staging"]["dev"] == 0 and r["staging"]["host"] > 0


# ------------------------------------------------------------------ 5. ordering
def test_two_unrolls_without_a_host_wait_equal_the_waited_steps():
    from freeimpala_amd import env
    from freeimpala_amd.actor import Actor

    def make():
        a = Actor("atari", N, num_actions=A, seed=ACTOR_SEED)
        a.set_params(p0_atari())
        a.begin_rollout(T)
        return a, env.CatchEnv(N, GAMMA, ENV_SEED)

    def result(a, e):
        d = dict(entries=a.read_rollout(), stacks=a.stacks(), state=e.state(), stats=e.stats(), **e.read())
        d.update(a.read_outputs())
        return d

    fast, fe = make()
    assert fe.rollout(fast, T) == T and fe.rollout(fast, T) == T  # nothing waits between the two
    assert fast.sync() == 0
    slow, se = make()
    t = se.tensors()
    for _ in range(2 * T):  # the same 2 T steps, one call at a time, the host waiting after each
        slow.act_planes_dev(t["planes"], t["episode_start"], se.stepped_event)
        slow.sync()
        o = slow.outputs_dev()
        se.step(o["actions"], o["done_event"])  # on the null stream, behind the actor's event
        se.stats()  # waits
        slow.outcome_dev(t["rewards"], t["discounts"], se.stepped_event)
        slow.sync()
    assert fast.rollout_ready() and slow.rollout_ready()
    got, want = result(fast, fe), result(slow, se)
    assert got.keys() == want.keys()
    for nm in got:
        if nm in ("state", "stats"):
            assert str(got[nm]) == str(want[nm]), nm
        else:
            np.testing.assert_array_equal(got[nm], want[nm], err_msg=nm)
    # and the unroll that the next step completes
    for a, e in ((fast, fe), (slow, se)):
        a.release_rollout()
        assert e.rollout(a, 1) == 1 and a.rollout_ready()
    np.testing.assert_array_equal(fast.read_rollout(), slow.read_rollout())
    for a, e in ((fast, fe), (slow, se)):
        a.end_rollout()
        a.close()
        e.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_actor_recorder_and_environment_as_they_were():
    from freeimpala_amd import env, hip
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.actor import Actor
    p0 = p0_atari()
    e = env.CatchEnv(N, GAMMA, ENV_SEED)
    t = e.tensors()
    a = Actor("atari", N, num_actions=A, seed=ACTOR_SEED)
    twin = Actor("atari", N, num_actions=A, seed=ACTOR_SEED)  # takes only the calls that are not refused
    with pytest.raises(FiError, match=r"rc=-4: .*no parameters"):  # before set_params
        a.act_planes_dev(t["planes"], t["episode_start"])
    with pytest.raises(FiError, match=r"rc=-4: .*no parameters") as ei:
        e.rollout(a, 2)
    assert ei.value.steps_enqueued == 0
    a.set_params(p0)
    twin.set_params(p0)
    a.begin_rollout(T)
    twin.begin_rollout(T)
    te = env.CatchEnv(N, GAMMA, ENV_SEED)

    def refused(match, call, *args):
        before = (e.state(), e.stats(), e.read(), a.rollout_ready())
        with pytest.raises(FiError, match=match) as info:
            call(*args)
        after = (e.state(), e.stats(), e.read(), a.rollout_ready())
        assert str(before) == str(after)
        for x, y in zip(before[2].values(), after[2].values()):
            np.testing.assert_array_equal(x, y)
        return info.value

    host_planes, host_start = np.zeros(N * PLANE + 16, np.uint8), np.zeros(N + 16, np.uint8)
    hp = host_planes.ctypes.data + (-host_planes.ctypes.data) % 16
    hs = host_start.ctypes.data + (-host_start.ctypes.data) % 16
    short = hip.DeviceBuffer((N - 1) * PLANE)  # one row short
    tail = hip.DeviceBuffer(4096)
    refused(r"rc=-1: .*planes_dev is not device memory", a.act_planes_dev, hp, t["episode_start"])
    refused(r"rc=-1: .*episode_start_dev is not device memory", a.act_planes_dev, t["planes"], hs)
    refused(r"rc=-1: .*planes_dev must be 16-byte aligned", a.act_planes_dev, t["planes"] + 8, t["episode_start"])
    refused(r"rc=-1: .*episode_start_dev must be 16-byte aligned", a.act_planes_dev, t["planes"], t["episode_start"] + 1)
    refused(rf"rc=-1: .*planes_dev: the allocation ends .*{N * PLANE} are read", a.act_planes_dev, short.ptr,
            t["episode_start"])
    refused(r"rc=-1: .*Atari handle", a.act_obs_dev, t["planes"])
    refused(r"rc=-4: .*no act call since", a.outcome_dev, t["rewards"], t["discounts"])  # before any act call
    ml = Actor("mlp", MLP_N, num_actions=MLP_A, obs_dim=MLP_D, hidden=MLP_H)
    refused(r"rc=-1: .*MLP handle", ml.act_planes_dev, t["planes"], t["episode_start"])
    refused(r"rc=-1: .*Atari actor handle", e.rollout, ml, 1)
    ml.close()
    wide = Actor("atari", N + 1, num_actions=A)
    wide.set_params(p0)
    refused(rf"rc=-1: .*num_envs {N + 1} != the environment's {N}", e.rollout, wide, 1)
    wide.close()
    d_bad_actions = np.zeros(N + 4, np.int32)
    refused(r"rc=-1: .*actions_dev is not device memory", e.step, d_bad_actions.ctypes.data)
    refused(rf"rc=-1: .*actions_dev: the allocation ends 16 bytes .*{4 * N} are read", e.step, tail.ptr + 4096 - 16)

    # one step by hand: the outcome twice, and an act call without the outcome
    a.act_planes_dev(t["planes"], t["episode_start"])
    refused(r"rc=-4: .*never supplied", a.act_planes_dev, t["planes"], t["episode_start"])
    ei = refused(r"rc=-4: .*never supplied", e.rollout, a, 2)
    assert ei.steps_enqueued == 0
    refused(r"rc=-1: .*rewards_dev must be 16-byte aligned", a.outcome_dev, t["rewards"] + 4, t["discounts"])
    refused(r"rc=-1: .*discounts_dev is not device memory", a.outcome_dev, t["rewards"], hp)
    e.step(a.outputs_dev()["actions"], a.outputs_dev()["done_event"])
    a.outcome_dev(t["rewards"], t["discounts"], e.stepped_event)
    refused(r"rc=-4: .*no act call since", a.outcome_dev, t["rewards"], t["discounts"])
    a.sync()
    # across an unreleased unroll: T more steps complete unroll 0; the next T - 1 fill unroll 1, and
    # the step that would complete it is refused -- the rollout stops there and reports the count
    assert e.rollout(a, T) == T and a.rollout_ready()
    with pytest.raises(FiError, match=r"rc=-4: .*not been released") as info:
        e.rollout(a, T + 2)
    assert info.value.steps_enqueued == T - 1
    refused(r"rc=-4: .*not been released", e.rollout, a, 1)  # and nothing of the refused step was enqueued
    first = a.read_rollout()
    a.release_rollout()
    assert e.rollout(a, 1) == 1 and a.rollout_ready()
    # the twin took 1 + T + (T - 1) + 1 steps and no refusal: the same two unrolls, the same state
    assert te.rollout(twin, T + 1) == T + 1
    np.testing.assert_array_equal(first, twin.read_rollout())
    twin.release_rollout()
    assert te.rollout(twin, T) == T
    np.testing.assert_array_equal(a.read_rollout(), twin.read_rollout())
    assert str(e.state()) == str(te.state()) and e.stats() == te.stats()
    np.testing.assert_array_equal(a.stacks(), twin.stacks())
    got, want = a.read_outputs(), twin.read_outputs()  # the same draw index behind the refusals
    np.testing.assert_array_equal(got["actions"], want["actions"])
    np.testing.assert_array_equal(got["logits"], want["logits"])
    for x in (a, twin):
        x.end_rollout()
        x.close()
    for x in (e, te):
        x.close()
    short.free()
    tail.free()


# ------------------------------------------------------------------ 7. the C++ check program
def test_cpp_check_program_steps_from_rollouts_of_the_environment():
    exe = os.path.join(ROOT, "build", "host_env_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_env_check"], check=True)
    runs = [subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    lines = [[ln for ln in r.stdout.splitlines() if ln.startswith("env ")] for r in runs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], "a second run prints the same line"
    assert "version 3 episodes 3 return" in lines[0][0] and "nan" not in lines[0][0]


def test_sync_reports_nonfinite_rows_and_recovers():
    from freeimpala_amd import env
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.actor import Actor
    p0 = p0_atari()
    bad = p0.copy()
    bad[-(A + 1):] = np.nan  # the heads' biases: every logit and value
    e = env.CatchEnv(N, GAMMA, ENV_SEED)
    a = Actor("atari", N, num_actions=A, seed=ACTOR_SEED)
    a.set_params(bad)
    assert e.rollout(a, 2) == 2  # a device call cannot report the rows itself
    with pytest.raises(FiError, match=rf"rc=-7: .*{2 * N} rows") as ei:
        a.sync()
    assert ei.value.nonfinite_rows == 2 * N
    assert a.sync() == 0, "counted since the last sync"
    o = a.read_outputs()
    assert (o["actions"] == 0).all() and np.isnan(o["logits"]).all()
    a.set_params(p0)
    assert e.rollout(a, 2) == 2
    assert a.sync() == 0
    assert np.isfinite(a.read_outputs()["logits"]).all()
    a.close()
    e.close()
