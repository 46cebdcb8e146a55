"""Rollouts recorded on the device (include/fi_rollout.h): the record and history kernels alone
against the packer, a recording actor's completed unrolls against pack_atari_plane_records /
pack_records of split_unrolls (the recording rule on the host), a learner that steps from the
device entries against one that steps from their host copy, the closed loop, and the refusals.

Every comparison is exact. The closed loop alone also checks vs / pg_adv against the oracle's
V-trace on the device's own logits, within 1e-5 of the largest magnitude (the bound of
test_closed_loop_actor_records_learner, whose assertion this brings to the device path)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE, FRAME = 84 * 84, 84 * 84 * 4
REC, HIST = 7168, 21504
FLAGS = 7140
GUARD = 256


def entry_bytes(T):
    return (T + 1) * REC + HIST


def flags_words(entries, T):
    """The flags word of every record: (N, T+1) uint32."""
    e = np.asarray(entries)
    return np.stack([e[:, t * REC + FLAGS:t * REC + FLAGS + 4].copy().view(np.uint32)[:, 0] for t in range(T + 1)], 1)


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_record_and_history_kernels_equal_the_packer(N, A):
    """T + 1 = 3 record launches and one history launch into entries that lie between 0xA5 guards
    with a stride 48 bytes above the entry size: the entries are the packer's bytes, the guards and
    the padding between entries are untouched. The flags pointer is off 4-byte alignment."""
    from freeimpala_amd import hip, rollout
    from freeimpala_amd.learner import pack_atari_plane_records
    T = 2
    E = entry_bytes(T)
    stride = E + 48
    rs = np.random.RandomState(100 * N + A)
    planes = rs.randint(0, 256, (T + 1, N, 84, 84)).astype(np.uint8)
    start = rs.rand(T + 1, N) < 0.5
    start[0, 0] = True
    start[1, 0] = False
    mu = rs.standard_normal((T, N, A)).astype(np.float32)
    act = rs.randint(0, A, (T, N)).astype(np.int32)
    stacks = rs.randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    history = np.ascontiguousarray(np.moveaxis(stacks[..., :3], -1, 0))
    zero = np.zeros((T, N), np.float32)
    want = np.stack([np.frombuffer(e, np.uint8) for e in
                     pack_atari_plane_records(planes, history, start, mu, act, zero, zero)])
    assert want.shape == (N, E)

    init = np.full(2 * GUARD + N * stride, 0xA5, np.uint8)
    body = init[GUARD:GUARD + N * stride].reshape(N, stride)
    body[:, :E] = 0
    buf = hip.DeviceBuffer.from_array(init)
    dst = buf.ptr + GUARD
    dpl, dfl = hip.DeviceBuffer(N * PLANE), hip.DeviceBuffer(N + 8)
    dlo, dac = hip.DeviceBuffer(N * A * 4), hip.DeviceBuffer(N * 4)
    dst_stacks = hip.DeviceBuffer.from_array(stacks)
    off = 1
    for t in range(T + 1):
        dpl.upload(planes[t])
        fl = np.full(N + 8, 0xFF, np.uint8)  # the bytes around the flags are not flags
        fl[off:off + N] = start[t]
        dfl.upload(fl)
        if t < T:
            dlo.upload(mu[t])
            dac.upload(act[t])
            rollout.record_plane_step(dst, stride, t, dpl.ptr, dfl.ptr + off, dlo.ptr, dac.ptr, 0, N, A)
        else:
            rollout.record_plane_step(dst, stride, t, dpl.ptr, dfl.ptr + off, None, None, 0x55, N, A)
        hip.synchronize()
    rollout.extract_history(dst, stride, (T + 1) * REC, dst_stacks.ptr, N)
    hip.synchronize()

    def check(what):
        got = buf.download(np.uint8, (init.size,))
        assert (got[:GUARD] == 0xA5).all() and (got[GUARD + N * stride:] == 0xA5).all(), f"{what}: guard overwritten"
        rows = got[GUARD:GUARD + N * stride].reshape(N, stride)
        assert (rows[:, E:] == 0xA5).all(), f"{what}: stride padding overwritten"
        return rows[:, :E]

    np.testing.assert_array_equal(check("records"), want)
    # the flags word alone: record 1 again, with another value
    dpl.upload(planes[1])
    fl = np.full(N + 8, 0xFF, np.uint8)
    fl[off:off + N] = start[1]
    dfl.upload(fl)
    dlo.upload(mu[1])
    dac.upload(act[1])
    rollout.record_plane_step(dst, stride, 1, dpl.ptr, dfl.ptr + off, dlo.ptr, dac.ptr, 0x01020304, N, A)
    hip.synchronize()
    got = check("flags")
    w = flags_words(got, T)
    assert (w[:, 1] == 0x01020304).all() and (w[:, 0] == 0).all() and (w[:, 2] == 0).all()
    again = got.copy()
    again[:, REC + FLAGS:REC + FLAGS + 4] = 0
    np.testing.assert_array_equal(again, want)
    for b in (buf, dpl, dfl, dlo, dac, dst_stacks):
        b.free()


# ------------------------------------------------------------------ the shared Atari run
A_, T_, N_, CALLS = 6, 3, 4, 10
_run = {}

LEARNER_TENSORS = (("frames", np.uint8), ("logits", np.float32), ("mu", np.float32), ("vs", np.float32),
                   ("values", np.float32), ("pg_adv", np.float32), ("actions", np.int32), ("rewards", np.float32),
                   ("discounts", np.float32))


def snapshot(L, stats):
    d = {nm: L.tensor(nm, dt) for nm, dt in LEARNER_TENSORS}
    d["params"] = L.get_params()
    d["stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    return d


def start_pattern():
    """Every env starts at call 0; env 0 restarts mid-unroll (call 1); env 1 on the carry-over call
    3; env 3 at calls 4 and 5 (two in a row); env 2 never again."""
    s = np.zeros((CALLS, N_), bool)
    s[0] = True
    s[1, 0] = True
    s[3, 1] = True
    s[4, 3] = s[5, 3] = True
    return s


def atari_run():
    """10 act calls of a recording actor (N = 4, T = 3, A = 6: 3 unrolls, buffer 0 used twice), a
    plain actor beside it on the same inputs, and after each completing call: the entries read
    back, then three learners from the same parameters -- `still` (lr = 0) through
    step_entries_dev on the acquired buffer, `dev` (Adam) through step_rollout, `host` (Adam)
    through step() on the host copy. Everything the tests compare, computed once."""
    if _run:
        return _run
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    kw = dict(seq_len=T_, batch=N_, num_actions=A_, records="planes")
    dev = DeviceLearner("atari", optimizer="adam", lr=1e-3, **kw)
    host = DeviceLearner("atari", optimizer="adam", lr=1e-3, **kw)
    still = DeviceLearner("atari", optimizer="sgd", lr=0.0, **kw)
    p0 = dev.get_params()
    host.set_params(p0)
    still.set_params(p0)
    rec = Actor("atari", N_, num_actions=A_, seed=17)
    plain = Actor("atari", N_, num_actions=A_, seed=17)
    rec.set_params(p0)
    plain.set_params(p0)
    rec.begin_rollout(T_)
    assert rec.rollout_entry_bytes == entry_bytes(T_) == dev.entry_bytes
    rs = np.random.RandomState(55)
    planes = rs.randint(0, 256, (CALLS, N_, 84, 84)).astype(np.uint8)
    start = start_pattern()
    rew = rs.randint(-1, 2, (CALLS, N_)).astype(np.float32)
    disc = (0.99 * (rs.rand(CALLS, N_) > 0.2)).astype(np.float32)
    outs, plain_outs, entries, ready = [], [], [], []
    snaps = dict(dev=[], host=[], still=[])
    for j in range(CALLS):
        outs.append(rec.act_planes(planes[j], start[j]))
        plain_outs.append(plain.act_planes(planes[j], start[j]))
        rec.outcome(rew[j], disc[j])
        ready.append(rec.rollout_ready())
        if not ready[-1]:
            continue
        e = rec.read_rollout()
        entries.append(e)
        ptr, stride, ev = rec.acquire_rollout()
        assert stride == entry_bytes(T_)
        snaps["still"].append(snapshot(still, still.step_entries_dev(ptr, stride, ev)))
        assert rec.rollout_ready()  # step_entries_dev does not release
        snaps["dev"].append(snapshot(dev, dev.step_rollout(rec)))
        assert not rec.rollout_ready()
        snaps["host"].append(snapshot(host, host.step([row for row in e])))
    _run.update(p0=p0, planes=planes, start=start, rew=rew, disc=disc, outs=outs, plain_outs=plain_outs,
                entries=entries, ready=ready, snaps=snaps,
                staging=dict(dev=dev.staging_bytes, host=host.staging_bytes, still=still.staging_bytes),
                stacks=(rec.stacks(), plain.stacks()))
    rec.end_rollout()
    for h in (rec, plain, dev, host, still):
        h.close()
    return _run


# ------------------------------------------------------------------ 2. recorded entries = packed entries
def test_recorded_unrolls_equal_the_packed_unrolls():
    from freeimpala_amd.learner import pack_atari_plane_records
    from freeimpala_amd.rollout import split_unrolls
    r = atari_run()
    assert r["ready"] == [j > 0 and j % T_ == 0 for j in range(CALLS)]
    assert len(r["entries"]) == 3
    mu = np.stack([o["logits"] for o in r["outs"]])
    act = np.stack([o["actions"] for o in r["outs"]])
    unrolls = split_unrolls(r["planes"], r["start"], mu, act, r["rew"], r["disc"], T_)
    for k, u in enumerate(unrolls):
        want = np.stack([np.frombuffer(e, np.uint8) for e in pack_atari_plane_records(*u)])
        got = r["entries"][k]
        assert got.shape == want.shape == (N_, entry_bytes(T_))
        np.testing.assert_array_equal(got, want, err_msg=f"unroll {k}")


def test_flags_word_carries_the_parameter_version():
    """Version 7 is set before the call that completes unroll 0: that call writes record T of
    unroll 0 (no flags) and record 0 of unroll 1 (7)."""
    from freeimpala_amd.actor import Actor
    r = atari_run()
    a = Actor("atari", N_, num_actions=A_, seed=17)
    a.set_params(r["p0"])
    a.begin_rollout(T_)
    words = []
    for j in range(2 * T_ + 1):
        if j == T_:
            a.set_params(r["p0"], version=7)
        out = a.act_planes(r["planes"][j], r["start"][j])
        np.testing.assert_array_equal(out["logits"], r["outs"][j]["logits"])
        a.outcome(r["rew"][j], r["disc"][j])
        if a.rollout_ready():
            words.append(flags_words(a.read_rollout(), T_))
            a.release_rollout()
    a.close()
    assert len(words) == 2
    assert (words[0] == 0).all()
    assert (words[1][:, :T_] == 7).all() and (words[1][:, T_] == 0).all()


# ------------------------------------------------------------------ 3. MLP
@pytest.mark.parametrize("D", [128, 7])
def test_mlp_recording_equals_pack_records(D):
    """Two unrolls of an MLP actor against pack_records, byte for byte; then a learner that steps
    from the device entries against one that steps from their host copy, both with Adam: they
    stay bit-equal in the ingested tensors, logits, values, vs, the step stats and the parameters.
    (H = 32 with A = 64 is the shape whose heads' weight-gradient slabs used to run into the bias
    column sums behind them, A + 1 > max(D, H): the two learners agree only since they do not.)"""
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner, pack_records
    N, T, A, H = 5, 2, 64, 32
    kw = dict(seq_len=T, batch=N, num_actions=A, obs_dim=D, hidden=H, optimizer="adam", lr=1e-3)
    dev, host = DeviceLearner("mlp", **kw), DeviceLearner("mlp", **kw)
    p0 = dev.get_params()
    host.set_params(p0)
    a = Actor("mlp", N, num_actions=A, obs_dim=D, hidden=H, seed=5)
    a.set_params(p0)
    a.begin_rollout(T)
    assert a.rollout_entry_bytes == (T + 1) * 1024 == dev.entry_bytes
    rs = np.random.RandomState(D)
    S = 2 * T + 1
    obs = rs.standard_normal((S, N, D)).astype(np.float32)
    rew = rs.standard_normal((S, N)).astype(np.float32)
    disc = (0.99 * (rs.rand(S, N) > 0.2)).astype(np.float32)
    outs, k = [], 0
    for j in range(S):
        outs.append(a.act_obs(obs[j]))
        a.outcome(rew[j], disc[j])
        assert a.rollout_ready() == (j > 0 and j % T == 0)
        if not a.rollout_ready():
            continue
        lo = k * T
        mu = np.stack([o["logits"] for o in outs[lo:lo + T]])
        act = np.stack([o["actions"] for o in outs[lo:lo + T]])
        want = np.stack([np.frombuffer(e, np.uint8)
                         for e in pack_records(obs[lo:lo + T + 1], mu, act, rew[lo:lo + T], disc[lo:lo + T])])
        got = a.read_rollout()
        np.testing.assert_array_equal(got, want, err_msg=f"unroll {k}")
        sd = dev.step_rollout(a)
        sh = host.step([row for row in got])
        for nm, dt in (("obs", np.float32), ("mu", np.float32), ("actions", np.int32), ("rewards", np.float32),
                       ("discounts", np.float32), ("logits", np.float32), ("values", np.float32), ("vs", np.float32)):
            np.testing.assert_array_equal(dev.tensor(nm, dt), host.tensor(nm, dt), err_msg=f"unroll {k}: {nm}")
        np.testing.assert_array_equal(dev.tensor("obs").reshape(T + 1, N, D), obs[lo:lo + T + 1])
        same = ("pg_loss", "baseline_loss", "entropy_loss", "total_loss", "grad_norm", "version")
        assert {x: sd[x] for x in same} == {x: sh[x] for x in same}
        np.testing.assert_array_equal(dev.get_params(), host.get_params())
        k += 1
    assert k == 2 and dev.staging_bytes == 0 and host.staging_bytes > 0
    assert (dev.get_params() != p0).any()
    a.end_rollout()
    for h in (a, dev, host):
        h.close()


# ------------------------------------------------------------------ 4. device step = host step
def test_step_from_device_entries_equals_step_from_their_host_copy():
    r = atari_run()
    dev, host = r["snaps"]["dev"], r["snaps"]["host"]
    assert len(dev) == len(host) == 3
    for k, (d, h) in enumerate(zip(dev, host)):
        for nm in ("frames", "logits", "mu", "vs", "params"):
            np.testing.assert_array_equal(d[nm], h[nm], err_msg=f"unroll {k}: {nm}")
        assert d["stats"] == h["stats"], (k, d["stats"], h["stats"])
        assert d["stats"]["version"] == k + 1
    assert (dev[0]["params"] != r["p0"]).any(), "Adam at lr > 0 moves the parameters"
    # the learners that stepped from device memory never allocated the host-entry staging
    assert r["staging"]["dev"] == 0 and r["staging"]["still"] == 0
    assert r["staging"]["host"] == 4 * N_ * entry_bytes(T_)


# ------------------------------------------------------------------ 5. closed loop
def test_closed_loop_on_the_device(orc):
    """The learner that holds the actor's parameters (lr = 0) rebuilds the actor's stacks from the
    device entries and recomputes its logits bit for bit, so pi = mu exactly, in every unroll (from
    the second on the stacks come out of the recorded history block); vs and pg_adv are the
    oracle's at those logits within 1e-5."""
    from freeimpala_amd.learner import stack_planes
    r = atari_run()
    whole = stack_planes(r["planes"], np.zeros((3, N_, 84, 84), np.uint8), r["start"])
    for k, s in enumerate(r["snaps"]["still"]):
        lo = k * T_
        np.testing.assert_array_equal(s["frames"].reshape(T_ + 1, N_, 84, 84, 4), whole[lo:lo + T_ + 1])
        logits = s["logits"].reshape(T_ + 1, N_, A_)
        values = s["values"].reshape(T_ + 1, N_)
        mu = s["mu"].reshape(T_, N_, A_)
        for t in range(T_ + 1):
            np.testing.assert_array_equal(logits[t], r["outs"][lo + t]["logits"], err_msg=f"logits of call {lo + t}")
            np.testing.assert_array_equal(values[t], r["outs"][lo + t]["values"], err_msg=f"values of call {lo + t}")
        np.testing.assert_array_equal(mu, logits[:T_])
        act = s["actions"].reshape(T_, N_)
        np.testing.assert_array_equal(act, np.stack([o["actions"] for o in r["outs"][lo:lo + T_]]))
        np.testing.assert_array_equal(s["rewards"].reshape(T_, N_), r["rew"][lo:lo + T_])
        np.testing.assert_array_equal(s["discounts"].reshape(T_, N_), r["disc"][lo:lo + T_])
        vt = orc.vtrace_loss(logits[:T_], mu, act, r["rew"][lo:lo + T_], r["disc"][lo:lo + T_], values)
        for nm in ("vs", "pg_adv"):
            got = s[nm].reshape(T_, N_)
            err = np.abs(got - vt[nm]).max() / max(1.0, np.abs(vt[nm]).max())
            print(f"closed loop, unroll {k}: {nm} err {err:.2e}")
            assert err <= 1e-5, (k, nm, err)
    np.testing.assert_array_equal(r["stacks"][0], whole[-1])


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handles_usable():
    from freeimpala_amd import hip
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    r = atari_run()
    T = 2
    planes, start = r["planes"], r["start"]
    zeros, ones = np.zeros(N_, np.float32), np.ones(N_, np.float32)
    a = Actor("atari", N_, num_actions=A_, seed=17)
    a.set_params(r["p0"])
    with pytest.raises(FiError, match=r"rc=-4: .*does not record"):
        a.outcome(zeros, ones)
    with pytest.raises(FiError, match=r"rc=-4: .*does not record"):
        a.acquire_rollout()
    with pytest.raises(FiError, match=r"rc=-1: .*seq_len"):
        a.begin_rollout(0)
    a.begin_rollout(T)
    with pytest.raises(FiError, match=r"rc=-4: .*records already"):
        a.begin_rollout(T)
    with pytest.raises(FiError, match=r"rc=-4: .*no act call"):  # an outcome before any step
        a.outcome(zeros, ones)
    with pytest.raises(FiError, match=r"rc=-1: .*stacked records are not produced"):
        a.act_frames(np.zeros((N_, 84, 84, 4), np.uint8))
    with pytest.raises(FiError, match=r"rc=-4: .*break the history"):
        a.reset_stacks()
    with pytest.raises(FiError, match=r"rc=-4: .*no completed unroll"):
        a.acquire_rollout()
    with pytest.raises(FiError, match=r"rc=-4: .*no completed unroll"):
        a.read_rollout()
    with pytest.raises(FiError, match=r"rc=-4: .*no completed unroll"):
        a.release_rollout()
    outs = [a.act_planes(planes[0], start[0])]
    stacks = a.stacks()
    with pytest.raises(FiError, match=r"rc=-4: .*never supplied"):  # an act call without an outcome
        a.act_planes(planes[1], start[1])
    np.testing.assert_array_equal(a.stacks(), stacks)  # refused before the push
    a.outcome(r["rew"][0], r["disc"][0])
    with pytest.raises(FiError, match=r"rc=-4: .*no act call"):  # a double outcome
        a.outcome(zeros, ones)
    for j in (1, 2):
        outs.append(a.act_planes(planes[j], start[j]))
        a.outcome(r["rew"][j], r["disc"][j])
    assert a.rollout_ready()  # unroll 0, and nobody releases it
    outs.append(a.act_planes(planes[3], start[3]))
    a.outcome(r["rew"][3], r["disc"][3])
    stacks = a.stacks()
    with pytest.raises(FiError, match=r"rc=-4: .*has not been released"):  # the call that completes unroll 1
        a.act_planes(planes[4], start[4])
    np.testing.assert_array_equal(a.stacks(), stacks)
    first = a.read_rollout()

    # the learner side, on the waiting unroll
    ptr, stride, ev = a.acquire_rollout()
    L = DeviceLearner("atari", seq_len=T, batch=N_, num_actions=A_, records="planes", optimizer="sgd", lr=0.0)
    L.set_params(r["p0"])
    with pytest.raises(FiError, match=r"rc=-1: .*16-byte aligned"):
        L.step_entries_dev(ptr + 4, stride, ev)
    with pytest.raises(FiError, match=r"rc=-1: .*16-byte aligned"):
        L.step_entries_dev(ptr, stride + 8, ev)
    with pytest.raises(FiError, match=rf"rc=-1: .*entry_stride {stride - 16} < {stride}"):
        L.step_entries_dev(ptr, stride - 16, ev)
    with pytest.raises(FiError, match=r"rc=-1: .*allocation ends"):  # the stride would run past the buffer
        L.step_entries_dev(ptr, 2 * stride, ev)
    host_mem = np.zeros(N_ * stride + 16, np.uint8)
    with pytest.raises(FiError, match=r"rc=-1: .*not device memory"):
        L.step_entries_dev(host_mem.ctypes.data + (-host_mem.ctypes.data) % 16, stride)
    stacked = DeviceLearner("atari", seq_len=T, batch=N_, num_actions=A_, optimizer="sgd")
    with pytest.raises(FiError, match=r"rc=-1: .*planes format"):
        stacked.step_rollout(a)
    with pytest.raises(FiError, match=r"rc=-1: .*planes format"):
        stacked.step_entries_dev(ptr, stride, ev)
    stacked.close()
    wide = DeviceLearner("atari", seq_len=T, batch=N_ + 4, num_actions=A_, records="planes", optimizer="sgd")
    with pytest.raises(FiError, match=rf"rc=-1: .*num_envs {N_} != the learner's {N_ + 4}"):
        wide.step_rollout(a)
    wide.close()
    long = DeviceLearner("atari", seq_len=T + 1, batch=N_, num_actions=A_, records="planes", optimizer="sgd")
    with pytest.raises(FiError, match=rf"rc=-1: .*seq_len {T} != the learner's {T + 1}"):
        long.step_rollout(a)
    long.close()
    mlp = DeviceLearner("mlp", seq_len=T, batch=N_, num_actions=A_, optimizer="sgd")
    with pytest.raises(FiError, match=r"rc=-1: .*arch"):
        mlp.step_rollout(a)
    mlp.close()
    assert a.rollout_ready()  # every refusal left the unroll waiting
    np.testing.assert_array_equal(a.read_rollout(), first)

    # and both handles still work: the unroll steps, the refused call goes through, unroll 1 completes
    L.step_rollout(a)
    with pytest.raises(FiError, match=r"rc=-4: .*no completed unroll"):
        L.step_rollout(a)
    logits = L.tensor("logits", shape=(T + 1, N_, A_))
    for t in range(T + 1):
        np.testing.assert_array_equal(logits[t], outs[t]["logits"])
    outs.append(a.act_planes(planes[4], start[4]))
    a.outcome(r["rew"][4], r["disc"][4])
    assert a.rollout_ready()
    L.step_rollout(a)
    logits = L.tensor("logits", shape=(T + 1, N_, A_))
    for t in range(T + 1):
        np.testing.assert_array_equal(logits[t], outs[T + t]["logits"])
    L.step_resident()  # re-steps the same batch
    np.testing.assert_array_equal(L.tensor("logits", shape=(T + 1, N_, A_)), logits)
    a.end_rollout()
    a.end_rollout()  # not recording: nothing to do
    a.reset_stacks()  # allowed again
    a.act_frames(np.zeros((N_, 84, 84, 4), np.uint8))
    a.close()
    L.close()

    d = hip.DeviceBuffer(4 * REC)
    from freeimpala_amd import rollout
    with pytest.raises(FiError, match=r"rc=-1: .*entry_stride"):
        rollout.record_plane_step(d.ptr, REC, 1, d.ptr, d.ptr, None, None, 0, 1, 6)
    with pytest.raises(FiError, match=r"rc=-1: .*aligned"):
        rollout.record_plane_step(d.ptr + 4, 2 * REC, 1, d.ptr, d.ptr, None, None, 0, 1, 6)
    with pytest.raises(FiError, match=r"rc=-1: .*2 <= A <= 18"):
        rollout.record_plane_step(d.ptr, 2 * REC, 1, d.ptr, d.ptr, None, None, 0, 1, 19)
    with pytest.raises(FiError, match=r"rc=-1: .*entry_stride"):
        rollout.extract_history(d.ptr, 3 * PLANE, 16, d.ptr, 1)
    with pytest.raises(FiError, match=r"rc=-1: .*N must be >= 1"):
        rollout.extract_history(d.ptr, 4 * REC, 0, d.ptr, 0)
    d.free()


# ------------------------------------------------------------------ 7. no change without begin
def test_an_actor_that_never_records_is_unchanged():
    """The plain actor beside the recording one: the same outputs and stacks for the same inputs,
    call by call (and test_gpu_actor.py, unmodified, pins what a plain actor computes)."""
    r = atari_run()
    for j, (o, p) in enumerate(zip(r["outs"], r["plain_outs"])):
        for nm in ("actions", "logits", "values"):
            np.testing.assert_array_equal(o[nm], p[nm], err_msg=f"call {j}: {nm}")
    np.testing.assert_array_equal(r["stacks"][0], r["stacks"][1])


# ------------------------------------------------------------------ 8. C++ wrapper
EXE = os.path.join(ROOT, "build", "host_rollout_check")


def test_cpp_wrapper_records_and_steps():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_rollout_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("rollout ")]
    assert len(lines) == 2 and lines[0].startswith("rollout mlp:") and lines[1].startswith("rollout atari:")
    for ln in lines:
        assert ln.endswith("version 1") and "nan" not in ln
