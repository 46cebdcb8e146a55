"""Parameter publication on the device (include/fi_publish.h): the kernel alone against the numpy
rule, the snapshot against the host blob, an actor fed either way, stream order without a host wait,
a skipped update, the refusals, the version in the records, actor threads, a closed loop driven both
ways, and the C++ check program.

Everything is compared bit for bit: the published form is a copy or an integer rounding rule, and
the learner's step is bit-reproducible, so there is no tolerance anywhere in this file.

The policies: an MLP with obs_dim 128, hidden 256, A = 5 (100,358 parameters, n mod 4 = 2) and the
Atari policy with A = 3 (1,686,180 parameters, whole quads alone) and A = 18 (n odd). N = 4 environments and T = 3 unless a test says otherwise.

The resident step without statistics (step_resident(stats=False)) only enqueues: it is the
asynchronous resident step of tests 4 and 8. wait() checks for skipped updates only behind a step of
the _async entry points, so test 5 steps its batch with one action = A through step_async, from the
host copy of the resident batch."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = [("mlp", 5), ("atari", 3), ("atari", 18)]
DTYPES = ["fp32", "bf16"]
D, H = 128, 256
# a tie both ways, the largest finite value, +-Inf, -0.0, a denormal, signalling NaNs of both signs
SPECIALS = np.array([0x3f808000, 0x3f818000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x80000000, 0x00000001,
                     0x807fffff, 0x7f800001, 0xff800001, 0x7fa00000, 0xffc12345], np.uint32)
SENTINEL = np.uint32(0x7FC12345)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_learner(policy, publish="fp32", B=4, T=3, **kw):
    from freeimpala_amd.learner import DeviceLearner
    arch, A = policy
    kw.setdefault("seed", 3)
    kw.setdefault("lr", 1e-3)
    if arch == "atari":
        kw.setdefault("records", "planes")
    return DeviceLearner(arch, seq_len=T, batch=B, num_actions=A, obs_dim=D, hidden=H, publish=publish, **kw)


def make_actor(policy, N=4, seed=11):
    from freeimpala_amd.actor import Actor
    arch, A = policy
    return Actor(arch, num_envs=N, num_actions=A, obs_dim=D, hidden=H, seed=seed)


def widen(blob, n):
    """What fi_actor_set_params makes of a published blob: fp32 as it is, bf16 shifted up."""
    if len(blob) == 4 * n:
        return np.frombuffer(blob, np.float32).copy()
    assert len(blob) == 2 * n
    return (np.frombuffer(blob, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def refused(rc, call, *args):
    from freeimpala_amd._abi import FiError
    with pytest.raises(FiError, match=rf"rc={rc}\b") as e:
        call(*args)
    return str(e.value)


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.fixture(scope="module")
def kernel_input():
    rs = np.random.RandomState(65539)
    x = (rs.standard_normal(65539) * 10.0 ** rs.uniform(-20, 20, 65539)).astype(np.float32)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1027, 65539])
def test_publish_copy_is_the_numpy_rule(kernel_input, n, dtype):
    from freeimpala_amd import hip, publish
    x = kernel_input[:n].copy()
    k = min(n, SPECIALS.size)
    # the special values among the random ones: spread over the quads and, from the end, the tail
    where = np.unique(np.concatenate([np.arange(k) * max(1, n // (2 * k)), n - 1 - np.arange(min(k, 3))]))[:k]
    x.view(np.uint32)[where] = np.roll(SPECIALS, n)[:where.size]
    src = hip.DeviceBuffer.from_array(x)
    guard = np.full(n + 16, SENTINEL, np.uint32)
    dst = hip.DeviceBuffer.from_array(guard)
    publish.publish_copy(dst.ptr, src.ptr, n, dtype)
    hip.synchronize()
    got = dst.download(np.uint32, (n + 16,))
    want = publish.round_params(x, dtype).view(np.uint32)
    np.testing.assert_array_equal(got[:n], want)
    assert (got[n:] == SENTINEL).all(), "the 16 floats behind dst are untouched"
    np.testing.assert_array_equal(src.download(np.uint32, (n,)), x.view(np.uint32), err_msg="src is read only")
    if dtype == "bf16":
        assert (got[:n] & 0xffff == 0).all()
    if n >= 8:  # a pointer off 16-byte alignment is refused, either one, and nothing is written
        dst.upload(guard)
        assert "16-byte" in refused(-1, publish.publish_copy, dst.ptr + 4, src.ptr, n - 1, dtype)
        assert "16-byte" in refused(-1, publish.publish_copy, dst.ptr, src.ptr + 8, n - 2, dtype)
        hip.synchronize()
        assert (dst.download(np.uint32, (n + 16,)) == SENTINEL).all()
    src.free()
    dst.free()


# ------------------------------------------------------------------ 2. the snapshot is the blob
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: f"{p[0]}{p[1]}")
def test_snapshot_equals_blob(policy, dtype):
    from freeimpala_amd import publish
    L = make_learner(policy, dtype)
    n = L.param_count
    # whole quads alone (Atari, A = 3), a tail of two (MLP) and an odd count (Atari, A = 18)
    assert (n % 4 == 2) if policy == ("mlp", 5) else (n % 4 == 0) if policy == ("atari", 3) else (n % 2 == 1), n
    st = L.publish_state()
    assert st["publications"] == 0 and st["dtype"] == dtype and L.publish_event is None
    assert "published nothing" in refused(-4, L.published)
    L.synth(seed=7)
    for k, steps in enumerate((0, 2)):
        for _ in range(steps):
            L.step_resident()
        tag = L.publish()
        snap, version = L.published()
        blob, blob_version = L.get_blob()
        np.testing.assert_array_equal(bits(snap), bits(widen(blob, n)))
        np.testing.assert_array_equal(bits(snap), bits(publish.round_params(L.get_params(), dtype)))
        assert version == blob_version == tag == steps
        st = L.publish_state()
        assert st == dict(publications=k + 1, tag=steps, version=steps, slot=k, dtype=dtype, readers=[0, 0])
        assert L.publish_event is not None
    if dtype == "bf16":
        assert (bits(snap) & 0xffff == 0).all() and (bits(snap) != bits(L.get_params())).any()
    L.close()


# ------------------------------------------------------------------ 3. an actor fed either way
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: f"{p[0]}{p[1]}")
def test_actor_equal_by_blob_and_by_device(policy, dtype):
    L = make_learner(policy, dtype)
    L.synth(seed=9)
    L.step_resident()
    host, dev = make_actor(policy), make_actor(policy)
    assert "no parameters" in refused(-4, dev.read_params)
    blob, version = L.get_blob()
    host.set_params(blob, version)
    assert L.publish() == version
    dev.set_params_dev(L)
    assert dev.version == host.version == 1
    np.testing.assert_array_equal(bits(dev.read_params()), bits(host.read_params()))
    np.testing.assert_array_equal(bits(dev.read_params()), bits(widen(blob, L.param_count)))
    rs = np.random.RandomState(4)
    for _ in range(2):
        if policy[0] == "mlp":
            obs = rs.standard_normal((4, D)).astype(np.float32)
            a, b = host.act_obs(obs), dev.act_obs(obs)
        else:
            planes = rs.randint(0, 256, (4, 84, 84)).astype(np.uint8)
            start = np.array([1, 0, 0, 1], np.uint8)
            a, b = host.act_planes(planes, start), dev.act_planes(planes, start)
        for k in ("logits", "values"):
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
        np.testing.assert_array_equal(a["actions"], b["actions"])
        assert np.isfinite(a["logits"]).all()
    assert L.publish_state()["readers"] == [1, 0]
    for x in (host, dev, L):
        x.close()


# ------------------------------------------------------------------ 4. no host wait, slot reuse
def test_stream_order_without_a_host_wait_and_slot_reuse():
    from freeimpala_amd import publish
    policy = POLICIES[0]
    L = make_learner(policy)
    a = make_actor(policy)
    L.synth(seed=5)
    L.step_resident()
    L.wait()
    blob, version = L.get_blob()
    reference = widen(blob, L.param_count)
    assert version == 1
    # from here on nothing waits until a.sync()
    assert L.publish() == 1
    a.set_params_dev(L)
    for k in range(3):
        L.step_resident(stats=False)
        assert L.publish() == 2 + k  # publication 2 goes into the slot the actor reads: it waits for the reader's event
    a.sync()
    assert a.version == 1
    np.testing.assert_array_equal(bits(a.read_params()), bits(reference), err_msg="the actor holds version 1, not a later one")
    st = L.publish_state()
    assert st["publications"] == 4 and st["tag"] == 4 and st["version"] == 4 and st["slot"] == 1
    assert st["readers"] == [0, 0], "publication 2 took slot 0's reader"
    snap, exact = L.published()
    assert exact == 4
    np.testing.assert_array_equal(bits(snap), bits(publish.round_params(L.get_params(), "fp32")))
    assert (bits(snap) != bits(reference)).any()
    a.set_params_dev(L)
    assert a.version == 4
    np.testing.assert_array_equal(bits(a.read_params()), bits(snap))
    a.close()
    L.close()


# ------------------------------------------------------------------ 5. a skipped update
def test_skipped_update_tag_and_exact_version():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import pack_records
    policy, (T, B, A) = POLICIES[0], (3, 4, 5)
    L = make_learner(policy)
    L.synth(seed=6)
    L.step_resident()
    obs = L.tensor("obs", shape=(T + 1, B, D))
    mu = L.tensor("mu", shape=(T, B, A))
    act = L.tensor("actions", np.int32, (T, B)).copy()
    rew, disc = L.tensor("rewards", shape=(T, B)), L.tensor("discounts", shape=(T, B))
    act[1, 2] = A  # one action outside [0, A): the batch is rejected on the device, the update skipped
    before = L.get_params()
    L.step_async(pack_records(obs, mu, act, rew, disc))
    tag = L.publish()  # no wait in between
    snap, exact = L.published()
    assert tag == 2 and exact == 1, "the tag counts the enqueued update, the exact version does not"
    np.testing.assert_array_equal(bits(snap), bits(before), err_msg="the snapshot holds the parameters before the step")
    st = L.publish_state()
    assert st["tag"] == 2 and st["version"] == 1
    assert L.get_blob()[1] == 1
    with pytest.raises(FiError, match=r"rc=-1\b.*outside \[0, 5\)"):
        L.wait()
    tag = L.publish()
    snap, exact = L.published()
    assert tag == exact == 1
    np.testing.assert_array_equal(bits(snap), bits(before))
    act[1, 2] = 0
    L.step_async(pack_records(obs, mu, act, rew, disc))
    assert L.publish() == 2
    L.wait()
    snap, exact = L.published()
    assert exact == 2 and (bits(snap) != bits(before)).any()
    np.testing.assert_array_equal(bits(snap), bits(L.get_params()))
    L.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_actor_as_it_was():
    from freeimpala_amd import hip
    from freeimpala_amd.actor import Actor
    mlp, atari = POLICIES[0], POLICIES[1]
    L = make_learner(mlp)
    blob, _ = L.get_blob()
    held = widen(blob, L.param_count)
    a = make_actor(mlp, N=1)
    a.set_params(blob, 123)

    def unchanged(x=a):
        assert x.version == 123
        np.testing.assert_array_equal(bits(x.read_params()), bits(held))

    assert "published nothing" in refused(-4, a.set_params_dev, L)
    unchanged()
    L.synth(seed=2)
    L.step_resident()
    L.publish()
    other_a = Actor("mlp", num_envs=1, num_actions=6, obs_dim=D, hidden=H)
    assert "num_actions 6 != the learner's 5" in refused(-1, other_a.set_params_dev, L)
    assert other_a.version == 0 and "no parameters" in refused(-4, other_a.read_params)
    other_h = Actor("mlp", num_envs=1, num_actions=5, obs_dim=D, hidden=128)
    assert "hidden 128 != the learner's 256" in refused(-1, other_h.set_params_dev, L)
    other_d = Actor("mlp", num_envs=1, num_actions=5, obs_dim=64, hidden=H)
    assert "obs_dim 64 != the learner's 128" in refused(-1, other_d.set_params_dev, L)
    conv = make_actor(atari, N=1)
    assert "arch" in refused(-1, conv.set_params_dev, L)
    LA = make_learner(atari)
    LA.publish()
    assert "arch" in refused(-1, a.set_params_dev, LA)
    unchanged()
    # the layer underneath: a wrong count, a host pointer, a pointer off alignment, a short allocation
    n = a.param_count
    buf = hip.DeviceBuffer.from_array(np.zeros(n + 4, np.float32))
    assert f"count {n - 1} != the handle's parameter count {n}" in refused(-1, a.set_params_ptr, buf.ptr, n - 1, 7)
    host = np.zeros(n, np.float32)
    assert "not device memory" in refused(-1, a.set_params_ptr, host.ctypes.data, n, 7)
    assert "16-byte" in refused(-1, a.set_params_ptr, buf.ptr + 4, n, 7)
    assert "allocation ends" in refused(-1, a.set_params_ptr, buf.ptr + 32, n, 7)
    unchanged()
    # 64 distinct readers of one slot; the 65th is refused, one of the 64 may read again
    crowd = [make_actor(mlp, N=1) for _ in range(64)]
    for c in crowd:
        c.set_params_dev(L)
    assert L.publish_state()["readers"] == [64, 0]
    assert "reader 65" in refused(-4, a.set_params_dev, L)
    unchanged()
    crowd[5].set_params_dev(L)
    assert L.publish_state()["readers"] == [64, 0]
    L.publish()  # the other slot: it takes the 65th
    a.set_params_dev(L)
    assert a.version == 1 and L.publish_state()["readers"] == [64, 1]
    np.testing.assert_array_equal(bits(a.read_params()), bits(L.get_params()))
    # and through the layer underneath, from a buffer of the caller's
    buf.upload(np.concatenate([held, np.zeros(4, np.float32)]))
    assert a.set_params_ptr(buf.ptr, n, 77) is not None
    assert a.version == 77
    np.testing.assert_array_equal(bits(a.read_params()), bits(held))
    for x in crowd + [a, other_a, other_h, other_d, conv]:
        x.close()  # actors first here, the learner first in test 8: either order
    buf.free()
    L.close()
    LA.close()


# ------------------------------------------------------------------ 7. the version in the records
def test_new_version_in_the_records_mid_unroll():
    from freeimpala_amd.env import CatchEnv
    policy, N, T = POLICIES[1], 2, 4
    L = make_learner(policy, B=N, T=T)
    a = make_actor(policy, N=N)
    e = CatchEnv(N, 0.99, seed=1)
    assert L.publish() == 0
    a.set_params_dev(L)
    a.begin_rollout(T)
    assert e.rollout(a, 2) == 2
    L.synth(seed=8)  # one update on another batch: the resident one
    L.step_resident()
    assert L.publish() == 1
    a.set_params_dev(L)  # a recording handle, mid-unroll
    assert e.rollout(a, T + 1 - 2) == T - 1 and a.rollout_ready()
    st = L.step_rollouts([a])
    bv = L.batch_versions
    assert bv["min"] == 0 and bv["max"] == 1 and bv["mean"] == 0.5 and bv["count"] == T * N
    assert st["version"] == 2 and np.isfinite(st["total_loss"])
    a.sync()
    a.end_rollout()
    for x in (a, e, L):
        x.close()


# ------------------------------------------------------------------ 8. actor threads
def test_actor_threads_pull_while_the_learner_publishes():
    policy, rounds = POLICIES[0], 30
    L = make_learner(policy)
    L.synth(seed=4)
    actors = [make_actor(policy, seed=20 + i) for i in range(2)]
    L.publish()
    seen, errors = [[], []], []
    obs = np.random.RandomState(1).standard_normal((4, D)).astype(np.float32)

    def work(i):
        try:
            for _ in range(rounds):
                actors[i].set_params_dev(L)
                actors[i].act_obs(obs)
                seen[i].append(actors[i].version)
        except Exception as ex:  # noqa: BLE001 -- reported below, on the main thread
            errors.append((i, repr(ex)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for k in range(rounds):
        L.step_resident(stats=False)
        assert L.publish() == k + 1
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "an actor thread hangs"
    assert not errors, errors
    for s in seen:
        assert len(s) == rounds and all(x <= y for x, y in zip(s, s[1:])) and 0 <= s[0] and s[-1] <= rounds, s
    L.wait()
    assert L.publish() == rounds
    want = L.get_params()
    for a in actors:
        a.set_params_dev(L)
        assert a.version == rounds
        np.testing.assert_array_equal(bits(a.read_params()), bits(want))
    st = L.publish_state()
    assert st["publications"] == rounds + 2 and st["tag"] == st["version"] == rounds
    L.close()  # the learner first: the reader events are its block's
    for a in actors:
        a.close()


# ------------------------------------------------------------------ 9. the closed loop, both ways
def drive_closed_loop(device):
    from freeimpala_amd.env import CatchEnv
    policy, N, T, unrolls = POLICIES[1], 16, 4, 6
    L = make_learner(policy, B=N, T=T, lr=2e-3)
    a = make_actor(policy, N=N, seed=31)
    e = CatchEnv(N, 0.99, seed=17)

    def hand_over():
        if device:
            L.publish()
            a.set_params_dev(L)
        else:
            blob, version = L.get_blob()
            a.set_params(blob, version)

    hand_over()
    a.begin_rollout(T)
    assert e.rollout(a, T + 1) == T + 1
    triples = []
    for _ in range(unrolls):
        # the --overlap order: the next unroll's steps go first, up to the one that needs the released buffer
        assert e.rollout(a, T - 1) == T - 1
        L.step_rollouts_async([a])
        hand_over()
        assert e.rollout(a, 1) == 1 and a.rollout_ready()
        bv = L.batch_versions
        triples.append((bv["min"], bv["max"], bv["mean"]))
    st = L.wait()
    a.sync()
    out = dict(params=L.get_params(), stats=e.stats(), triples=triples, version=st["version"], actor_version=a.version,
               actor_params=a.read_params())
    a.end_rollout()
    for x in (a, e, L):
        x.close()
    return out


def test_closed_loop_is_bit_equal_by_device_and_by_blob():
    dev, host = drive_closed_loop(True), drive_closed_loop(False)
    print("batch_versions (min, max, mean) per unroll:", dev["triples"])
    np.testing.assert_array_equal(bits(dev["params"]), bits(host["params"]))
    np.testing.assert_array_equal(bits(dev["actor_params"]), bits(host["actor_params"]))
    assert dev["stats"] == host["stats"] and dev["stats"]["episodes"] >= 16
    assert dev["triples"] == host["triples"]
    assert dev["version"] == host["version"] == 6 and dev["actor_version"] == host["actor_version"] == 6
    # the lag V-trace corrects: unroll u >= 1 is acted under version u - 1 (its last step's hand-over
    # comes behind update u) and stepped as update u + 1, one version behind the parameters it updates
    assert dev["triples"] == [(0, 0, 0.0)] + [(u - 1, u - 1, float(u - 1)) for u in range(1, 6)]
    np.testing.assert_array_equal(bits(dev["params"]), bits(dev["actor_params"]))


# ------------------------------------------------------------------ 10. the C++ check program
def test_cpp_check_program():
    exe = os.path.join(ROOT, "build", "host_publish_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_publish_check"], check=True)
    runs = [subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    lines = [[ln for ln in r.stdout.splitlines() if ln.startswith("publish atari:")] for r in runs]
    assert len(lines[0]) == 1 and lines[0] == lines[1], "a second run prints the same line"
    m = re.search(r"version (\d+) tag (\d+) publications (\d+) params (\d+)", lines[0][0])
    assert m and [int(g) for g in m.groups()[:3]] == [1, 1, 2] and "nan" not in lines[0][0]
