"""The device Breakout environment (include/fi_breakout.h) against breakout_reference byte for byte:
the handle and its two kernels alone between guard bands in a random run that meets walls, bricks,
the paddle, misses and truncations; every event of the rule, one per environment, from states
written with set_state; the render over more than one workgroup; the totals over partial waves and
two blocks; a recording actor driven by fi_env_rollout against the packer on the reference stepped
with the recorded actions, and a learner that steps from those unrolls against one fed the packed
entries; the refusals; and the C++ check program.

No comparison has a tolerance: everything compared is integer data, or the output of the same
kernel on the same bytes."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_ring import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE = 84 * 84
FULL = (1 << 63) - 1
GAMMA = 0.99
TENSORS = ("planes", "episode_start", "rewards", "discounts")
NAMES = ("state", "planes", "episode_start", "rewards", "discounts", "totals")


def guarded(n):
    return Guarded([(8 * n, np.uint32), (n * PLANE, np.uint8), (n, np.uint8), (n, np.float32), (n, np.float32),
                    (2, np.uint64)])


def check_handle(e, ref, what):
    """every byte of the handle's state and tensors, and the totals"""
    got, st = e.read(), e.state()
    for nm in TENSORS:
        assert got[nm].dtype == getattr(ref, nm).dtype
        np.testing.assert_array_equal(got[nm], getattr(ref, nm), err_msg=f"{what}: {nm}")
    for nm, want in ref.state().items():
        assert st[nm].dtype == want.dtype, nm
        np.testing.assert_array_equal(st[nm], want, err_msg=f"{what}: {nm}")
    assert e.stats() == dict(episodes=ref.episodes, return_sum=ref.return_sum), what


def check_guarded(g, ref, what):
    from freeimpala_amd.breakout import pack_state
    got = g.read(NAMES)  # asserts the guards
    np.testing.assert_array_equal(got["state"].reshape(-1, 8), pack_state(ref.state()), err_msg=f"{what}: state words")
    np.testing.assert_array_equal(got["planes"].reshape(-1, 84, 84), ref.planes, err_msg=f"{what}: planes")
    for nm in TENSORS[1:]:
        np.testing.assert_array_equal(got[nm], getattr(ref, nm), err_msg=f"{what}: {nm}")
    assert (int(got["totals"][0]), int(got["totals"].view(np.int64)[1])) == (ref.episodes, ref.return_sum), what


# ------------------------------------------------------------------ 1. parity in a random run
@pytest.mark.parametrize("seed", [1, 3])
def test_environment_equals_breakout_reference_for_120_steps(seed):
    """N = 5 (odd, below a wave), max_steps = 40, 120 steps of RandomState(seed).randint(0, 4)."""
    from freeimpala_amd import breakout, hip
    n, max_steps, steps = 5, 40, 120
    ref = breakout.breakout_reference(n, GAMMA, seed, max_steps)
    e = breakout.BreakoutEnv(n, GAMMA, seed, max_steps)
    assert e.max_steps == max_steps and breakout.lib().fi_env_num_envs(e._h) == n
    g = guarded(n)
    hip.upload_ptr(g.ptr[0], breakout.pack_state(ref.state()))
    hip.upload_ptr(g.ptr[5], np.zeros(2, np.uint64))
    for j, nm in ((2, "episode_start"), (3, "rewards"), (4, "discounts")):
        hip.upload_ptr(g.ptr[j], getattr(ref, nm))
    breakout.breakout_render(g.ptr[0], g.ptr[1], n)
    hip.synchronize()
    check_handle(e, ref, "first observation")  # Reset(i, 0), episode_start = 1
    check_guarded(g, ref, "first observation")
    assert (e.read()["episode_start"] == 1).all()
    actions = np.random.RandomState(seed).randint(0, 4, (steps, n)).astype(np.int32)
    d_act = hip.DeviceBuffer(n * 4)
    for t in range(steps):
        d_act.upload(actions[t])
        e.step(d_act.ptr)
        breakout.breakout_update(g.ptr[0], d_act.ptr, n, GAMMA, seed, max_steps, g.ptr[2], g.ptr[3], g.ptr[4], g.ptr[5])
        breakout.breakout_render(g.ptr[0], g.ptr[1], n)
        hip.synchronize()
        ref.step(actions[t])
        check_handle(e, ref, f"step {t}")
        check_guarded(g, ref, f"step {t}")
    for ev in ("wall", "brick", "paddle", "miss", "truncation"):  # what the run has to have met
        assert ref.events[ev] >= 1, (ev, ref.events)
    g.free()
    d_act.free()
    e.close()


# ------------------------------------------------------------------ 2. every event, from set_state
def scenario_states():
    """Two rounds of 8 hand-written states (max_steps = 50) and their actions: one event each."""
    q = dict(r=10, c=10, p=10, k=7, dr=1, dc=1, t=3, score=2, bricks=FULL)  # a quiet mid-field state
    bit = 2 * 21 + 5
    first = [dict(q, c=20, dc=1),                                   # right wall
             dict(q, c=0, dc=-1, dr=-1),                            # left wall
             dict(q, r=0, c=0, dr=-1, dc=-1),                       # corner: wall and ceiling
             dict(q, r=0, c=5, dr=-1),                              # ceiling
             dict(q, r=6, c=4, dr=-1),                              # brick hit from below
             dict(q, r=6, c=4, dr=-1, bricks=1 << bit),             # the last brick: refill
             dict(q, r=6, c=4, dr=-1, bricks=FULL & ~(1 << bit)),   # the brick is gone: passes into the row
             dict(q, r=2, c=4, dr=1, dc=-1, k=2 ** 32 - 2)]         # brick hit from above
    second = [dict(q, r=19, c=8, p=10),                             # paddle, nc < p: steered left
              dict(q, r=19, c=9, p=10),                             # paddle, nc = p
              dict(q, r=19, c=12, dc=-1, p=10),                     # paddle, nc > p: steered right
              dict(q, r=19, c=11, p=10),                            # a miss unless the paddle moves right first
              dict(q, r=19, c=3, p=10, score=5),                    # miss
              dict(q, t=49, score=4),                               # truncation
              dict(q, t=49, score=4, r=19, c=3, p=10),              # a miss on the truncating step: once
              dict(q, t=49, score=4, r=6, c=4, dr=-1)]              # the truncating step's brick counts
    acts = [np.array([0, 1, 2, 3, 4, 5, 0, 1], np.int32), np.array([0, 0, 0, 2, 1, 0, 0, 0], np.int32)]
    return [{f: [s[f] for s in rnd] for f in q} for rnd in (first, second)], acts


def test_every_event_from_set_state():
    from freeimpala_amd import breakout, hip
    n, max_steps = 8, 50
    ref = breakout.breakout_reference(n, GAMMA, 4, max_steps)
    e = breakout.BreakoutEnv(n, GAMMA, 4, max_steps)
    d_act = hip.DeviceBuffer(n * 4)
    rounds, acts = scenario_states()
    for j, (fields, a) in enumerate(zip(rounds, acts)):
        before = e.read()
        ref.set_state(**fields)
        e.set_state(**fields)
        after = e.read()
        for nm in TENSORS[1:]:  # set_state leaves the scalars alone and renders
            np.testing.assert_array_equal(before[nm], after[nm], err_msg=nm)
        check_handle(e, ref, f"round {j}: after set_state")
        d_act.upload(a)
        e.step(d_act.ptr)
        ref.step(a)
        check_handle(e, ref, f"round {j}: after the step")
    assert ref.events == dict(wall=3, ceiling=2, brick=4, refill=1, paddle=4, steer=3, miss=2, truncation=3), ref.events
    assert ref.episodes == 4 and ref.return_sum == 5 + 4 + 4 + 5
    d_act.free()
    e.close()


# ------------------------------------------------------------------ 3. render
def test_render_fills_more_than_one_block():
    """N = 300: 132,300 pieces, 517 workgroups, the last one's lanes 204 .. 255 idle; the grid's
    corners, full, single-bit and random masks, the ball on a standing brick."""
    from freeimpala_amd import breakout, hip
    n = 300
    ref = breakout.breakout_reference(n, GAMMA, 9)
    rs = np.random.RandomState(2)
    s = ref.state()
    s["r"][:] = rs.randint(0, 20, n)
    s["c"][:] = rs.randint(0, 21, n)
    s["p"][:] = rs.randint(1, 20, n)
    s["bricks"][:] = (rs.randint(0, 2 ** 31, n).astype(np.uint64) << np.uint64(32)
                      | rs.randint(0, 2 ** 32, n, dtype=np.uint64)) | np.uint64(1)
    s["r"][:4], s["c"][:4], s["p"][:4] = (0, 0, 19, 19), (0, 20, 0, 20), (1, 19, 1, 19)
    s["bricks"][4:8] = FULL
    s["bricks"][8:12] = [1, 1 << 20, 1 << 21, 1 << 62]
    s["r"][12:15], s["c"][12:15] = (3, 4, 5), (0, 7, 20)  # the ball on a standing brick
    s["bricks"][12:15] = FULL
    s["r"][15], s["c"][15], s["bricks"][15] = 4, 7, FULL & ~(1 << 28)  # and on a cleared one
    ref.set_state(**s)
    assert (ref.planes[13] == 64).sum() == 16 * 62 and (ref.planes[15] == 64).sum() == 16 * 62
    g = Guarded([(8 * n, np.uint32), (n * PLANE, np.uint8)])
    hip.upload_ptr(g.ptr[0], breakout.pack_state(s))
    breakout.breakout_render(g.ptr[0], g.ptr[1], n)
    hip.synchronize()
    got = g.read(("state", "planes"))
    np.testing.assert_array_equal(got["planes"].reshape(n, 84, 84), ref.planes)
    np.testing.assert_array_equal(got["state"].reshape(n, 8), breakout.pack_state(s))  # read only
    g.free()


# ------------------------------------------------------------------ 4. totals
@pytest.mark.parametrize("n", [70, 300])
def test_totals_over_partial_waves_and_two_blocks(n):
    """Every environment truncates in one step: episodes = N and the exact sum of the scores."""
    from freeimpala_amd import breakout, hip
    max_steps = 1000
    e = breakout.BreakoutEnv(n, GAMMA, 6, max_steps)
    s = e.state()
    s["t"][:] = max_steps - 1
    s["score"][:] = (np.arange(n) * 211 + 5) % 65000
    e.set_state(**s)
    d_act = hip.DeviceBuffer.from_array(np.zeros(n, np.int32))
    e.step(d_act.ptr)
    assert e.stats() == dict(episodes=n, return_sum=int(s["score"].sum()))
    after = e.state()
    assert (after["k"] == 1).all() and (after["t"] == 0).all() and (after["score"] == 0).all()
    assert (e.read()["episode_start"] == 1).all() and (e.read()["discounts"] == 0).all()
    e.step(d_act.ptr)  # nothing ends: the totals stay
    assert e.stats() == dict(episodes=n, return_sum=int(s["score"].sum()))
    d_act.free()
    e.close()


# ------------------------------------------------------------------ 5. a recording actor and a learner
def test_rollout_records_equal_the_packed_reference_and_the_learner_steps_alike():
    """N = 5, T = 3: rollout(actor, T + 1), then rollout(actor, T). Environments 0 and 1 miss on steps
    3 and 5 (an episode start inside unroll 1), 2 takes a brick on step 2; 3 and 4 start as reset."""
    from freeimpala_amd import breakout
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner, pack_atari_plane_records, unpack_atari_plane_records
    from freeimpala_amd.rollout import split_unrolls
    n, T, A, seed, max_steps = 5, 3, 4, 5, 40
    on_dev, on_host = (DeviceLearner("atari", seq_len=T, batch=n, num_actions=A, records="planes", optimizer="adam",
                                     lr=1e-3) for _ in range(2))
    p0 = on_dev.get_params()
    on_host.set_params(p0)
    rec = Actor("atari", n, num_actions=A, seed=17)
    rec.set_params(p0)
    rec.begin_rollout(T)
    e = breakout.BreakoutEnv(n, GAMMA, seed, max_steps)
    ref = breakout.breakout_reference(n, GAMMA, seed, max_steps)
    s = ref.state()
    s["r"][:3], s["c"][:3], s["p"][:3], s["dr"][:3], s["dc"][:3] = (17, 15, 7), (2, 18, 9), (15, 3, 10), (1, 1, -1), (-1, 1, 1)
    ref.set_state(**s)
    e.set_state(**s)
    entries, dev_stats = [], []
    for k in range(2):
        assert e.rollout(rec, T + 1 if k == 0 else T) == (T + 1 if k == 0 else T)
        assert rec.rollout_ready()
        entries.append(rec.read_rollout())
        st = on_dev.step_rollout(rec)
        dev_stats.append({a: b for a, b in st.items() if a != "step_ms"})
        assert not rec.rollout_ready()
    # the reference stepped with the recorded actions
    rows = dict(planes=[], start=[], mu=[], act=[], rew=[], disc=[])
    for k in range(2):
        _, _, _, mu, act, _, _ = unpack_atari_plane_records(entries[k], T, n, A)
        for t in range(T):
            rows["planes"].append(ref.planes.copy())
            rows["start"].append(ref.episode_start.copy())
            ref.step(act[t])
            rows["mu"].append(mu[t])
            rows["act"].append(act[t])
            rows["rew"].append(ref.rewards.copy())
            rows["disc"].append(ref.discounts.copy())
    rows["planes"].append(ref.planes.copy())
    rows["start"].append(ref.episode_start.copy())
    h = {a: np.stack(b) for a, b in rows.items()}
    packed = [np.stack([np.frombuffer(x, np.uint8) for x in pack_atari_plane_records(*u)])
              for u in split_unrolls(h["planes"], h["start"], h["mu"], h["act"], h["rew"], h["disc"], T)]
    for k in range(2):
        assert entries[k].shape == packed[k].shape == (n, (T + 1) * 7168 + 21504)
        np.testing.assert_array_equal(entries[k], packed[k], err_msg=f"unroll {k}")
    # what the run held: starts inside both unrolls, a reward inside an episode, varying actions
    assert h["start"][3, 0] == 1 and h["start"][5, 1] == 1 and h["start"][1:].sum() == 2
    assert h["rew"][1, 2] == 1 and h["rew"].sum() == 1 and ref.events["miss"] == 2 and ref.events["brick"] == 1
    assert len(np.unique(h["act"])) > 1
    assert (h["planes"][1] != h["planes"][0]).any()
    for k in range(2):
        st = on_host.step([row for row in packed[k]])
        assert {a: b for a, b in st.items() if a != "step_ms"} == dev_stats[k], k
    assert dev_stats[1]["version"] == 2 and np.isfinite(dev_stats[1]["total_loss"])
    np.testing.assert_array_equal(on_dev.get_params(), on_host.get_params())
    assert on_dev.staging_bytes == 0
    rec.sync()
    rec.end_rollout()
    for x in (rec, e, on_dev, on_host):
        x.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from freeimpala_amd import breakout, env, hip
    from freeimpala_amd._abi import FiError
    for bad in (0, 65536, -1):
        with pytest.raises(FiError, match=rf"rc=-1: .*max_steps {bad} outside \[1, 65535\]"):
            breakout.BreakoutEnv(5, GAMMA, 1, max_steps=bad)
    with pytest.raises(FiError, match=r"rc=-1: .*num_envs"):
        breakout.BreakoutEnv(0, GAMMA, 1)
    with pytest.raises(FiError, match=r"rc=-1: .*gamma"):
        breakout.BreakoutEnv(5, 1.5, 1)
    for ok in (1, 65535):
        x = breakout.BreakoutEnv(2, GAMMA, 1, max_steps=ok)
        assert x.max_steps == ok
        x.close()
    n, max_steps = 5, 40
    e = breakout.BreakoutEnv(n, GAMMA, 3, max_steps)
    ref = breakout.breakout_reference(n, GAMMA, 3, max_steps)
    base = e.state()
    outside = dict(r=(-1, 20), c=(-1, 21), p=(0, 20), dr=(0, 2), dc=(0, -2), t=(-1, max_steps),
                   score=(-1, 65535 - max_steps + 1), bricks=(0, 1 << 63))
    for field, values in outside.items():
        for j, v in enumerate(values):
            s = {f: a.copy() for f, a in base.items()}
            i = (j + len(field)) % n
            s[field][i] = v
            shown = v if field != "bricks" else int(np.uint64(v))
            with pytest.raises(FiError, match=rf"rc=-1: .*{field}\[{i}\] = {shown} outside"):
                e.set_state(**s)
            check_handle(e, ref, f"{field} = {v}")  # nothing was written
    s = {f: a.copy() for f, a in base.items()}
    s["t"][:], s["score"][:], s["k"][:] = max_steps - 1, 65535 - 1, 2 ** 32 - 1  # the ranges' far ends are taken
    e.set_state(**s)
    ref.set_state(**s)
    check_handle(e, ref, "the far ends")
    # fi_env_read_state on a Breakout handle: words 0-3
    r, c, p = (np.empty(n, np.int32) for _ in range(3))
    k = np.empty(n, np.uint32)
    assert env.lib().fi_env_read_state(e._h, r.ctypes.data, c.ctypes.data, p.ctypes.data, k.ctypes.data) == 0
    for got, nm in ((r, "r"), (c, "c"), (p, "p"), (k, "k")):
        np.testing.assert_array_equal(got, s[nm])
    # the Breakout-only calls on a Catch handle
    catch = env.CatchEnv(n, GAMMA, 3)
    before = (str(catch.state()), catch.read())
    assert breakout.lib().fi_breakout_max_steps(catch._h) == 0
    with pytest.raises(FiError, match=r"rc=-1: .*breakout_read_state: a Catch handle"):
        breakout.read_state(catch._h, n)
    with pytest.raises(FiError, match=r"rc=-1: .*breakout_set_state: a Catch handle"):
        breakout.set_state(catch._h, n, **s)
    # the two kernels take device pointers: a handle is host memory and is refused before any launch
    d_act = hip.DeviceBuffer.from_array(np.zeros(n, np.int32))
    out = guarded(n)
    with pytest.raises(FiError, match=r"rc=-1: .*breakout_update: state_dev is not device memory"):
        breakout.breakout_update(catch._h.value, d_act.ptr, n, GAMMA, 3, max_steps, out.ptr[2], out.ptr[3], out.ptr[4],
                                 out.ptr[5])
    with pytest.raises(FiError, match=r"rc=-1: .*breakout_render: state_dev is not device memory"):
        breakout.breakout_render(catch._h.value, out.ptr[1], n)
    with pytest.raises(FiError, match=r"rc=-1: .*breakout_render: state_dev: the allocation ends"):
        breakout.breakout_render(out.ptr[0], out.ptr[1], n + 3)  # 3 states more than the buffer holds
    hip.synchronize()
    for nm, a in out.read(NAMES).items():
        assert (a.view(np.uint8) == 0xA5).all(), nm  # nothing was launched
    assert str(catch.state()) == before[0]
    for nm in TENSORS:
        np.testing.assert_array_equal(catch.read()[nm], before[1][nm])
    out.free()
    d_act.free()
    catch.close()
    e.close()


# ------------------------------------------------------------------ 7. the C++ check program
def test_cpp_check_program_prints_the_references_stats():
    from freeimpala_amd import breakout
    exe = os.path.join(ROOT, "build", "host_breakout_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_breakout_check"], check=True)
    runs = [subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    lines = [[ln for ln in r.stdout.splitlines() if ln.startswith("breakout ")] for r in runs]
    assert len(lines[0]) == 2 and lines[0] == lines[1], "a second run prints the same lines"
    n, T, max_steps = 3, 10, 16
    actions = np.array(lines[0][0].split(":")[1].split(), np.int32).reshape(2 * T, n)
    words = lines[0][1].split()
    val = {w: words[j + 1] for j, w in enumerate(words[:-1])}
    ref = breakout.breakout_reference(n, GAMMA, 5, max_steps)
    s = ref.state()
    s["r"][0], s["dr"][0], s["r"][1] = 7, -1, 12  # the program's first states
    ref.set_state(**s)
    ended = 0
    for a in actions:
        ref.step(a)
        ended += int((ref.discounts == 0).sum())
    assert ended == ref.episodes and ref.events["brick"] >= 1 and ref.episodes >= 1
    assert int(val["recorded_episodes"]) == ref.episodes and int(val["recorded_rewards"]) == ref.events["brick"]
    j = words.index("plane_sums")
    assert [int(w) for w in words[j + 1:j + 1 + n]] == [int(ref.planes[i].astype(np.int64).sum()) for i in range(n)]
    assert val["version"] == "2" and "nan" not in lines[0][1]
    assert ref.episodes <= int(val["final_episodes"]) <= ref.episodes + n
