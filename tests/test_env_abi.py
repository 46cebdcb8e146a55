"""CPU-side checks of the device environments' ABI (include/fi_env.h): the in-tree libfi_learner.so
exports every function the header declares, freeimpala_amd.env binds exactly that set, the seven
older headers and their tables are what they were, and catch_reference -- the host form of the
environment's rule -- has the properties the rule promises, with its Philox words checked against
the oracle's."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("fi_actor_act_planes_dev", "fi_actor_act_obs_dev", "fi_actor_outputs_dev", "fi_rollout_outcome_dev",
             "fi_actor_sync", "fi_actor_stream", "fi_env_create", "fi_env_destroy", "fi_env_num_envs", "fi_env_step", "fi_env_tensors",
             "fi_env_stepped_event", "fi_env_read_state", "fi_env_stats", "fi_env_rollout", "fi_env_update",
             "fi_env_render")
# the older headers' functions, counted when this header was added
OLDER = {"fi_learner.h": 43, "fi_farmer.h": 13, "fi_actor.h": 17, "fi_rollout.h": 15, "fi_gather.h": 7,
         "fi_ring.h": 14, "fi_prio.h": 9}


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_env_header_symbol():
    from freeimpala_amd import env
    lib = env.lib()
    names = header_functions("fi_env.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(env.SIGNATURES), set(names) ^ set(env.SIGNATURES)
    assert lib.fi_abi_version() == 1


def test_older_headers_and_tables_are_unchanged():
    from freeimpala_amd import _abi, actor, env, farmer, gather, prio, ring, rollout
    tables = {"fi_learner.h": _abi.SIGNATURES, "fi_farmer.h": farmer.SIGNATURES, "fi_actor.h": actor.SIGNATURES,
              "fi_rollout.h": rollout.SIGNATURES, "fi_gather.h": gather.SIGNATURES, "fi_ring.h": ring.SIGNATURES,
              "fi_prio.h": prio.SIGNATURES}
    lib = env.lib()
    new = set(header_functions("fi_env.h"))
    for header, table in tables.items():
        old = header_functions(header)
        assert not new & set(old), header
        assert not new & set(table), header
        assert set(table) <= set(old) | {"fi_abi_version", "fi_last_error"}, header
        assert len(table) == OLDER[header], (header, len(table))
        assert not [n for n in table if not hasattr(lib, n)], header


def test_philox_words_are_the_oracles(orc):
    from freeimpala_amd.env import ST_ENV, philox4
    assert ST_ENV == 9
    counters = [0, 1, 4, 5 * 7 + 3, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17, 2 ** 64 - 1]
    for seed in (0, 7, 2 ** 63 + 11, 2 ** 64 - 1):
        got = philox4(seed, np.array(counters, np.uint64), ST_ENV)
        for j, e in enumerate(counters):
            np.testing.assert_array_equal(got[j], orc.philox4(seed, e, ST_ENV), err_msg=f"seed {seed}, counter {e}")


def test_catch_reference_keeps_the_rules_promises():
    from freeimpala_amd.env import PLANE_BYTES, catch_reference
    N, STEPS, gamma = 5, 60, 0.99
    ref = catch_reference(N, gamma, seed=3)
    actions = np.random.RandomState(0).randint(0, 4, (STEPS, N))  # A = 4: a mod 3 wraps
    assert (ref.episode_start == 1).all() and (ref.r == 0).all() and (ref.k == 0).all()
    assert ((0 <= ref.c) & (ref.c <= 20) & (1 <= ref.p) & (ref.p <= 19)).all()
    firsts = [(ref.c.copy(), ref.p.copy())]
    for t in range(STEPS):
        assert ref.planes.shape == (N, 84, 84) and ref.planes.dtype == np.uint8 and ref.planes[0].size == PLANE_BYTES
        for i in range(N):
            # the ball never shares a cell with the paddle before the step that ends the episode
            assert (ref.planes[i] == 255).sum() == 16 and (ref.planes[i] == 128).sum() == 48, (t, i)
            assert set(np.unique(ref.planes[i])) == {0, 128, 255}
        c, p, r = ref.c.copy(), ref.p.copy(), ref.r.copy()
        ref.step(actions[t])
        last = (t + 1) % 20 == 0  # every episode lasts exactly 20 steps
        m = actions[t] % 3
        moved = np.clip(p + (m == 2) - (m == 1), 1, 19)
        if last:
            want = np.where(np.abs(c - moved) <= 1, 1.0, -1.0)
            np.testing.assert_array_equal(ref.rewards, want.astype(np.float32))
            assert (ref.discounts == 0).all() and (ref.episode_start == 1).all()
            assert (ref.r == 0).all() and (ref.k == (t + 1) // 20).all()
            firsts.append((ref.c.copy(), ref.p.copy()))
        else:
            assert (ref.rewards == 0).all() and (ref.discounts == np.float32(gamma)).all()
            assert (ref.episode_start == 0).all()
            assert (ref.r == r + 1).all() and (ref.c == c).all() and (ref.p == moved).all()
    assert ref.episodes == 3 * N and -3 * N <= ref.return_sum <= 3 * N
    assert (ref.k == 3).all()
    # the resets draw: not every episode of every environment starts in one place
    assert len({(int(c[i]), int(p[i])) for c, p in firsts for i in range(N)}) > N
    # the same seed gives the same run, another seed another
    again = catch_reference(N, gamma, seed=3)
    np.testing.assert_array_equal(again.c, firsts[0][0])
    other = catch_reference(N, gamma, seed=4)
    assert (other.c != firsts[0][0]).any() or (other.p != firsts[0][1]).any()


def test_catch_reference_paddle_and_actions():
    from freeimpala_amd.env import catch_reference
    ref = catch_reference(3, 0.5, seed=1)
    ref.p[:] = (1, 10, 19)
    ref.step([1, 1, 2])  # left at the left wall, left, right at the right wall
    assert list(ref.p) == [1, 9, 19]
    ref.step([3, 4, 5])  # 3 mod 3 = stay, 4 = left, 5 = right (clamped)
    assert list(ref.p) == [1, 8, 19]
    assert (ref.discounts == np.float32(0.5)).all()
    try:
        ref.step([-1, 0, 0])
    except ValueError:
        pass
    else:
        raise AssertionError("a negative action is outside the rule")
