"""CPU-side checks of rollouts recorded on the device (include/fi_rollout.h,
freeimpala_amd/rollout.py): split_unrolls, the host form of the recording rule and the GPU tests'
reference, is consistent with stack_planes; the library exports every function the header
declares and rollout.SIGNATURES binds exactly that set, none of it in the older headers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_split_unrolls_is_consistent_with_stack_planes():
    """Starts at record 0 of the run, mid-unroll, on a carry-over step and twice in a row: every
    unroll's (planes, history, start) rebuilds its slice of the whole run's stacks, byte for byte,
    and consecutive unrolls share their boundary step."""
    from freeimpala_amd.learner import stack_planes
    from freeimpala_amd.rollout import split_unrolls
    T, K, B, A = 3, 3, 4, 6
    S = K * T + 1
    rs = np.random.RandomState(3)
    planes = rs.randint(0, 256, (S, B, 84, 84)).astype(np.uint8)
    start = np.zeros((S, B), bool)
    start[0, :3] = True        # env 3 never starts: its first stacks hold the zero history
    start[1, 0] = True         # mid-unroll
    start[3, 1] = True         # on the carry-over step of unroll 0
    start[4, 2] = start[5, 2] = True  # twice in a row
    start[6, 0] = start[7, 0] = True  # a carry-over step and the step behind it
    mu = rs.standard_normal((S, B, A)).astype(np.float32)
    act = rs.randint(0, A, (S, B)).astype(np.int32)
    rew = rs.standard_normal((S, B)).astype(np.float32)
    disc = rs.rand(S, B).astype(np.float32)
    whole = stack_planes(planes, np.zeros((3, B, 84, 84), np.uint8), start)
    unrolls = split_unrolls(planes, start, mu, act, rew, disc, T)
    assert len(unrolls) == K
    for k, (p, h, s, m, a, r, d) in enumerate(unrolls):
        lo = k * T
        assert p.shape == (T + 1, B, 84, 84) and h.shape == (3, B, 84, 84) and s.shape == (T + 1, B)
        assert m.shape == (T, B, A) and a.shape == r.shape == d.shape == (T, B)
        np.testing.assert_array_equal(stack_planes(p, h, s), whole[lo:lo + T + 1], err_msg=f"unroll {k}")
        np.testing.assert_array_equal(p, planes[lo:lo + T + 1])
        np.testing.assert_array_equal(m, mu[lo:lo + T])
        np.testing.assert_array_equal(a, act[lo:lo + T])
        np.testing.assert_array_equal(r, rew[lo:lo + T])
        np.testing.assert_array_equal(d, disc[lo:lo + T])
        if k:
            np.testing.assert_array_equal(p[0], unrolls[k - 1][0][T])
            np.testing.assert_array_equal(s[0], unrolls[k - 1][2][T])
    assert (unrolls[0][1][:, 3] == 0).all() and (unrolls[0][1][:, 0] == planes[0, 0]).all()
    # the header arrays may stop at the last whole step
    again = split_unrolls(planes, start, mu[:-1], act[:-1], rew[:-1], disc[:-1], T)
    for u, v in zip(unrolls, again):
        for x, y in zip(u, v):
            np.testing.assert_array_equal(x, y)


def test_split_unrolls_refuses_a_run_that_is_not_whole_unrolls():
    import pytest
    from freeimpala_amd.rollout import split_unrolls
    z = np.zeros((6, 1, 84, 84), np.uint8)
    h = np.zeros((6, 1))
    with pytest.raises(ValueError):
        split_unrolls(z, h, np.zeros((6, 1, 2)), h, h, h, 3)
    with pytest.raises(ValueError):
        split_unrolls(z[:4], h[:4], np.zeros((2, 1, 2)), h[:2], h[:2], h[:2], 3)


def test_library_exports_every_rollout_header_symbol():
    from freeimpala_amd import _abi, actor, farmer, rollout
    lib = rollout.lib()
    names = header_functions("fi_rollout.h")
    for must in ("fi_rollout_begin", "fi_rollout_outcome", "fi_rollout_ready", "fi_rollout_acquire",
                 "fi_rollout_release", "fi_rollout_read", "fi_rollout_end", "fi_learner_step_entries_dev",
                 "fi_learner_step_entries_dev_async", "fi_learner_entries_consumed_event", "fi_learner_step_rollout",
                 "fi_record_plane_step", "fi_extract_history"):
        assert must in names, must
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(rollout.SIGNATURES), set(names) ^ set(rollout.SIGNATURES)
    for other in ("fi_learner.h", "fi_actor.h", "fi_farmer.h"):
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, actor.SIGNATURES, farmer.SIGNATURES):
        assert not set(names) & set(table)
