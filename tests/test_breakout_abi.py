"""CPU-side checks of the Breakout environment's ABI (include/fi_breakout.h): the in-tree
libfi_learner.so exports every function the header declares, freeimpala_amd.breakout binds exactly
that set, the ten older headers and their tables are what they were, and breakout_reference -- the
host form of the rule -- does what the rule says, one event at a time from states written by hand,
and in a random run that meets every event a short run can meet."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("fi_breakout_create", "fi_breakout_max_steps", "fi_breakout_read_state", "fi_breakout_set_state",
             "fi_breakout_update", "fi_breakout_render")
# the older headers' functions, as the ABI tests before this header pin them
OLDER = {"fi_learner.h": 43, "fi_farmer.h": 13, "fi_actor.h": 17, "fi_rollout.h": 15, "fi_gather.h": 7,
         "fi_ring.h": 14, "fi_prio.h": 9, "fi_weights.h": 9, "fi_env.h": 17, "fi_train.h": 8}
FULL = (1 << 63) - 1


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_breakout_header_symbol():
    from freeimpala_amd import breakout
    lib = breakout.lib()
    names = header_functions("fi_breakout.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(breakout.SIGNATURES), set(names) ^ set(breakout.SIGNATURES)
    assert lib.fi_abi_version() == 1
    assert breakout.ST_BREAKOUT == 10
    src = open(os.path.join(ROOT, "freeimpala_amd", "csrc", "fi_common.h")).read()
    assert re.search(r"ST_ENV = 9, ST_BREAKOUT = 10\b", src)


def test_older_headers_and_tables_are_unchanged():
    from freeimpala_amd import _abi, actor, breakout, env, farmer, gather, prio, ring, rollout, train, weights
    tables = {"fi_learner.h": _abi.SIGNATURES, "fi_farmer.h": farmer.SIGNATURES, "fi_actor.h": actor.SIGNATURES,
              "fi_rollout.h": rollout.SIGNATURES, "fi_gather.h": gather.SIGNATURES, "fi_ring.h": ring.SIGNATURES,
              "fi_prio.h": prio.SIGNATURES, "fi_weights.h": weights.SIGNATURES, "fi_env.h": env.SIGNATURES,
              "fi_train.h": train.SIGNATURES}
    assert tables.keys() == OLDER.keys()
    lib = breakout.lib()
    new = set(header_functions("fi_breakout.h"))
    for header, table in tables.items():
        old = header_functions(header)
        assert not new & set(old), header
        assert not new & set(table), header
        assert set(table) <= set(old) | {"fi_abi_version", "fi_last_error"}, header
        assert len(table) == OLDER[header], (header, len(table))
        assert not [n for n in table if not hasattr(lib, n)], header
    assert len(header_functions("fi_env.h")) == 17


# ---------------------------------------------------------------------- one event at a time
def one(max_steps=1000, gamma=0.5, **fields):
    """One environment in a state written by hand; what is not given is a quiet mid-field state."""
    from freeimpala_amd.breakout import breakout_reference
    ref = breakout_reference(1, gamma, seed=1, max_steps=max_steps)
    s = dict(r=10, c=10, p=10, k=7, dr=1, dc=1, t=3, score=2, bricks=FULL)
    s.update(fields)
    ref.set_state(**{f: [v] for f, v in s.items()})
    return ref


def got(ref, *names):
    return tuple(int(getattr(ref, n)[0]) for n in names)


def only(ref, **counts):
    want = dict.fromkeys(ref.events, 0)
    want.update(counts)
    assert ref.events == want, (ref.events, want)


def quiet(ref, gamma=0.5):
    assert ref.rewards[0] == 0 and ref.discounts[0] == np.float32(gamma) and ref.episode_start[0] == 0
    assert (ref.episodes, ref.return_sum) == (0, 0)


def test_reference_walls_and_corner():
    ref = one(c=20, dc=1)
    ref.step([0])
    assert got(ref, "r", "c", "dr", "dc", "t", "score") == (11, 19, 1, -1, 4, 2)
    only(ref, wall=1)
    quiet(ref)
    ref = one(c=0, dc=-1, dr=-1)
    ref.step([0])
    assert got(ref, "r", "c", "dr", "dc") == (9, 1, -1, 1)
    only(ref, wall=1)
    ref = one(r=0, c=0, dr=-1, dc=-1)  # a corner: both turn in one step
    ref.step([0])
    assert got(ref, "r", "c", "dr", "dc") == (1, 1, 1, 1)
    only(ref, wall=1, ceiling=1)
    quiet(ref)


def test_reference_ceiling():
    ref = one(r=0, c=5, dr=-1, dc=1)
    ref.step([0])
    assert got(ref, "r", "c", "dr", "dc") == (1, 6, 1, 1)
    only(ref, ceiling=1)
    quiet(ref)


def test_reference_brick_hit_and_refill():
    ref = one(r=6, c=4, dr=-1, dc=1)  # moves into (5, 5): bit 2 * 21 + 5
    ref.step([0])
    bit = 2 * 21 + 5
    assert got(ref, "r", "c", "dr", "dc", "score", "t") == (6, 5, 1, 1, 3, 4)  # the row unchanged, dr flipped
    assert int(ref.bricks[0]) == FULL & ~(1 << bit)
    assert ref.rewards[0] == 1 and ref.discounts[0] == np.float32(0.5) and ref.episode_start[0] == 0
    only(ref, brick=1)
    # from above, moving down into row 3
    ref = one(r=2, c=4, dr=1, dc=-1)
    ref.step([0])
    assert got(ref, "r", "c", "dr") == (2, 3, -1) and int(ref.bricks[0]) == FULL & ~(1 << 3)
    # a cell whose brick is gone is passed through; the ball may then stand on a standing brick's row
    ref = one(r=6, c=4, dr=-1, dc=1, bricks=FULL & ~(1 << bit))
    ref.step([0])
    assert got(ref, "r", "c", "dr") == (5, 5, -1) and ref.rewards[0] == 0
    only(ref)
    # the last brick refills the mask
    ref = one(r=6, c=4, dr=-1, dc=1, bricks=1 << bit)
    ref.step([0])
    assert int(ref.bricks[0]) == FULL and ref.rewards[0] == 1 and got(ref, "r", "score") == (6, 3)
    only(ref, brick=1, refill=1)


@pytest.mark.parametrize("c0,dc0,p,want_c,want_dc,steer", [(8, 1, 10, 9, -1, 1), (9, 1, 10, 10, 1, 0),
                                                           (11, -1, 10, 10, -1, 0), (10, 1, 10, 11, 1, 1),
                                                           (12, -1, 10, 11, 1, 1)])
def test_reference_paddle(c0, dc0, p, want_c, want_dc, steer):
    ref = one(r=19, c=c0, dr=1, dc=dc0, p=p)
    ref.step([0])
    assert got(ref, "r", "c", "dr", "dc", "p") == (19, want_c, -1, want_dc, p)
    only(ref, paddle=1, steer=steer)
    quiet(ref)


def test_reference_paddle_moves_before_the_ball_is_tested():
    ref = one(r=19, c=11, dr=1, dc=1, p=10)  # nc = 12: a miss unless the paddle moves right first
    ref.step([2])
    assert got(ref, "r", "c", "dr", "dc", "p") == (19, 12, -1, 1, 11)
    only(ref, paddle=1, steer=1)


def test_reference_miss_truncation_and_both_at_once():
    ref = one(r=19, c=3, dr=1, dc=1, p=10, score=5, k=7)
    ref.step([0])
    assert ref.rewards[0] == 0 and ref.discounts[0] == 0 and ref.episode_start[0] == 1
    assert (ref.episodes, ref.return_sum) == (1, 5)
    assert got(ref, "r", "dr", "t", "score", "k") == (6, 1, 0, 0, 8) and int(ref.bricks[0]) == FULL
    only(ref, miss=1)
    ref = one(max_steps=9, t=8, score=4)  # truncation in mid-field
    ref.step([0])
    assert ref.discounts[0] == 0 and ref.episode_start[0] == 1 and (ref.episodes, ref.return_sum) == (1, 4)
    assert got(ref, "r", "t", "score", "k") == (6, 0, 0, 8)
    only(ref, truncation=1)
    ref = one(max_steps=9, t=8, score=4, r=6, c=4, dr=-1, dc=1)  # the truncating step's brick still counts
    ref.step([0])
    assert ref.rewards[0] == 1 and (ref.episodes, ref.return_sum) == (1, 5)
    ref = one(max_steps=9, t=8, score=4, r=19, c=3, dr=1, dc=1, p=10)  # a miss on the truncating step: once
    ref.step([0])
    assert (ref.episodes, ref.return_sum) == (1, 4) and got(ref, "k", "t") == (8, 0)
    only(ref, miss=1, truncation=1)


def test_reference_plane_pixel_counts():
    from freeimpala_amd.breakout import PLANE_BYTES
    rs = np.random.RandomState(5)
    for trial in range(6):
        mask = [FULL, 1, 1 << 62, int(rs.randint(1, 2 ** 31)) | int(rs.randint(0, 2 ** 31)) << 32][trial % 4]
        on_brick = trial >= 4
        r, c = (4, 7) if on_brick else (int(rs.randint(6, 20)), int(rs.randint(0, 21)))
        if on_brick:
            mask |= 1 << (21 + 7)
        ref = one(r=r, c=c, bricks=mask, p=int(rs.randint(1, 20)))
        pl = ref.planes[0]
        assert pl.shape == (84, 84) and pl.dtype == np.uint8 and pl.size == PLANE_BYTES
        assert (pl == 255).sum() == 16 and (pl == 128).sum() == 48
        assert (pl == 64).sum() == 16 * bin(mask).count("1") - (16 if on_brick else 0)
        assert set(np.unique(pl)) <= {0, 64, 128, 255}
        assert (pl[80:84, 4 * (int(ref.p[0]) - 1):4 * (int(ref.p[0]) + 2)] == 128).all()


def random_run(seed):
    """N = 5, max_steps = 40, 120 steps of RandomState(seed) actions: the run of the GPU parity test."""
    from freeimpala_amd.breakout import breakout_reference
    ref = breakout_reference(5, 0.99, seed, max_steps=40)
    actions = np.random.RandomState(seed).randint(0, 4, (120, 5))
    trace = [ref.state()]
    for a in actions:
        ref.step(a)
        trace.append(ref.state())
    return ref, trace


@pytest.mark.parametrize("seed", [1, 3])
def test_reference_random_run_meets_every_short_run_event(seed):
    ref, trace = random_run(seed)
    for ev in ("wall", "brick", "paddle", "miss", "truncation"):
        assert ref.events[ev] >= 1, (ev, ref.events)
    assert ref.events["ceiling"] == 0 and ref.events["refill"] == 0  # those come from set_state
    assert ref.episodes == ref.events["miss"] + ref.events["truncation"] and ref.return_sum == ref.events["brick"]
    for s in trace:
        assert ((0 <= s["r"]) & (s["r"] <= 19) & (0 <= s["c"]) & (s["c"] <= 20) & (1 <= s["p"]) & (s["p"] <= 19)).all()
        assert (np.abs(s["dr"]) == 1).all() and (np.abs(s["dc"]) == 1).all() and (s["t"] < 40).all()
    if seed == 1:
        assert [ref.events[e] for e in ("wall", "brick", "paddle", "miss", "truncation")] == [30, 5, 5, 25, 5]


def test_reference_same_seed_same_run_another_seed_another():
    a, ta = random_run(1)
    b, tb = random_run(1)
    np.testing.assert_array_equal(a.planes, b.planes)
    assert a.events == b.events and str(ta) == str(tb)
    from freeimpala_amd.breakout import breakout_reference
    x, y = breakout_reference(5, 0.99, 1, 40), breakout_reference(5, 0.99, 2, 40)
    assert (x.c != y.c).any() or (x.p != y.p).any() or (x.dc != y.dc).any()
    assert (x.r == 6).all() and (x.dr == 1).all() and (x.t == 0).all() and (x.bricks == np.uint64(FULL)).all()
    assert (x.episode_start == 1).all() and (x.rewards == 0).all() and (x.discounts == 0).all()
    try:
        x.step([-1, 0, 0, 0, 0])
    except ValueError:
        pass
    else:
        raise AssertionError("a negative action is outside the rule")
