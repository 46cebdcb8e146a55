"""Host side of the second built-in device environment (include/fi_breakout.h): Breakout on 84x84
planes, where the ball's direction is visible only across frames.

``BreakoutEnv`` is an ``fi_env`` handle like ``CatchEnv`` and reuses its methods (``step``,
``tensors``, ``stats``, ``read``, ``rollout`` ...); it adds ``state()`` with all nine fields and
``set_state()``:

  env = BreakoutEnv(num_envs=256, gamma=0.99, seed=1, max_steps=1000)
  actor.begin_rollout(T)
  env.rollout(actor, T + 1)
  learner.step_rollout(actor)

This module holds the ctypes table of the header, ``BreakoutEnv``, the two standalone kernels and
``breakout_reference``, the numpy form of the rule (all integer arithmetic: the tests' reference,
byte for byte), which also counts every kind of event it sees."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, env
from ._abi import check
from .env import CELLS, LAST_ROW, PLANE_BYTES, CatchEnv, philox4  # noqa: F401

ST_BREAKOUT = 10  # the Philox stream of the resets (csrc/fi_common.h)
BRICK_ROW0, BRICK_ROWS, START_ROW = 3, 3, 6
FULL_MASK = (1 << 63) - 1
MAX_STEPS_LIMIT = 65535
STATE_WORDS = 8
FIELDS = ("r", "c", "p", "k", "dr", "dc", "t", "score", "bricks")
EVENTS = ("wall", "ceiling", "brick", "refill", "paddle", "steer", "miss", "truncation")

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_breakout.h declares
    "fi_breakout_create": ([C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_int32, C.POINTER(_P)], C.c_int),
    "fi_breakout_max_steps": ([_P], C.c_int32),
    "fi_breakout_read_state": ([_P] * 10, C.c_int),
    "fi_breakout_set_state": ([_P] * 10, C.c_int),
    "fi_breakout_update": ([_P, _P, C.c_int, C.c_float, C.c_uint64, C.c_int32, _P, _P, _P, _P, _P], C.c_int),
    "fi_breakout_render": ([_P, _P, C.c_int, _P], C.c_int),
}
_bound = None


def lib():
    global _bound
    L = env.lib()
    if _bound is not L:
        for name, (args, res) in SIGNATURES.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = L
    return L


_DTYPES = dict(r=np.int32, c=np.int32, p=np.int32, k=np.uint32, dr=np.int32, dc=np.int32, t=np.int32, score=np.int32,
               bricks=np.uint64)


def read_state(handle, n: int) -> dict:
    """fi_breakout_read_state on a raw fi_env handle of n environments."""
    out = {f: np.empty(n, _DTYPES[f]) for f in FIELDS}
    check(lib().fi_breakout_read_state(handle, *[out[f].ctypes.data for f in FIELDS]), "fi_breakout_read_state")
    return out


def set_state(handle, n: int, **fields) -> None:
    """fi_breakout_set_state on a raw fi_env handle of n environments: all nine fields, n values each."""
    if set(fields) != set(FIELDS):
        raise ValueError(f"set_state takes exactly {FIELDS}")
    a = {f: np.ascontiguousarray(np.asarray(fields[f]).astype(_DTYPES[f]).reshape(n)) for f in FIELDS}
    check(lib().fi_breakout_set_state(handle, *[a[f].ctypes.data for f in FIELDS]), "fi_breakout_set_state")


class BreakoutEnv(CatchEnv):
    """N Breakout environments on the device: an fi_env handle, so everything ``CatchEnv`` does
    works on it; ``state()`` returns all nine fields and ``set_state()`` writes them."""

    def __init__(self, num_envs: int, gamma: float = 0.99, seed: int = 0, max_steps: int = 1000, device: int = 0):
        self._h = _P()
        check(lib().fi_breakout_create(device, num_envs, gamma, seed, max_steps, C.byref(self._h)), "fi_breakout_create")
        self.N, self.gamma, self.seed, self.device = num_envs, float(np.float32(gamma)), seed, device
        self.max_steps = lib().fi_breakout_max_steps(self._h)

    def state(self) -> dict:
        """r, c, p, dr, dc, t, score (int32), k (uint32) and bricks (uint64) of every environment,
        after the last step."""
        return read_state(self._h, self.N)

    def set_state(self, **fields) -> None:
        """Write the state of every environment (all nine fields of ``state()``) and render it.
        episode_start, rewards, discounts and the totals stay; nothing may be in flight."""
        set_state(self._h, self.N, **fields)


def breakout_update(state_ptr: int, actions_ptr: int, n: int, gamma: float, seed: int, max_steps: int, start_ptr: int,
                    rewards_ptr: int, discounts_ptr: int, totals_ptr=None, stream=None) -> None:
    """fi_breakout_update on device pointers."""
    check(lib().fi_breakout_update(state_ptr, actions_ptr, n, gamma, seed, max_steps, start_ptr, rewards_ptr,
                                   discounts_ptr, totals_ptr, stream), "fi_breakout_update")


def breakout_render(state_ptr: int, planes_ptr: int, n: int, stream=None) -> None:
    """fi_breakout_render on device pointers."""
    check(lib().fi_breakout_render(state_ptr, planes_ptr, n, stream), "fi_breakout_render")


def pack_state(s: dict) -> np.ndarray:
    """The nine fields as the (N, 8) uint32 words of device memory."""
    n = len(s["r"])
    w = np.zeros((n, STATE_WORDS), np.uint32)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = s["r"], s["c"], s["p"], s["k"]
    w[:, 4] = (np.asarray(s["dc"]) > 0).astype(np.uint32) | ((np.asarray(s["dr"]) > 0).astype(np.uint32) << 1)
    w[:, 5] = np.asarray(s["t"]).astype(np.uint32) | (np.asarray(s["score"]).astype(np.uint32) << 16)
    b = np.asarray(s["bricks"], np.uint64)
    w[:, 6] = (b & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w[:, 7] = (b >> np.uint64(32)).astype(np.uint32)
    return w


# ---------------------------------------------------------------------- the rule on the host
class BreakoutReference:
    """The rule of include/fi_breakout.h in numpy. After construction and after every ``step`` the
    attributes hold what the device handle holds: ``planes`` (N, 84, 84) uint8, ``episode_start``
    (N,) uint8, ``rewards`` and ``discounts`` (N,) float32, the state ``r``, ``c``, ``p``, ``dr``,
    ``dc``, ``t``, ``score`` (int32), ``k`` (uint32) and ``bricks`` (uint64), and the totals
    ``episodes`` and ``return_sum`` (Python ints). ``events`` counts what happened since
    construction, one counter per name of ``EVENTS``; a steer is a paddle hit off the centre."""

    def __init__(self, num_envs: int, gamma: float = 0.99, seed: int = 0, max_steps: int = 1000):
        if not 1 <= max_steps <= MAX_STEPS_LIMIT:
            raise ValueError("max_steps outside [1, 65535]")
        self.N, self.gamma, self.seed, self.max_steps = num_envs, np.float32(gamma), seed, max_steps
        for f in FIELDS:
            setattr(self, f, np.zeros(num_envs, _DTYPES[f]))
        for i in range(num_envs):
            self._reset(i)
        self.episode_start = np.ones(num_envs, np.uint8)
        self.rewards = np.zeros(num_envs, np.float32)
        self.discounts = np.zeros(num_envs, np.float32)
        self.episodes, self.return_sum = 0, 0
        self.events = dict.fromkeys(EVENTS, 0)
        self.planes = self.render()

    def _reset(self, i: int) -> None:
        w = philox4(self.seed, np.array([int(self.k[i]) * self.N + i], np.uint64), ST_BREAKOUT)[0]
        self.c[i] = (int(w[0]) * CELLS) >> 32
        self.p[i] = 1 + ((int(w[1]) * 19) >> 32)
        self.dc[i] = 1 if int(w[2]) & 1 else -1
        self.r[i], self.dr[i], self.t[i], self.score[i] = START_ROW, 1, 0, 0
        self.bricks[i] = FULL_MASK

    def render(self) -> np.ndarray:
        cy, cx = np.arange(84)[:, None] >> 2, np.arange(84)[None, :] >> 2
        out = np.zeros((self.N, 84, 84), np.uint8)
        for i in range(self.N):
            mask = int(self.bricks[i])
            rows = np.zeros((CELLS, CELLS), bool)
            for b in range(BRICK_ROWS * CELLS):
                rows[BRICK_ROW0 + b // CELLS, b % CELLS] = (mask >> b) & 1
            out[i][rows[cy, cx]] = 64
            out[i][(cy == LAST_ROW) & (np.abs(cx - self.p[i]) <= 1)] = 128
            out[i][(cy == self.r[i]) & (cx == self.c[i])] = 255
        return out

    def step(self, actions) -> None:
        a = np.asarray(actions, np.int64).reshape(self.N)
        if (a < 0).any():
            raise ValueError("actions must be >= 0")
        ev = self.events
        for i in range(self.N):
            r, c, p, dr, dc = (int(getattr(self, f)[i]) for f in ("r", "c", "p", "dr", "dc"))
            t, score, mask = int(self.t[i]), int(self.score[i]), int(self.bricks[i])
            m = int(a[i]) % 3
            p = min(max(p + (m == 2) - (m == 1), 1), 19)
            nc = c + dc
            if nc < 0 or nc > CELLS - 1:
                dc = -dc
                nc = c + dc
                ev["wall"] += 1
            nr = r + dr
            if nr < 0:
                dr = 1
                nr = r + dr
                ev["ceiling"] += 1
            reward, ended = 0.0, False
            bit = (nr - BRICK_ROW0) * CELLS + nc
            if BRICK_ROW0 <= nr < BRICK_ROW0 + BRICK_ROWS and (mask >> bit) & 1:
                mask &= ~(1 << bit)
                reward = 1.0
                score += 1
                dr = -dr
                nr = r
                ev["brick"] += 1
                if mask == 0:
                    mask = FULL_MASK
                    ev["refill"] += 1
            elif nr == LAST_ROW and abs(nc - p) <= 1:
                dr = -1
                nr = r
                ev["paddle"] += 1
                if nc != p:
                    dc = -1 if nc < p else 1
                    ev["steer"] += 1
            elif nr == LAST_ROW:
                ended = True
                ev["miss"] += 1
            r, c = nr, nc
            t += 1
            if t == self.max_steps:
                ended = True
                ev["truncation"] += 1
            self.rewards[i] = reward
            self.p[i] = p
            if ended:
                self.discounts[i] = 0.0
                self.episode_start[i] = 1
                self.episodes += 1
                self.return_sum += score
                self.k[i] += 1
                self._reset(i)
            else:
                self.discounts[i] = self.gamma
                self.episode_start[i] = 0
                self.r[i], self.c[i], self.dr[i], self.dc[i] = r, c, dr, dc
                self.t[i], self.score[i], self.bricks[i] = t, score, mask
        self.planes = self.render()

    def state(self) -> dict:
        return {f: getattr(self, f).copy() for f in FIELDS}

    def set_state(self, **fields) -> None:
        """The host form of ``BreakoutEnv.set_state``: the nine fields, then the render."""
        if set(fields) != set(FIELDS):
            raise ValueError(f"set_state takes exactly {FIELDS}")
        for f in FIELDS:
            setattr(self, f, np.asarray(fields[f]).astype(_DTYPES[f]).reshape(self.N).copy())
        self.planes = self.render()


def breakout_reference(num_envs: int, gamma: float = 0.99, seed: int = 0, max_steps: int = 1000) -> BreakoutReference:
    """N host environments in their first state (Reset(i, 0), episode_start = 1)."""
    return BreakoutReference(num_envs, gamma, seed, max_steps)
