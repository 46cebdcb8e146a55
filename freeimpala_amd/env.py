"""Host side of device-resident environments (include/fi_env.h).

An ``Actor`` acts on observations that are in device memory already and only enqueues; ``CatchEnv``
is the built-in environment (Catch on 84x84 planes, N environments whose state lives on the device);
``CatchEnv.rollout`` enqueues a whole unroll -- act, environment step, outcome, record -- on the
actor's stream without the host waiting once:

  env = CatchEnv(num_envs=1024, gamma=0.99, seed=1)
  actor.begin_rollout(T)
  env.rollout(actor, T + 1)            # returns at once
  while True:
      learner.step_rollout(actor)      # waits on the device for the unroll's event
      env.rollout(actor, T)

This module holds the ctypes table of the header, ``CatchEnv``, and ``catch_reference``, the numpy
form of the environment's rule (all integer arithmetic: the tests' reference, byte for byte). The
actor's methods (``act_planes_dev``, ``act_obs_dev``, ``outputs_dev``, ``outcome_dev``, ``sync``)
live on ``Actor``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

ST_ENV = 9  # the Philox stream of the resets (csrc/fi_common.h)
CELLS, LAST_ROW, EPISODE_STEPS = 21, 20, 20
PLANE_BYTES = 84 * 84

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_env.h declares
    "fi_actor_act_planes_dev": ([_P, _P, _P, _P], C.c_int),
    "fi_actor_act_obs_dev": ([_P, _P, _P], C.c_int),
    "fi_actor_outputs_dev": ([_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)], C.c_int),
    "fi_rollout_outcome_dev": ([_P, _P, _P, _P], C.c_int),
    "fi_actor_sync": ([_P, C.POINTER(C.c_int64)], C.c_int),
    "fi_actor_stream": ([_P], _P),
    "fi_env_create": ([C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.POINTER(_P)], C.c_int),
    "fi_env_destroy": ([_P], None),
    "fi_env_num_envs": ([_P], C.c_int32),
    "fi_env_step": ([_P, _P, _P, _P], C.c_int),
    "fi_env_tensors": ([_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)], C.c_int),
    "fi_env_stepped_event": ([_P], _P),
    "fi_env_read_state": ([_P, _P, _P, _P, _P], C.c_int),
    "fi_env_stats": ([_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)], C.c_int),
    "fi_env_rollout": ([_P, _P, C.c_int32, C.POINTER(C.c_int32)], C.c_int),
    "fi_env_update": ([_P, _P, C.c_int, C.c_float, C.c_uint64, _P, _P, _P, _P, _P], C.c_int),
    "fi_env_render": ([_P, _P, C.c_int, _P], C.c_int),
}
_bound = None


def lib():
    global _bound
    L = _abi.lib()
    if _bound is not L:
        for name, (args, res) in SIGNATURES.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = L
    return L


class CatchEnv:
    """N Catch environments on the device. ``tensors()`` gives the device pointers an actor acts on."""

    def __init__(self, num_envs: int, gamma: float = 0.99, seed: int = 0, device: int = 0):
        self._h = _P()
        check(lib().fi_env_create(device, num_envs, gamma, seed, C.byref(self._h)), "fi_env_create")
        self.N, self.gamma, self.seed, self.device = num_envs, float(np.float32(gamma)), seed, device

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().fi_env_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, actions_ptr: int, ready_event=None, stream=None) -> None:
        """Enqueue one step with N int32 actions in device memory; nothing waits."""
        check(lib().fi_env_step(self._h, actions_ptr, ready_event, stream), "fi_env_step")

    def tensors(self) -> dict:
        """Device pointers: planes u8[N*7056], episode_start u8[N], rewards and discounts float[N]."""
        p = [_P() for _ in range(4)]
        check(lib().fi_env_tensors(self._h, *[C.byref(x) for x in p]), "fi_env_tensors")
        return dict(zip(("planes", "episode_start", "rewards", "discounts"), [x.value for x in p]))

    @property
    def stepped_event(self) -> int | None:
        return lib().fi_env_stepped_event(self._h)

    def state(self) -> dict:
        """r, c, p (int32) and k (uint32) of every environment, after the last step."""
        r, c, p = (np.empty(self.N, np.int32) for _ in range(3))
        k = np.empty(self.N, np.uint32)
        check(lib().fi_env_read_state(self._h, r.ctypes.data, c.ctypes.data, p.ctypes.data, k.ctypes.data),
              "fi_env_read_state")
        return dict(r=r, c=c, p=p, k=k)

    def stats(self) -> dict:
        """Finished episodes and the sum of their returns since create (exact integers)."""
        n, s = C.c_uint64(0), C.c_int64(0)
        check(lib().fi_env_stats(self._h, C.byref(n), C.byref(s)), "fi_env_stats")
        return dict(episodes=n.value, return_sum=s.value)

    def read(self) -> dict:
        """The four tensors copied to the host, after the last step (tests and host-stepped loops)."""
        from . import hip
        check(lib().fi_env_read_state(self._h, None, None, None, None), "fi_env_read_state")  # waits
        t = self.tensors()
        return dict(planes=hip.download_ptr(t["planes"], np.uint8, (self.N, 84, 84)),
                    episode_start=hip.download_ptr(t["episode_start"], np.uint8, (self.N,)),
                    rewards=hip.download_ptr(t["rewards"], np.float32, (self.N,)),
                    discounts=hip.download_ptr(t["discounts"], np.float32, (self.N,)))

    def rollout(self, actor, n_steps: int) -> int:
        """Enqueue n_steps of act -> step -> outcome on the actor's stream and return the number
        enqueued. A refusal of an act call raises FiError; ``steps_enqueued`` rides on it."""
        n = C.c_int32(0)
        rc = lib().fi_env_rollout(self._h, actor._h, n_steps, C.byref(n))
        try:
            check(rc, "fi_env_rollout")
        except _abi.FiError as e:
            e.steps_enqueued = n.value
            raise
        return n.value


def env_update(state_ptr: int, actions_ptr: int, n: int, gamma: float, seed: int, start_ptr: int, rewards_ptr: int,
               discounts_ptr: int, totals_ptr=None, stream=None) -> None:
    """fi_env_update on device pointers."""
    check(lib().fi_env_update(state_ptr, actions_ptr, n, gamma, seed, start_ptr, rewards_ptr, discounts_ptr,
                              totals_ptr, stream), "fi_env_update")


def env_render(state_ptr: int, planes_ptr: int, n: int, stream=None) -> None:
    """fi_env_render on device pointers."""
    check(lib().fi_env_render(state_ptr, planes_ptr, n, stream), "fi_env_render")


# ---------------------------------------------------------------------- the rule on the host
def philox4(seed: int, counters, stream: int) -> np.ndarray:
    """Philox4x32-10 as csrc/fi_common.h runs it: key = seed, counter = (e lo, e hi, stream, 0) for
    every e of ``counters`` (uint64); (n, 4) uint32."""
    e = np.asarray(counters, np.uint64).reshape(-1)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = e & m32, e >> np.uint64(32)
    c2 = np.full(e.shape, stream, np.uint64)
    c3 = np.zeros(e.shape, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m32, n2, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


class CatchReference:
    """The rule of include/fi_env.h in numpy. After construction and after every ``step`` the
    attributes hold what the device handle holds: ``planes`` (N, 84, 84) uint8, ``episode_start``
    (N,) uint8, ``rewards`` and ``discounts`` (N,) float32, the state ``r``, ``c``, ``p`` (int32)
    and ``k`` (uint32), and the totals ``episodes`` and ``return_sum`` (Python ints)."""

    def __init__(self, num_envs: int, gamma: float = 0.99, seed: int = 0):
        self.N, self.gamma, self.seed = num_envs, np.float32(gamma), seed
        self.r = np.zeros(num_envs, np.int32)
        self.k = np.zeros(num_envs, np.uint32)
        self.c = np.zeros(num_envs, np.int32)
        self.p = np.zeros(num_envs, np.int32)
        self._reset(np.arange(num_envs))
        self.episode_start = np.ones(num_envs, np.uint8)
        self.rewards = np.zeros(num_envs, np.float32)
        self.discounts = np.zeros(num_envs, np.float32)
        self.episodes, self.return_sum = 0, 0
        self.planes = self.render()

    def _reset(self, idx) -> None:
        if len(idx) == 0:
            return
        w = philox4(self.seed, self.k[idx].astype(np.uint64) * np.uint64(self.N) + idx.astype(np.uint64), ST_ENV)
        self.c[idx] = (w[:, 0].astype(np.uint64) * np.uint64(CELLS)) >> np.uint64(32)
        self.p[idx] = 1 + ((w[:, 1].astype(np.uint64) * np.uint64(19)) >> np.uint64(32))
        self.r[idx] = 0

    def render(self) -> np.ndarray:
        cy, cx = np.arange(84)[:, None] >> 2, np.arange(84)[None, :] >> 2
        out = np.zeros((self.N, 84, 84), np.uint8)
        for i in range(self.N):
            out[i][(cy == LAST_ROW) & (np.abs(cx - self.p[i]) <= 1)] = 128
            out[i][(cy == self.r[i]) & (cx == self.c[i])] = 255
        return out

    def step(self, actions) -> None:
        a = np.asarray(actions, np.int64).reshape(self.N)
        if (a < 0).any():
            raise ValueError("actions must be >= 0")
        m = a % 3
        self.p = np.clip(self.p + (m == 2) - (m == 1), 1, 19).astype(np.int32)
        self.r = self.r + 1
        end = self.r == LAST_ROW
        hit = np.abs(self.c - self.p) <= 1
        self.rewards = np.where(end, np.where(hit, 1.0, -1.0), 0.0).astype(np.float32)
        self.discounts = np.where(end, np.float32(0), self.gamma).astype(np.float32)
        self.episode_start = end.astype(np.uint8)
        self.episodes += int(end.sum())
        self.return_sum += int(self.rewards[end].sum())
        idx = np.nonzero(end)[0]
        self.k[idx] += 1
        self._reset(idx)
        self.planes = self.render()

    def state(self) -> dict:
        return dict(r=self.r.copy(), c=self.c.copy(), p=self.p.copy(), k=self.k.copy())


def catch_reference(num_envs: int, gamma: float = 0.99, seed: int = 0) -> CatchReference:
    """N host environments in their first state (Reset(i, 0), episode_start = 1)."""
    return CatchReference(num_envs, gamma, seed)
