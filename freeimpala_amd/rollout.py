"""Host side of rollouts recorded on the device (include/fi_rollout.h).

A recording ``Actor`` writes the learner's own entry format into device memory as it acts, and a
``DeviceLearner`` on the same device steps straight from those entries:

  actor.begin_rollout(T)
  for every step:
      out = actor.act_planes(planes, episode_start)   # records the step on the device
      rew, disc = envs.step(out["actions"])
      actor.outcome(rew, disc)                        # 8 bytes per env-step cross PCIe
      if actor.rollout_ready():
          learner.step_rollout(actor)                 # ingest in place, step, release

This module holds the ctypes table of the header and ``split_unrolls``, the host form of the
recording rule (the tests' reference). The methods live on ``Actor`` and ``DeviceLearner``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import StepStats, check

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_rollout.h declares
    "fi_rollout_begin": ([_P, C.c_int32], C.c_int),
    "fi_rollout_outcome": ([_P, _P, _P], C.c_int),
    "fi_rollout_ready": ([_P], C.c_int),
    "fi_rollout_entry_bytes": ([_P], C.c_size_t),
    "fi_rollout_acquire": ([_P, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P)], C.c_int),
    "fi_rollout_release": ([_P, _P], C.c_int),
    "fi_rollout_read": ([_P, _P, C.c_size_t], C.c_int),
    "fi_rollout_end": ([_P], C.c_int),
    "fi_learner_step_entries_dev": ([_P, _P, C.c_size_t, _P, C.POINTER(StepStats)], C.c_int),
    "fi_learner_step_entries_dev_async": ([_P, _P, C.c_size_t, _P], C.c_int),
    "fi_learner_entries_consumed_event": ([_P], _P),
    "fi_learner_staging_bytes": ([_P], C.c_size_t),
    "fi_learner_step_rollout": ([_P, _P, C.POINTER(StepStats)], C.c_int),
    "fi_record_plane_step": ([_P, C.c_size_t, C.c_int32, _P, _P, _P, _P, C.c_uint32, C.c_int, C.c_int, _P], C.c_int),
    "fi_extract_history": ([_P, C.c_size_t, C.c_size_t, _P, C.c_int, _P], C.c_int),
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


def record_plane_step(entries_ptr: int, stride: int, t: int, planes_ptr: int, start_ptr: int, logits_ptr,
                      actions_ptr, flags: int, n: int, a: int, stream=None) -> None:
    """fi_record_plane_step on device pointers (logits_ptr None: the plane and episode_start only)."""
    check(lib().fi_record_plane_step(entries_ptr, stride, t, planes_ptr, start_ptr, logits_ptr, actions_ptr, flags,
                                     n, a, stream), "fi_record_plane_step")


def extract_history(entries_ptr: int, stride: int, history_offset: int, stacks_ptr: int, n: int, stream=None) -> None:
    """fi_extract_history on device pointers."""
    check(lib().fi_extract_history(entries_ptr, stride, history_offset, stacks_ptr, n, stream), "fi_extract_history")


def split_unrolls(planes, start, mu, act, rew, disc, T: int) -> list[tuple]:
    """The recording rule on the host. A run of K*T+1 steps -- planes (K*T+1, B, 84, 84) uint8,
    start (K*T+1, B), and for every step its mu (.., B, A), act, rew, disc (.., B); the last step's
    header values are not used, so these four may hold K*T rows -- becomes K unrolls that overlap
    by one step. Unroll k is ``(planes (T+1,B,84,84), history (3,B,84,84), start (T+1,B), mu (T,B,A),
    act, rew, disc (T,B))``: the arguments of pack_atari_plane_records. Its history is channels
    0..2 of the stack at step k*T, taken from stack_planes over the whole run from zero stacks."""
    from .learner import stack_planes
    planes = np.asarray(planes, np.uint8)
    start = np.asarray(start) != 0
    S, B = planes.shape[:2]
    if T < 1 or S < T + 1 or (S - 1) % T:
        raise ValueError(f"{S} steps are not K*{T}+1")
    K = (S - 1) // T
    for nm, x in (("mu", mu), ("act", act), ("rew", rew), ("disc", disc)):
        if len(x) < K * T:
            raise ValueError(f"{nm}: {len(x)} rows < {K * T}")
    frames = stack_planes(planes, np.zeros((3, B, 84, 84), np.uint8), start)
    out = []
    for k in range(K):
        lo = k * T
        history = np.ascontiguousarray(np.moveaxis(frames[lo, :, :, :, :3], -1, 0))
        out.append((planes[lo:lo + T + 1], history, start[lo:lo + T + 1], np.asarray(mu[lo:lo + T], np.float32),
                    np.asarray(act[lo:lo + T], np.int32), np.asarray(rew[lo:lo + T], np.float32),
                    np.asarray(disc[lo:lo + T], np.float32)))
    return out
