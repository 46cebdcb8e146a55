"""Host side of actor exploration (include/fi_explore.h): a sampling temperature and one epsilon
per environment, with the distribution the action was really drawn from recorded as mu.

  actor.set_exploration(temperature=1.0, epsilon=epsilon_ladder(actor.N))   # or a scalar epsilon
  out = actor.act_planes(planes, start)        # gains out["behaviour_logits"]: what the record's mu takes
  actor.clear_exploration()                    # back to the plain draw, bit for bit

V-trace needs mu to be the behaviour distribution itself, so the kernel that draws the action also
writes the behaviour logits and a recording handle stores those in place of the policy's; the
learner is unchanged. This module holds the ctypes table of the header, the kernel alone on device
pointers (``sample_behaviour``), Ape-X's ``epsilon_ladder`` and the host form of the rule in fp64
numpy (``behaviour_reference``, the tests' reference). ``Actor.set_exploration / clear_exploration /
exploration`` (actor.py) bind the handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

ST_SAMPLE = 6  # the Philox stream of the action draws (csrc/fi_common.h)
NEAR = 1e-5    # a draw within NEAR * W of a running sum may land one index away in fp32
TAU_MIN, TAU_MAX = 1.0 / 64.0, 64.0

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_explore.h declares
    "fi_explore_set": ([_P, C.c_float, _P], C.c_int),
    "fi_explore_clear": ([_P], C.c_int),
    "fi_explore_get": ([_P, C.POINTER(C.c_float), _P, C.POINTER(C.c_int)], C.c_int),
    "fi_explore_behaviour_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_explore_read_behaviour": ([_P, _P, C.c_size_t], C.c_int),
    "fi_sample_behaviour": ([_P, C.c_int, C.c_int, C.c_float, _P, C.c_uint64, C.c_uint64, _P, _P, _P, _P], C.c_int),
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


def epsilon_ladder(n: int, base: float = 0.4, alpha: float = 7.0) -> np.ndarray:
    """Ape-X's ladder: eps_i = base ** (1 + alpha * i / (n - 1)), i = 0 .. n-1, as fp32; n = 1 gives base."""
    if n < 1:
        raise ValueError(f"epsilon_ladder: n must be >= 1, not {n}")
    i = np.arange(n, dtype=np.float64)
    frac = i / (n - 1) if n > 1 else np.zeros(1)
    return (float(base) ** (1.0 + float(alpha) * frac)).astype(np.float32)


def uniforms(seed: int, draw: int, n: int) -> np.ndarray:
    """u_i of the act call with index ``draw``: (x >> 8) * 2^-24, x the first word of
    philox4(seed, draw * n + i, ST_SAMPLE); fp64, exact."""
    from .env import philox4
    ctr = (np.uint64(draw) * np.uint64(n) + np.arange(n, dtype=np.uint64))
    x = philox4(seed, ctr, ST_SAMPLE)[:, 0]
    return (x >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def behaviour_reference(logits, temperature, epsilon, seed: int, draw: int):
    """The rule of fi_explore.h in fp64 on the fp32 inputs: ``(actions, near, mu)``. logits (N, A)
    finite; temperature a scalar; epsilon None, a scalar or N values. ``near`` flags the rows whose
    threshold u W lies within NEAR * W of a running sum: there the fp32 kernel may land one index
    away. mu (N, A) fp64: log(w / W), by the formula of the row's c_i."""
    l32 = np.asarray(logits, np.float32)
    N, A = l32.shape
    tau = float(np.float32(temperature))
    eps = np.zeros(N, np.float32) if epsilon is None else np.broadcast_to(np.asarray(epsilon, np.float32), (N,))
    e = eps.astype(np.float64)[:, None]
    l = l32.astype(np.float64)
    z = (l - l.max(1, keepdims=True)) / tau
    p = np.exp(z)
    Z = p.sum(1, keepdims=True)
    w = (1.0 - e) * p + e * Z / A
    c = np.cumsum(w, 1)
    W = c[:, -1:]
    thr = uniforms(seed, draw, N)[:, None] * W
    over = c > thr
    actions = np.where(over.any(1), over.argmax(1), A - 1).astype(np.int32)
    near = (np.abs(thr - c) <= NEAR * W).any(1)
    # the header's branch: c_i = (eps_i Z) / A as fp32 sees it (0 only for an eps_i below 2^-126)
    floor = (e * Z / A).astype(np.float32) > 0
    with np.errstate(divide="ignore"):
        mu = np.where(floor, np.log(w) - np.log(W), z - np.log(Z))
    return actions, near, mu


def sample_behaviour(logits_ptr: int, n: int, a: int, temperature: float, epsilon_ptr, seed: int, draw: int,
                     actions_ptr: int, mu_ptr: int, nonfinite_ptr=None, stream=None) -> None:
    """fi_sample_behaviour on device pointers (epsilon_ptr None: all 0)."""
    check(lib().fi_sample_behaviour(logits_ptr, n, a, temperature, epsilon_ptr, seed, draw, actions_ptr, mu_ptr,
                                    nonfinite_ptr, stream), "fi_sample_behaviour")
