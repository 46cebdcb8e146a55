"""Host side of the training recipe on a learner handle (include/fi_train.h): RMSProp, a learning
rate that can change between steps, and reward clipping.

  learner = DeviceLearner("atari", ..., optimizer="rmsprop", lr=4.8e-4)   # set_rmsprop() with monobeast's numbers
  learner.set_rmsprop(decay=0.99, momentum=0.0, eps=0.01)                # or chosen by hand, before the first step
  learner.set_lr_schedule(lr_end=0.0, n_steps=2000)                      # update s runs at lr_at(s, lr, 0, 2000)
  learner.set_lr(3e-4)                                                   # a caller's own schedule, between steps
  learner.set_reward_clip(1.0)                                           # rewards clamped to [-1, 1] before V-trace
  learner.train_state()                                                  # dict: optimizer, lr_next, next_update, ...

This module holds the ctypes table of the header, the two standalone kernels on device pointers and
the host form of the three rules in fp64 (the tests' reference): ``rmsprop_reference``, ``lr_at`` and
``clip_rewards``. ``DeviceLearner.set_rmsprop / set_lr / set_lr_schedule / clear_lr_schedule /
set_reward_clip / train_state`` (learner.py) bind the rest. The recipe is configuration and not part
of ``save_state``'s blob: a resuming process makes the same calls, then ``load_state``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

FI_TRAIN_OPT_RMSPROP = 2
OPTIMIZERS = {_abi.FI_OPT_ADAM: "adam", _abi.FI_OPT_SGD: "sgd", FI_TRAIN_OPT_RMSPROP: "rmsprop"}


class TrainState(C.Structure):
    _fields_ = [("optimizer", C.c_uint32), ("eps_in_sqrt", C.c_uint32), ("decay", C.c_float), ("momentum", C.c_float),
                ("eps", C.c_float), ("lr_base", C.c_float), ("lr_end", C.c_float), ("lr_next", C.c_float),
                ("reward_clip", C.c_float), ("schedule_on", C.c_uint32), ("lr_steps", C.c_uint64),
                ("next_update", C.c_uint64)]

    def as_dict(self) -> dict:
        return dict(optimizer=OPTIMIZERS.get(int(self.optimizer), int(self.optimizer)), eps_in_sqrt=bool(self.eps_in_sqrt),
                    decay=float(self.decay), momentum=float(self.momentum), eps=float(self.eps), lr_base=float(self.lr_base),
                    lr_end=float(self.lr_end), lr_next=float(self.lr_next), reward_clip=float(self.reward_clip),
                    schedule_on=int(self.schedule_on), lr_steps=int(self.lr_steps), next_update=int(self.next_update))


_P = C.c_void_p
_F = C.c_float
SIGNATURES = {  # every symbol include/fi_train.h declares
    "fi_train_set_rmsprop": ([_P, _F, _F, _F, C.c_int], C.c_int),
    "fi_train_set_lr": ([_P, _F], C.c_int),
    "fi_train_set_lr_schedule": ([_P, _F, C.c_uint64], C.c_int),
    "fi_train_clear_lr_schedule": ([_P], C.c_int),
    "fi_train_set_reward_clip": ([_P, _F], C.c_int),
    "fi_train_get_state": ([_P, C.POINTER(TrainState)], C.c_int),
    "fi_train_rmsprop_update": ([_P, _P, _P, _P, C.c_size_t, _F, _F, _F, _F, C.c_int, _P, _F, _P, _P], C.c_int),
    "fi_train_clip_rewards": ([_P, C.c_size_t, _F, _P], C.c_int),
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


# ------------------------------------------------------------------ the rules on the host, in fp64
def rmsprop_reference(p, g, v, m, lr, decay, momentum, eps, eps_in_sqrt=False, scale=1.0):
    """One RMSProp update in fp64: returns (p, v, m) as new arrays; m is returned as it came (None
    allowed) when momentum == 0. The numbers are taken as given: a caller that compares with the
    fp32 kernel passes them as the fp32 values the kernel holds.
      g' = g scale;  v = decay v + (1 - decay) g'^2;  d = sqrt(v + eps) if eps_in_sqrt else sqrt(v) + eps
      momentum > 0: m = momentum m + g'/d, p = p - lr m;   momentum == 0: p = p - lr g'/d"""
    p, g, v = (np.asarray(x, np.float64) for x in (p, g, v))
    lr, decay, momentum, eps, scale = (float(x) for x in (lr, decay, momentum, eps, scale))
    gs = g * scale
    v = decay * v + (1.0 - decay) * gs * gs
    d = np.sqrt(v + eps) if eps_in_sqrt else np.sqrt(v) + eps
    u = gs / d
    if momentum > 0.0:
        m = momentum * np.asarray(m, np.float64) + u
        return p - lr * m, v, m
    return p - lr * u, v, m


def lr_at(s: int, lr_base: float, lr_end: float, n_steps: int) -> float:
    """The rate of the update numbered s >= 1 under fi_train_set_lr_schedule, as the fp32 number the
    kernel gets: lr_base and lr_end are taken as fp32, the line is evaluated in fp64 and rounded
    once. s = 1 gives lr_base; s > n_steps gives lr_end exactly."""
    if s < 1 or n_steps < 1:
        raise ValueError(f"s {s} and n_steps {n_steps} must be >= 1")
    b, e = float(np.float32(lr_base)), float(np.float32(lr_end))
    k = min(s - 1, n_steps)
    if k == n_steps:
        return e
    return float(np.float32(b + (e - b) * float(k) / float(n_steps)))


def clip_rewards(r, c: float) -> np.ndarray:
    """r clamped to [-c, c] by comparison, in r's dtype: a NaN stays a NaN, -0.0 stays -0.0, +-Inf
    becomes +-c. c is taken as the fp32 number the learner holds."""
    r = np.asarray(r)
    c = np.float32(c)
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"c {c} is not positive and finite")
    out = r.copy()
    with np.errstate(invalid="ignore"):
        out[r > c] = c
        out[r < -c] = -c
    return out


# ------------------------------------------------------------------ standalone kernels on device pointers
def rmsprop_update(p_ptr: int, g_ptr: int, v_ptr: int, m_ptr, n: int, lr: float, decay: float, momentum: float,
                   eps: float, eps_in_sqrt: bool = False, sqnorm_ptr=None, max_norm: float = 0.0, skip_ptr=None,
                   stream=None) -> None:
    """fi_train_rmsprop_update."""
    check(lib().fi_train_rmsprop_update(p_ptr, g_ptr, v_ptr, m_ptr, n, lr, decay, momentum, eps, int(bool(eps_in_sqrt)),
                                        sqnorm_ptr, max_norm, skip_ptr, stream), "fi_train_rmsprop_update")


def clip_rewards_dev(r_ptr: int, n: int, c: float, stream=None) -> None:
    """fi_train_clip_rewards."""
    check(lib().fi_train_clip_rewards(r_ptr, n, c, stream), "fi_train_clip_rewards")
