"""Host side of per-column loss weights and of prioritised replay's two exponents
(include/fi_weights.h).

  learner.set_column_weights(w)                      # (B,) finite, >= 0: the loss becomes sum_b w_b L_b
  learner.set_column_weights(None)                   # cleared: the unweighted step, bit for bit
  ring.enable_priorities(eta=0.9, init_priority=1.0)
  ring.set_priority_exponents(alpha=0.6, beta=0.4)   # the table holds p^alpha; steps weigh by (n q / Q)^-beta
  learner.step_ring(ring, n_fresh=B // 2, prioritized=True)
  ring.last_weights(B)                               # the step's importance weights, the largest exactly 1

This module holds the ctypes table of the header, the standalone kernels on device pointers and the
host form of the rule in fp64 (the tests' reference): ``is_weights`` and ``td_priorities_alpha``.
``DeviceLearner.set_column_weights / column_weights`` (learner.py) and
``EntryRing.set_priority_exponents / priority_exponents / last_weights`` (ring.py) delegate here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, prio
from ._abi import check


class ExponentsState(C.Structure):
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("weights_valid", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        return dict(alpha=float(self.alpha), beta=float(self.beta), weights_valid=bool(self.weights_valid))


_P = C.c_void_p
_U64 = C.c_uint64
SIGNATURES = {  # every symbol include/fi_weights.h declares
    "fi_learner_set_column_weights": ([_P, _P, C.c_int32], C.c_int),
    "fi_learner_clear_column_weights": ([_P], C.c_int),
    "fi_learner_column_weights": ([_P, _P, C.c_int32], C.c_int),
    "fi_prio_set_exponents": ([_P, C.c_float, C.c_float], C.c_int),
    "fi_prio_exponents": ([_P, C.POINTER(ExponentsState)], C.c_int),
    "fi_prio_last_weights": ([_P, C.c_int32, _P], C.c_int),
    "fi_weights_scale_columns": ([_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P], C.c_int),
    "fi_prio_from_td_alpha": ([_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P], C.c_int),
    "fi_prio_is_weights": ([_P, C.c_int32, C.c_int32, _P, C.c_int64, _U64, _U64, _P, C.c_float, _P, _P], C.c_int),
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


# ------------------------------------------------------------------ the rule on the host
def is_weights(q_cols, n_fresh: int, n_valid: int, Q: int, beta: float) -> np.ndarray:
    """(B,) float64: the importance weights of a prioritised step from q_cols, the table value of the
    entry every column names (the first n_fresh, the fresh columns, are not read), the window's
    n_valid and total Q. u = 1 for a fresh column and ((q * n_valid / Q) as fp32) ** -beta for a
    replayed one, w = u / max u. beta is taken as the fp32 number the ring holds."""
    q = np.asarray(q_cols).astype(np.float64)
    if not 0 <= n_fresh <= q.size:
        raise ValueError(f"n_fresh {n_fresh} outside 0 .. {q.size}")
    beta = float(np.float32(beta))
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta {beta} outside [0, 1]")
    u = np.ones(q.size, np.float64)
    if n_fresh < q.size:
        if n_valid < 1 or Q < 1 or q[n_fresh:].min() < 1:
            raise ValueError("replayed columns need n_valid, Q and every priority >= 1")
        ratio = q[n_fresh:] * float(n_valid) / float(Q)  # the product is below 2^51: one rounding
        u[n_fresh:] = ratio.astype(np.float32).astype(np.float64) ** -beta
    return u / u.max()


def td_priorities_alpha(vs, values, eta: float, alpha: float):
    """(B,) int64: ``prio.td_priorities`` with the exponent alpha on the priority, in fp64: Q_MAX for
    a NaN column, otherwise quantise(p) for alpha == 1 and quantise(p ** alpha) for any other alpha.
    alpha is taken as the fp32 number the ring holds."""
    alpha = float(np.float32(alpha))
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha {alpha} outside [0, 1]")
    if alpha == 1.0:
        return prio.td_priorities(vs, values, eta)
    p = prio.td_magnitudes(vs, values, eta)
    nan = np.isnan(p)
    with np.errstate(invalid="ignore", over="ignore"):
        q = prio.quantize_priority(np.where(nan, 0.0, p) ** alpha)
    return np.where(nan, prio.Q_MAX, q).astype(np.int64)


# ------------------------------------------------------------------ what DeviceLearner delegates here
def set_column_weights(learner, w) -> None:
    if w is None:
        check(lib().fi_learner_clear_column_weights(learner._h), "fi_learner_clear_column_weights")
        return
    a = np.ascontiguousarray(np.asarray(w, np.float32).ravel())
    check(lib().fi_learner_set_column_weights(learner._h, a.ctypes.data, a.size), "fi_learner_set_column_weights")


def column_weights(learner) -> np.ndarray:
    out = np.empty(learner.B, np.float32)
    check(lib().fi_learner_column_weights(learner._h, out.ctypes.data, out.size), "fi_learner_column_weights")
    return out


# ------------------------------------------------------------------ what EntryRing delegates here
def set_exponents(ring, alpha: float = 1.0, beta: float = 0.0) -> None:
    check(lib().fi_prio_set_exponents(ring._h, alpha, beta), "fi_prio_set_exponents")


def exponents(ring) -> dict:
    st = ExponentsState()
    check(lib().fi_prio_exponents(ring._h, C.byref(st)), "fi_prio_exponents")
    return st.as_dict()


def last_weights(ring, B: int) -> np.ndarray:
    out = np.empty(max(B, 1), np.float32)
    check(lib().fi_prio_last_weights(ring._h, B, out.ctypes.data), "fi_prio_last_weights")
    return out[:B]


# ------------------------------------------------------------------ standalone kernels on device pointers
def scale_columns(dlogits_ptr: int, dvalue_ptr: int, w_ptr: int, T: int, B: int, A: int, stream=None) -> None:
    """fi_weights_scale_columns."""
    check(lib().fi_weights_scale_columns(dlogits_ptr, dvalue_ptr, w_ptr, T, B, A, stream), "fi_weights_scale_columns")


def from_td_alpha(vs_ptr: int, values_ptr: int, T: int, B: int, eta: float, alpha: float, q_out_ptr: int,
                  stream=None) -> None:
    """fi_prio_from_td_alpha."""
    check(lib().fi_prio_from_td_alpha(vs_ptr, values_ptr, T, B, eta, alpha, q_out_ptr, stream), "fi_prio_from_td_alpha")


def is_weights_dev(entries_ptr: int, B: int, n_fresh: int, table_ptr, capacity: int, lo: int, n_valid: int, chunk_ws_ptr,
                   beta: float, w_out_ptr: int, stream=None) -> None:
    """fi_prio_is_weights."""
    check(lib().fi_prio_is_weights(entries_ptr, B, n_fresh, table_ptr, capacity, lo, n_valid, chunk_ws_ptr, beta,
                                   w_out_ptr, stream), "fi_prio_is_weights")
