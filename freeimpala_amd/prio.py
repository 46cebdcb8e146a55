"""Host side of prioritised replay for the device entry ring (include/fi_prio.h).

  ring = EntryRing(learner.entry_bytes, capacity=4 * learner.B, seed=1)
  ring.enable_priorities(eta=0.9, init_priority=1.0)
  ...
  learner.step_ring(ring, n_fresh=B // 2, prioritized=True)   # replayed columns by priority
  ring.priorities(first_entry, n)                             # u32, by entry index over [lo, tail)

This module holds the ctypes table of the header, the standalone kernels on device pointers and
the host form of the rule (the tests' reference): ``quantize_priority``, ``td_priorities`` and
``prio_batch_entries``. ``EntryRing.enable_priorities / priorities / set_priorities`` (ring.py) and
``DeviceLearner.step_ring(prioritized=True)`` (learner.py) delegate here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import StepStats, check

ST_PRIO = 8  # the Philox counter stream of the prioritised draws (csrc/fi_common.h)
Q_MAX = 2 ** 31 - 1
MAX_CAPACITY = 2 ** 20
CHUNK_WS_BYTES = 8 * 1024  # the chunk sums of one draw: 1024 u64


class PrioState(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("eta", C.c_float), ("q_init", C.c_uint32), ("reserved", C.c_uint32),
                ("prio_hi", C.c_uint64), ("table_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        return dict(enabled=bool(self.enabled), eta=float(self.eta), q_init=int(self.q_init), prio_hi=int(self.prio_hi),
                    table_bytes=int(self.table_bytes))


_P = C.c_void_p
_U64 = C.c_uint64
SIGNATURES = {  # every symbol include/fi_prio.h declares
    "fi_prio_enable": ([_P, C.c_float, C.c_float], C.c_int),
    "fi_prio_info": ([_P, C.POINTER(PrioState)], C.c_int),
    "fi_prio_read": ([_P, _U64, C.c_int32, _P], C.c_int),
    "fi_prio_set": ([_P, _U64, C.c_int32, _P], C.c_int),
    "fi_learner_step_ring_prioritized": ([_P, _P, C.c_int32, C.POINTER(StepStats)], C.c_int),
    "fi_learner_step_ring_prioritized_async": ([_P, _P, C.c_int32], C.c_int),
    "fi_prio_from_td": ([_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P], C.c_int),
    "fi_prio_scatter": ([_P, C.c_int64, _P, _P, C.c_int32, _P], C.c_int),
    "fi_prio_fill_columns": ([_P, _P, _P, _P, C.c_size_t, C.c_int64, C.c_int32, C.c_int32] + [_U64] * 3 + [_P, _P] +
                             [_U64] * 2 + [_P], C.c_int),
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
def quantize_priority(p):
    """u32 priority of p >= 0 (scalar or array): Q_MAX for NaN, Inf and p >= 32768, otherwise
    max(1, rint(p * 65536)) with ties to even."""
    a = np.asarray(p, np.float64)
    big = ~(a < 32768.0)  # NaN, Inf, >= 32768
    q = np.maximum(1.0, np.rint(np.where(big, 0.0, a) * 65536.0))
    q = np.where(big, float(Q_MAX), q).astype(np.int64)
    return int(q) if q.ndim == 0 else q


def td_magnitudes(vs, values, eta: float) -> np.ndarray:
    """(B,) float64: p = eta * max_t d + (1 - eta) * mean_t d with d = |vs - values|, from vs (T, B)
    and values (>= T rows, B) as the device holds them, computed in fp64; NaN for a column with a NaN
    difference. eta is taken as the fp32 number the ring holds."""
    vs = np.asarray(vs, np.float32).astype(np.float64)
    T = vs.shape[0]
    v = np.asarray(values, np.float32).astype(np.float64)[:T]
    eta = float(np.float32(eta))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(vs - v)
        nan = np.isnan(d).any(axis=0)
        p = eta * np.where(np.isnan(d), 0.0, d).max(axis=0) + (1.0 - eta) * d.sum(axis=0) / T
        return np.where(nan, np.nan, p)


def td_priorities(vs, values, eta: float):
    """(B,) int64: the quantised priority of every column from vs (T, B) and values (>= T rows, B)
    as the device holds them, computed in fp64 (td_magnitudes)."""
    return quantize_priority(td_magnitudes(vs, values, eta))


def prio_batch_entries(philox4, seed: int, draw: int, B: int, n_fresh: int, head: int, tail: int, capacity: int,
                       q_window) -> list[int]:
    """The prioritised batch rule on the host: the entry index of every column of a step with
    n_fresh fresh columns, from the ring's numbers before the call and q_window, the priorities of
    the entries lo .. tail - 1 (lo = max(0, head - capacity)). Column c < n_fresh is entry
    tail + c; column c >= n_fresh takes lo + min{ j : q_0 + ... + q_j > r } with
    r = (x * Q) >> 64, Q the window's total and x = w0 * 2^32 + w1 from
    philox4(seed, draw * B + c, 8). Every sum is exact: q <= 2^31 - 1 and capacity <= 2^20."""
    if not 0 <= n_fresh <= B:
        raise ValueError(f"n_fresh {n_fresh} outside 0 .. {B}")
    if n_fresh > head - tail:
        raise ValueError(f"{head - tail} entries unread, n_fresh = {n_fresh}")
    if capacity > MAX_CAPACITY:
        raise ValueError(f"capacity {capacity} above 2^20 = {MAX_CAPACITY}")
    lo = head - capacity if head > capacity else 0
    n_valid = tail - lo
    out = [tail + c for c in range(n_fresh)]
    if n_fresh == B:
        return out
    if n_valid <= 0:
        raise ValueError("nothing to replay")
    q = np.asarray(q_window).astype(np.uint64)
    if q.shape != (n_valid,):
        raise ValueError(f"q_window holds {q.shape} priorities, the window [{lo}, {tail}) {n_valid}")
    if int(q.min()) < 1 or int(q.max()) > Q_MAX:
        raise ValueError("priorities outside 1 .. 2^31 - 1")
    cum = np.cumsum(q, dtype=np.uint64)  # below 2^51: exact
    total = int(cum[-1])
    for c in range(n_fresh, B):
        w = philox4(seed, (draw * B + c) & (2 ** 64 - 1), ST_PRIO)
        x = (int(w[0]) << 32) | int(w[1])
        r = (x * total) >> 64
        out.append(lo + int(np.searchsorted(cum, np.uint64(r), side="right")))  # the first j with cum[j] > r
    return out


# ------------------------------------------------------------------ what EntryRing delegates here
def enable(ring, eta: float = 0.9, init_priority: float = 1.0) -> None:
    check(lib().fi_prio_enable(ring._h, eta, init_priority), "fi_prio_enable")


def info(ring) -> dict:
    st = PrioState()
    check(lib().fi_prio_info(ring._h, C.byref(st)), "fi_prio_info")
    return st.as_dict()


def read(ring, first_entry: int, n: int) -> np.ndarray:
    out = np.empty(max(n, 1), np.uint32)
    check(lib().fi_prio_read(ring._h, first_entry, n, out.ctypes.data), "fi_prio_read")
    return out[:n]


def write(ring, first_entry: int, q) -> None:
    a = np.asarray(q, np.int64)
    if a.size and (a.min() < 0 or a.max() > 2 ** 32 - 1):
        raise ValueError("priorities are u32")
    a = np.ascontiguousarray(a.astype(np.uint32))
    check(lib().fi_prio_set(ring._h, first_entry, a.size, a.ctypes.data), "fi_prio_set")


# ------------------------------------------------------------------ standalone kernels on device pointers
def from_td(vs_ptr: int, values_ptr: int, T: int, B: int, eta: float, q_out_ptr: int, stream=None) -> None:
    """fi_prio_from_td."""
    check(lib().fi_prio_from_td(vs_ptr, values_ptr, T, B, eta, q_out_ptr, stream), "fi_prio_from_td")


def scatter(table_ptr: int, capacity: int, entries_ptr: int, q_cols_ptr: int, B: int, stream=None) -> None:
    """fi_prio_scatter."""
    check(lib().fi_prio_scatter(table_ptr, capacity, entries_ptr, q_cols_ptr, B, stream), "fi_prio_scatter")


def fill_columns(cols_ptr: int, entries_ptr, versions_ptr, base_ptr: int, entry_bytes: int, capacity: int, B: int,
                 n_fresh: int, tail: int, lo: int, n_valid: int, table_ptr, chunk_ws_ptr, seed: int, draw: int,
                 stream=None) -> None:
    """fi_prio_fill_columns."""
    check(lib().fi_prio_fill_columns(cols_ptr, entries_ptr, versions_ptr, base_ptr, entry_bytes, capacity, B, n_fresh,
                                     tail, lo, n_valid, table_ptr, chunk_ws_ptr, seed, draw, stream),
          "fi_prio_fill_columns")
