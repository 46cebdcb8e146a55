"""Host side of the learner's upgoing policy update, UPGO (include/fi_upgo.h): AlphaStar's second policy-gradient
term, whose return follows the behaviour trajectory's rewards for as long as they beat the value estimate (Vinyals
et al. 2019, Methods).

  learner.enable_upgo(coeff=1.0, rho_bar=1.0)        # under any objective; the term only adds onto dlogits
  learner.step_ring(ring, n_fresh=...); learner.upgo_state()   # dict: loss_u, sum_au, rows, links_up, rows_positive
  learner.disable_upgo()                             # the step without the term again, bit for bit

This module holds the ctypes table of the header, its two structures, the kernels alone on device pointers
(``returns_dev``, ``term_dev``) and the rule in fp64 numpy (``upgo_reference``: the tests' yardstick)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

COEFF, RHO_BAR = 1.0, 1.0  # FI_UPGO_COEFF, FI_UPGO_RHO_BAR
STATE_BYTES = 40           # the device block: double loss_u, sum_au; uint64 rows, links_up, rows_positive


class UpgoParams(C.Structure):
    _fields_ = [("coeff", C.c_float), ("rho_bar", C.c_float)]

    def as_dict(self) -> dict:
        return dict(coeff=float(self.coeff), rho_bar=float(self.rho_bar))


class UpgoStats(C.Structure):
    _fields_ = [("loss_u", C.c_double), ("sum_au", C.c_double), ("rows", C.c_uint64), ("links_up", C.c_uint64),
                ("rows_positive", C.c_uint64)]

    def as_dict(self) -> dict:
        return dict(loss_u=float(self.loss_u), sum_au=float(self.sum_au), rows=int(self.rows), links_up=int(self.links_up),
                    rows_positive=int(self.rows_positive))


_P = C.c_void_p
_I = C.c_int
SIGNATURES = {  # every symbol include/fi_upgo.h declares
    "fi_upgo_enable": ([_P, C.POINTER(UpgoParams)], C.c_int),
    "fi_upgo_disable": ([_P], C.c_int),
    "fi_upgo_get_state": ([_P, C.POINTER(UpgoParams), C.POINTER(UpgoStats), C.POINTER(C.c_uint32)], C.c_int),
    "fi_upgo_state_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_upgo_workspace_bytes": ([_I, _I, _I], C.c_size_t),
    "fi_upgo_returns_fp32": ([_I, _I] + [_P] * 7, C.c_int),
    "fi_upgo_term_fp32": ([_I, _I, _I] + [_P] * 6 + [C.POINTER(UpgoParams), _P, _P, _P, C.c_size_t, _P], C.c_int),
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


def params(coeff: float = COEFF, rho_bar: float = RHO_BAR) -> UpgoParams:
    return UpgoParams(coeff, rho_bar)


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def workspace_bytes(T: int, B: int, A: int) -> int:
    """fi_upgo_workspace_bytes (needs no device); 0 for a refused shape."""
    return int(lib().fi_upgo_workspace_bytes(T, B, A))


def returns_dev(T: int, B: int, rewards: int, discounts: int, values: int, au: int, g: int | None = None,
                up: int | None = None, stream=None) -> None:
    """fi_upgo_returns_fp32 on device pointers: AU (T, B), and G (floats) and up (bytes) where asked for."""
    check(lib().fi_upgo_returns_fp32(T, B, rewards, discounts, values, au, g, up, stream), "fi_upgo_returns_fp32")


def term_dev(T: int, B: int, A: int, logits: int, mu: int, actions: int, rewards: int, discounts: int, values: int,
             prm: UpgoParams, dlogits: int, stats: int, ws: int, ws_bytes: int, stream=None) -> None:
    """fi_upgo_term_fp32 on device pointers: dlogits += coeff rho AU (pi - [a]); the block into stats, AU into ws."""
    check(lib().fi_upgo_term_fp32(T, B, A, logits, mu, actions, rewards, discounts, values,
                                  C.byref(prm) if prm is not None else None, dlogits, stats, ws, ws_bytes, stream),
          "fi_upgo_term_fp32")


def unpack_state(raw) -> dict:
    """The 40 bytes of the block as a dict."""
    raw = np.ascontiguousarray(raw, np.uint8)
    f, n = raw[:16].view(np.float64), raw[16:40].view(np.uint64)
    return dict(loss_u=float(f[0]), sum_au=float(f[1]), rows=int(n[0]), links_up=int(n[1]), rows_positive=int(n[2]))


# ------------------------------------------------------------------ the rule on the host, in fp64
def upgo_returns(rewards, discounts, values, dtype=np.float64) -> dict:
    """Rule 1 of include/fi_upgo.h as a plain loop over t in ``dtype`` on the fp32 inputs: G, AU (T, B), up (T, B)
    bool and ``margin``, the least |r_{t+1} + g_{t+1} V_{t+2} - V_{t+1}| (inf at T = 1): where it is small another
    precision may decide a link the other way."""
    r, g, v = (np.asarray(x, np.float32).astype(dtype) for x in (rewards, discounts, values))
    T, B = r.shape
    with np.errstate(all="ignore"):
        gap = r[1:] + g[1:] * v[2:] - v[1:T]
        up = np.zeros((T, B), bool)
        up[:T - 1] = gap >= 0  # NaN: not up
        G = np.zeros((T, B), dtype)
        for t in range(T - 1, -1, -1):
            G[t] = r[t] + g[t] * (np.where(up[t], G[t + 1], v[t + 1]) if t < T - 1 else v[t + 1])
        finite = np.abs(gap[np.isfinite(gap)])
    return dict(G=G, AU=G - v[:T], up=up, margin=float(finite.min()) if finite.size else float("inf"))


def upgo_reference(logits, mu, actions, rewards, discounts, values, coeff: float = COEFF, rho_bar: float = RHO_BAR) -> dict:
    """Rules 1 to 3 in fp64 on the fp32 inputs; coeff and rho_bar as the kernel holds them, rounded to floats.
    Returns upgo_returns' G, AU, up and margin, ``dlogits`` (T, B, A: the increment coeff rho AU (pi - [a])), rho and
    the block's loss_u, sum_au, rows, links_up, rows_positive."""
    z, zm = (np.asarray(x, np.float32).astype(np.float64) for x in (logits, mu))
    T, B, A = z.shape
    out = upgo_returns(rewards, discounts, values)
    a = np.clip(np.asarray(actions, np.int64), 0, A - 1)[..., None]
    c, rb = float(np.float32(coeff)), float(np.float32(rho_bar))

    def log_softmax(x):
        d = x - x.max(-1, keepdims=True)
        return d - np.log(np.exp(d).sum(-1, keepdims=True))

    with np.errstate(all="ignore"):
        lp = log_softmax(z)
        lpa = np.take_along_axis(lp, a, -1)[..., 0]
        rho = np.minimum(rb, np.exp(lpa - np.take_along_axis(log_softmax(zm), a, -1)[..., 0]))
        w = rho * out["AU"]
        out.update(dlogits=c * w[..., None] * (np.exp(lp) - (np.arange(A) == a)), rho=rho, loss_u=float(-(w * lpa).sum()),
                   sum_au=float(out["AU"].sum()), rows=T * B, links_up=int(out["up"].sum()),
                   rows_positive=int((out["AU"] > 0).sum()))
    return out
