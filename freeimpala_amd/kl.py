"""Host side of the learner's adaptive KL penalty (include/fi_kl.h): c KL(q || pi) on a reference policy q of
the very batch -- the behaviour logits mu, or the target network's logits -- with a coefficient that adapts to a
KL target on the device (PPO's second form, Schulman et al. 2017, section 4; APPO's use_kl_loss).

  learner.set_objective("surrogate", clip=0.2); learner.enable_target(period=4)
  learner.enable_kl_penalty("target", coeff=1.0, kl_target=0.01)
  learner.step_ring(ring, n_fresh=...); learner.kl_state()   # dict: coeff, mean_kl, updates, raised, lowered, ...
  learner.disable_kl_penalty()                               # the step without the penalty again, bit for bit

This module holds the ctypes table of the header, its two structures, the kernels alone on device pointers
(``kl_penalty_dev``, ``kl_finalize_dev``) and the rule in fp64 numpy (``kl_reference``, ``adapt_reference``: the
tests' references, and ``near_threshold``: whether a mean KL lies where fp32 rows may decide the adaptation the
other way)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import check

REF_BEHAVIOUR, REF_TARGET = 0, 1  # FI_KL_REF_*
REFERENCES = {"behaviour": REF_BEHAVIOUR, "target": REF_TARGET}
COEFF, KL_TARGET, BAND, FACTOR = 1.0, 0.01, 1.5, 2.0  # FI_KL_COEFF, FI_KL_TARGET, FI_KL_BAND, FI_KL_FACTOR
COEFF_MIN, COEFF_MAX = 2.0 ** -20, 2.0 ** 20          # FI_KL_COEFF_MIN, FI_KL_COEFF_MAX
STATE_BYTES = 48  # the device block: double coeff, mean_kl, kl_sum; uint64 rows, updates; uint32 raised, lowered
NEAR = 1e-3       # near_threshold's relative distance


class KlParams(C.Structure):
    _fields_ = [("reference", C.c_uint32), ("adapt", C.c_uint32), ("coeff", C.c_float), ("kl_target", C.c_float),
                ("band", C.c_float), ("factor", C.c_float), ("coeff_min", C.c_float), ("coeff_max", C.c_float)]

    def as_dict(self) -> dict:
        return dict(reference={v: k for k, v in REFERENCES.items()}.get(int(self.reference), int(self.reference)),
                    adapt=bool(self.adapt), kl_target=float(self.kl_target), band=float(self.band),
                    factor=float(self.factor), coeff_min=float(self.coeff_min), coeff_max=float(self.coeff_max))


class KlStats(C.Structure):
    _fields_ = [("coeff", C.c_double), ("mean_kl", C.c_double), ("kl_sum", C.c_double), ("rows", C.c_uint64),
                ("updates", C.c_uint64), ("raised", C.c_uint32), ("lowered", C.c_uint32)]

    def as_dict(self) -> dict:
        return dict(coeff=float(self.coeff), mean_kl=float(self.mean_kl), kl_sum=float(self.kl_sum), rows=int(self.rows),
                    updates=int(self.updates), raised=int(self.raised), lowered=int(self.lowered))


_P = C.c_void_p
_I = C.c_int
SIGNATURES = {  # every symbol include/fi_kl.h declares
    "fi_kl_enable": ([_P, C.POINTER(KlParams)], C.c_int),
    "fi_kl_disable": ([_P], C.c_int),
    "fi_kl_set_coeff": ([_P, C.c_double], C.c_int),
    "fi_kl_get_state": ([_P, C.POINTER(KlParams), C.POINTER(KlStats), C.POINTER(C.c_uint32)], C.c_int),
    "fi_kl_state_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_kl_workspace_bytes": ([_I, _I, _I], C.c_size_t),
    "fi_kl_penalty_fp32": ([_I, _I, _I, _P, _P, _P, _P, _P, C.c_size_t, _P], C.c_int),
    "fi_kl_finalize": ([_I, _I, _I, C.POINTER(KlParams), _P, _P, C.c_size_t, _P, _P], C.c_int),
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


def params(reference="behaviour", adapt: bool = True, coeff: float = COEFF, kl_target: float = KL_TARGET, band: float = BAND,
           factor: float = FACTOR, coeff_min: float = COEFF_MIN, coeff_max: float = COEFF_MAX) -> KlParams:
    """fi_kl_params; reference: "behaviour", "target" or the number."""
    ref = REFERENCES[reference] if isinstance(reference, str) else int(reference)
    return KlParams(ref, int(adapt), coeff, kl_target, band, factor, coeff_min, coeff_max)


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def workspace_bytes(T: int, B: int, A: int) -> int:
    """fi_kl_workspace_bytes (needs no device); 0 for a refused shape."""
    return int(lib().fi_kl_workspace_bytes(T, B, A))


def kl_penalty_dev(T: int, B: int, A: int, pi: int, q: int, dlogits: int, state: int, ws: int, ws_bytes: int,
                   stream=None) -> None:
    """fi_kl_penalty_fp32 on device pointers: dlogits += coeff (softmax(pi) - softmax(q)), the partials into ws."""
    check(lib().fi_kl_penalty_fp32(T, B, A, pi, q, dlogits, state, ws, ws_bytes, stream), "fi_kl_penalty_fp32")


def kl_finalize_dev(T: int, B: int, A: int, prm: KlParams, state: int, ws: int, ws_bytes: int, skip: int | None = None,
                    stream=None) -> None:
    """fi_kl_finalize on device pointers; skip: two device ints (the optimiser's flag words) or None."""
    check(lib().fi_kl_finalize(T, B, A, C.byref(prm) if prm is not None else None, state, ws, ws_bytes, skip, stream),
          "fi_kl_finalize")


def unpack_state(raw) -> dict:
    """The 48 bytes of the block as a dict."""
    raw = np.ascontiguousarray(raw, np.uint8)
    f, n, c = raw[:24].view(np.float64), raw[24:40].view(np.uint64), raw[40:48].view(np.uint32)
    return dict(coeff=float(f[0]), mean_kl=float(f[1]), kl_sum=float(f[2]), rows=int(n[0]), updates=int(n[1]),
                raised=int(c[0]), lowered=int(c[1]))


def pack_state(coeff: float = COEFF, mean_kl: float = 0.0, kl_sum: float = 0.0, rows: int = 0, updates: int = 0,
               raised: int = 0, lowered: int = 0) -> np.ndarray:
    """The block's 48 bytes, what a stand-alone launch is given."""
    return np.frombuffer(np.array([coeff, mean_kl, kl_sum], np.float64).tobytes() + np.array([rows, updates], np.uint64).tobytes() +
                         np.array([raised, lowered], np.uint32).tobytes(), np.uint8).copy()


# ------------------------------------------------------------------ the rule on the host, in fp64
def _log_softmax(z):
    m = z.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = z - m
        return d - np.log(np.exp(d).sum(-1, keepdims=True))


def kl_reference(pi, q, dlogits, coeff: float) -> dict:
    """Rule 1 of include/fi_kl.h in fp64 on the fp32 inputs. pi, q, dlogits (T, B, A); coeff: the block's value,
    used as the kernel uses it, rounded to a float. Returns dlogits (+ c (softmax(pi) - softmax(q))), kl per row
    (T, B), kl_sum, mean_kl and rows."""
    z = np.asarray(pi, np.float32).astype(np.float64)
    zq = np.asarray(q, np.float32).astype(np.float64)
    T, B, _ = z.shape
    c = float(np.float32(coeff))
    with np.errstate(all="ignore"):
        lp, lq = _log_softmax(z), _log_softmax(zq)
        p, pq = np.exp(lp), np.exp(lq)
        kl = (pq * (lq - lp)).sum(-1)
    out = np.asarray(dlogits, np.float64) + c * (p - pq)  # a float32 tensor, or another reference's doubles
    s = float(kl.sum())
    return dict(dlogits=out, kl=kl, kl_sum=s, mean_kl=s / (T * B), rows=T * B)


def _prm(p) -> dict:
    if isinstance(p, dict):
        return p
    return dict(adapt=bool(p.adapt), **{k: float(getattr(p, k)) for k in ("kl_target", "band", "factor", "coeff_min",
                                                                         "coeff_max")})


def adapt_reference(state: dict, mean_kl: float, params, skipped: bool = False, rows: int | None = None,
                    kl_sum: float | None = None) -> dict:
    """Rule 2 on a block (a dict as unpack_state's): the block behind a finalize whose partials averaged to mean_kl.
    params: a KlParams or a dict with adapt, kl_target, band, factor, coeff_min, coeff_max (floats as the structure
    holds them). rows, kl_sum: written when given. Python floats are doubles: the arithmetic is the kernel's."""
    p = _prm(params)
    s = dict(state)
    s["mean_kl"] = float(mean_kl)
    if rows is not None:
        s["rows"] = int(rows)
    if kl_sum is not None:
        s["kl_sum"] = float(kl_sum)
    if skipped:
        return s
    s["updates"] += 1
    if not p["adapt"] or not math.isfinite(mean_kl):
        return s
    if mean_kl > p["band"] * p["kl_target"]:
        s["coeff"] = min(s["coeff"] * p["factor"], p["coeff_max"])
        s["raised"] += 1
    elif mean_kl < p["kl_target"] / p["band"]:
        s["coeff"] = max(s["coeff"] / p["factor"], p["coeff_min"])
        s["lowered"] += 1
    return s


def near_threshold(mean_kl: float, params) -> bool:
    """True when mean_kl lies within a relative 1e-3 of band * kl_target or of kl_target / band: there a device mean
    inside the tests' bar of the reference's may take the other branch."""
    p = _prm(params)
    return any(abs(mean_kl / th - 1.0) <= NEAR for th in (p["band"] * p["kl_target"], p["kl_target"] / p["band"]))
