"""Host side of PopArt value normalisation on a learner handle (include/fi_popart.h): the value head
predicts a normalised value n, the statistics mu, sigma of the V-trace targets are tracked on the
device, and each time they move the head's value column is rewritten so that sigma n + mu is preserved.

  learner.enable_popart()                      # the paper's beta = 3e-4, sigma in [1e-4, 1e6]
  learner.step_resident(); learner.popart_state()   # dict: enabled, beta, mu, nu, sigma, updates, ...
  learner.set_popart_state(mu, nu)             # resume: enable_popart, set_popart_state, load_state

This module holds the ctypes table of the header, the stand-alone kernels on device pointers and the
whole rule in fp64 numpy (the tests' reference): ``popart_reference`` and ``preserved_output``. The
statistics are not part of ``save_state``'s blob."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import check

BETA, SIGMA_MIN, SIGMA_MAX = 3e-4, 1e-4, 1e6  # the paper's defaults (FI_POPART_*)
STREAM_GRID_MAX = 1024  # workgroups of 256 lanes of the two streaming kernels, at most (csrc/kernels.h)
STATE_BYTES = 32        # the device block: double mu, nu, sigma; uint64 updates


class PopartState(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("reserved", C.c_uint32), ("beta", C.c_double), ("sigma_min", C.c_double),
                ("sigma_max", C.c_double), ("mu", C.c_double), ("nu", C.c_double), ("sigma", C.c_double),
                ("updates", C.c_uint64)]

    def as_dict(self) -> dict:
        return dict(enabled=bool(self.enabled), beta=float(self.beta), sigma_min=float(self.sigma_min),
                    sigma_max=float(self.sigma_max), mu=float(self.mu), nu=float(self.nu), sigma=float(self.sigma),
                    updates=int(self.updates))


_P = C.c_void_p
_D = C.c_double
SIGNATURES = {  # every symbol include/fi_popart.h declares
    "fi_popart_enable": ([_P, _D, _D, _D], C.c_int),
    "fi_popart_get_state": ([_P, C.POINTER(PopartState)], C.c_int),
    "fi_popart_set_state": ([_P, _D, _D], C.c_int),
    "fi_popart_state_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_popart_plan": ([C.c_size_t], C.c_int),
    "fi_popart_workspace_bytes": ([C.c_size_t], C.c_size_t),
    "fi_popart_denormalize": ([_P, C.c_size_t, _P, _P], C.c_int),
    "fi_popart_scale_grad": ([_P, C.c_size_t, _P, _P], C.c_int),
    "fi_popart_update": ([_P, C.c_size_t, _P, _P, C.c_size_t, C.c_int, _P, _D, _D, _D, _P, _P, C.c_size_t, _P], C.c_int),
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


# ------------------------------------------------------------------ the rule on the host, in fp64
def sigma_of(mu: float, nu: float, sigma_min: float = SIGMA_MIN, sigma_max: float = SIGMA_MAX) -> float:
    """clamp(sqrt(max(nu - mu^2, 0)), sigma_min, sigma_max)."""
    return min(max(math.sqrt(max(nu - mu * mu, 0.0)), sigma_min), sigma_max)


def popart_reference(values_n, vs, w, b, mu, nu, beta=BETA, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, sigma=None):
    """One step's PopArt arithmetic in fp64. values_n: the head's normalised outputs; vs: the step's
    V-trace targets (any shape, all of them counted); w, b: the value column and its bias as the
    optimiser left them; mu, nu: the statistics the step began with (sigma: what they imply, unless
    given). Returns a dict: ``values`` = sigma values_n + mu (unrounded: the kernel's fmaf uses the
    fp32 sigma_f, mu_f), the new ``mu``, ``nu``, ``sigma`` and the rewritten ``w``, ``b`` (fp64, not
    rounded to fp32), and ``updated``: False, with everything handed back unchanged, when a sum is not
    finite. The sums are exact (math.fsum)."""
    values_n = np.asarray(values_n, np.float64)
    x = np.asarray(vs, np.float64).reshape(-1)
    w = np.asarray(w, np.float64)
    b, mu, nu, beta = float(b), float(mu), float(nu), float(beta)
    if sigma is None:
        sigma = sigma_of(mu, nu, sigma_min, sigma_max)
    out = dict(values=sigma * values_n + mu, mu=mu, nu=nu, sigma=sigma, w=w.copy(), b=b, updated=False)
    if x.size == 0 or not np.isfinite(x).all():
        return out
    s1, s2 = math.fsum(x), math.fsum(x * x)
    if not (math.isfinite(s1) and math.isfinite(s2)):
        return out
    n = float(x.size)
    mu2 = (1.0 - beta) * mu + beta * (s1 / n)
    nu2 = (1.0 - beta) * nu + beta * (s2 / n)
    sigma2 = sigma_of(mu2, nu2, sigma_min, sigma_max)
    out.update(mu=mu2, nu=nu2, sigma=sigma2, w=w * sigma / sigma2, b=(sigma * b + (mu - mu2)) / sigma2, updated=True)
    return out


def preserved_output(h, w, b, mu, sigma) -> np.ndarray:
    """The unnormalised value sigma (h . w + b) + mu in fp64, h: (..., H). What a PopArt update leaves
    unchanged: the same number from (w, b, mu, sigma) and from the rewritten (w', b', mu', sigma')."""
    h = np.asarray(h, np.float64)
    return float(sigma) * (h @ np.asarray(w, np.float64) + float(b)) + float(mu)


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def plan(n: int) -> int:
    """fi_popart_plan: workgroups of the moments kernel over n targets (needs no device)."""
    return int(lib().fi_popart_plan(n))


def workspace_bytes(n: int) -> int:
    """fi_popart_workspace_bytes (needs no device)."""
    return int(lib().fi_popart_workspace_bytes(n))


def denormalize(values_ptr: int, n: int, state_ptr: int, stream=None) -> None:
    """fi_popart_denormalize."""
    check(lib().fi_popart_denormalize(values_ptr, n, state_ptr, stream), "fi_popart_denormalize")


def scale_grad(dvalue_ptr: int, n: int, state_ptr: int, stream=None) -> None:
    """fi_popart_scale_grad."""
    check(lib().fi_popart_scale_grad(dvalue_ptr, n, state_ptr, stream), "fi_popart_scale_grad")


def update(vs_ptr: int, n: int, state_ptr: int, w_ptr: int, w_stride: int, H: int, b_ptr: int, beta: float = BETA,
           sigma_min: float = SIGMA_MIN, sigma_max: float = SIGMA_MAX, skip_ptr=None, ws_ptr=None, ws_bytes: int = 0,
           stream=None) -> None:
    """fi_popart_update."""
    check(lib().fi_popart_update(vs_ptr, n, state_ptr, w_ptr, w_stride, H, b_ptr, beta, sigma_min, sigma_max, skip_ptr,
                                 ws_ptr, ws_bytes, stream), "fi_popart_update")


def pack_state(mu: float, nu: float, sigma: float, updates: int = 0) -> np.ndarray:
    """The 32 bytes of the device block, as uint8."""
    return np.frombuffer(np.array([mu, nu, sigma], np.float64).tobytes() + np.uint64(updates).tobytes(), np.uint8).copy()


def unpack_state(raw) -> dict:
    raw = np.ascontiguousarray(raw, np.uint8)
    f = raw[:24].view(np.float64)
    return dict(mu=float(f[0]), nu=float(f[1]), sigma=float(f[2]), updates=int(raw[24:32].view(np.uint64)[0]))
