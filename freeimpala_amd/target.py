"""Host side of the learner's target network (include/fi_target.h): IMPACT's clipped ratio (Luo et al. 2020)
around a slowly moving copy theta- of the learner's parameters. V-trace's importance weights are taken
against the copy (pi_tgt / mu), the surrogate's trust region around it (pi / pi_tgt).

  learner.set_objective("surrogate", clip=0.2)
  learner.enable_target(period=4, tau=1.0)
  learner.step_ring(ring, n_fresh=...); learner.target_state()   # dict: period, tau, updates, mean_log_r, ...
  learner.disable_target()                                      # the plain surrogate step again, bit for bit

This module holds the ctypes table of the header, its two structures, the kernels alone on device
pointers (``target_loss_dev``, ``target_update_dev``) and the rule in fp64 numpy (``target_reference``,
``update_reference``: the tests' references, and ``near_rows``: the rows where fp32 may decide the clip, or
the sign of A~, the other way)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, surrogate
from ._abi import check
from .surrogate import ADV_EPS, CLIP, NEAR_ADV, NEAR_RHO, SurrogateParams, _log_softmax, clip_bounds

PERIOD, TAU = 4, 1.0  # FI_TARGET_PERIOD, FI_TARGET_TAU
STATS_BYTES = 32      # the device block: uint64 updates, rows; double mean_log_r, mean_sq_log_r


class TargetParams(C.Structure):
    _fields_ = [("period", C.c_uint32), ("tau", C.c_float), ("reserved", C.c_uint32 * 2)]


class TargetStats(C.Structure):
    _fields_ = [("updates", C.c_uint64), ("rows", C.c_uint64), ("mean_log_r", C.c_double), ("mean_sq_log_r", C.c_double)]

    def as_dict(self) -> dict:
        return dict(updates=int(self.updates), rows=int(self.rows), mean_log_r=float(self.mean_log_r),
                    mean_sq_log_r=float(self.mean_sq_log_r))


_P = C.c_void_p
_I = C.c_int
SIGNATURES = {  # every symbol include/fi_target.h declares
    "fi_target_enable": ([_P, C.POINTER(TargetParams)], C.c_int),
    "fi_target_disable": ([_P], C.c_int),
    "fi_target_sync": ([_P], C.c_int),
    "fi_target_get_params": ([_P, _P, C.c_size_t], C.c_int),
    "fi_target_set_params": ([_P, _P, C.c_size_t], C.c_int),
    "fi_target_get_state": ([_P, C.POINTER(TargetParams), C.POINTER(TargetStats), C.POINTER(C.c_uint32)], C.c_int),
    "fi_target_params_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_target_logits_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_target_stats_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_target_workspace_bytes": ([_I, _I, _I], C.c_size_t),
    "fi_target_loss_fp32": ([_I, _I, _I] + [_P] * 7 + [C.POINTER(_abi.VtraceHparams), C.POINTER(SurrogateParams)] +
                            [_P] * 8 + [C.c_size_t, _P, _P], C.c_int),
    "fi_target_update": ([_P, _P, C.c_size_t, C.c_float, _P, _P], C.c_int),
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


def params(period: int = PERIOD, tau: float = TAU) -> TargetParams:
    return TargetParams(period, tau, (C.c_uint32 * 2)(0, 0))


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def workspace_bytes(T: int, B: int, A: int) -> int:
    """fi_target_workspace_bytes (needs no device); 0 for a refused shape."""
    return int(lib().fi_target_workspace_bytes(T, B, A))


def target_loss_dev(T: int, B: int, A: int, pi: int, tgt: int, mu: int, act: int, rew: int, disc: int, val: int, hp, prm,
                    vs: int, adv: int, dlogits: int, dvalue: int, losses: int | None, sur_stats: int | None,
                    tgt_stats: int | None, ws: int, ws_bytes: int, bad: int | None = None, stream=None) -> None:
    """fi_target_loss_fp32 on device pointers: enqueues the kernels; losses, the two blocks and bad may be None."""
    check(lib().fi_target_loss_fp32(T, B, A, pi, tgt, mu, act, rew, disc, val, C.byref(hp), C.byref(prm), vs, adv, dlogits,
                                    dvalue, losses, sur_stats, tgt_stats, ws, ws_bytes, bad, stream), "fi_target_loss_fp32")


def target_update_dev(params_ptr: int, target_ptr: int, n: int, tau: float, skip: int | None = None, stream=None) -> None:
    """fi_target_update on device pointers: target <- tau-step towards params; skip: two device ints or None."""
    check(lib().fi_target_update(params_ptr, target_ptr, n, tau, skip, stream), "fi_target_update")


def unpack_stats(raw) -> dict:
    """The 32 bytes of the target's stats block as a dict."""
    raw = np.ascontiguousarray(raw, np.uint8)
    n, f = raw[:16].view(np.uint64), raw[16:32].view(np.float64)
    return dict(updates=int(n[0]), rows=int(n[1]), mean_log_r=float(f[0]), mean_sq_log_r=float(f[1]))


# ------------------------------------------------------------------ the rule on the host, in fp64
def _hp(hp) -> dict:
    if isinstance(hp, dict):
        return hp
    return {k: float(getattr(hp, k)) for k in ("rho_bar", "c_bar", "pg_rho_bar", "lambda_", "baseline_cost", "entropy_cost")}


def target_reference(pi, tgt, mu, act, rew, disc, val, hp, clip: float = CLIP, normalize: bool = False,
                     adv_eps: float = ADV_EPS) -> dict:
    """The rule of include/fi_target.h from 2. on, in fp64. pi, tgt, mu (T, B, A); act, rew, disc (T, B); val
    (T + 1, B); hp: a fi_vtrace_hparams or a dict with rho_bar, c_bar, pg_rho_bar, lambda_, baseline_cost,
    entropy_cost. Returns what surrogate_reference returns -- vs, pg_adv, adv_used, rho and log_rho (pi_tgt
    against mu), clipped, dlogits, dvalue, losses, rows, rows_clipped, adv_mean, adv_std, bad -- plus r and log_r
    (pi against pi_tgt), beta, mean_log_r and mean_sq_log_r."""
    h = _hp(hp)
    # 2. the targets: the surrogate's own, with pi_tgt where pi stood (clip and normalisation do not enter them)
    s = surrogate.surrogate_reference(tgt, mu, act, rew, disc, val, h, clip, normalize, adv_eps)
    pi, tg = np.asarray(pi, np.float64), np.asarray(tgt, np.float64)
    val = np.asarray(val, np.float64)
    T, B, A = pi.shape
    a = np.clip(np.asarray(act), 0, A - 1).astype(np.int64)[..., None]
    lpi, ltg = _log_softmax(pi), _log_softmax(tg)
    log_r = np.take_along_axis(lpi, a, -1)[..., 0] - np.take_along_axis(ltg, a, -1)[..., 0]
    r = np.exp(log_r)
    beta = np.minimum(h["pg_rho_bar"], s["rho"])
    used = s["adv_used"]
    lo, hi = clip_bounds(clip)
    clipped = ((used > 0) & (r > hi)) | ((used < 0) & (r < lo))
    l_pg = -beta * np.minimum(r * used, np.clip(r, lo, hi) * used)
    g = np.where(clipped, 0.0, -beta * r * used)
    p = np.exp(lpi)
    plogp = (p * lpi).sum(-1)
    onehot = np.zeros((T, B, A))
    np.put_along_axis(onehot, a, 1.0, -1)
    dlogits = g[..., None] * (onehot - p) + h["entropy_cost"] * p * (lpi - plogp[..., None])
    out = dict(s)
    out.update(clipped=clipped, rows_clipped=int(clipped.sum()), dlogits=dlogits,
               losses=np.array([l_pg.sum(), s["losses"][1], plogp.sum()]), r=r, log_r=log_r, beta=beta,
               mean_log_r=float(log_r.sum() / (T * B)), mean_sq_log_r=float((log_r ** 2).sum() / (T * B)))
    return out


def near_rows(pi, tgt, mu, act, rew, disc, val, hp, clip: float = CLIP, normalize: bool = False, adv_eps: float = ADV_EPS,
              ref: dict | None = None) -> int:
    """The rows where fp32 may decide the clip, or the sign of A~, the other way than fp64: |r / lo - 1| or
    |r / hi - 1| <= 1e-4, or |A~| <= 1e-6. ref: a target_reference of the same arguments, when there is one."""
    t = target_reference(pi, tgt, mu, act, rew, disc, val, hp, clip, normalize, adv_eps) if ref is None else ref
    lo, hi = clip_bounds(clip)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        near = (np.abs(t["r"] / lo - 1.0) <= NEAR_RHO) | (np.abs(t["r"] / hi - 1.0) <= NEAR_RHO)
    return int((near | (np.abs(t["adv_used"]) <= NEAR_ADV)).sum())


def update_reference(params, target, tau: float = TAU) -> np.ndarray:
    """theta- after one update, as float64: params when tau == 1, otherwise fmaf(tau, params - target, target)
    with the rule's roundings -- tau and the difference are floats, the product and the sum are exact up to
    fp64 -- so the kernel's float is this value rounded once: within one ulp (half of one, in fact)."""
    p, t = np.asarray(params, np.float32), np.asarray(target, np.float32)
    if np.float32(tau) == np.float32(1.0):
        return p.astype(np.float64)
    d = (p.astype(np.float64) - t.astype(np.float64)).astype(np.float32)  # the one fp32 rounding in front of the fma
    return float(np.float32(tau)) * d.astype(np.float64) + t.astype(np.float64)
