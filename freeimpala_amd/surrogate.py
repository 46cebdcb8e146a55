"""Host side of the clipped surrogate policy loss on V-trace targets (include/fi_surrogate.h): a second
objective of the learner, -min(rho A, clip(rho, 1 - eps, 1 + eps) A) on V-trace's own value targets
(PPO, Schulman et al. 2017; IMPACT, Luo et al. 2020), in place of the V-trace policy gradient.

  learner.set_objective("surrogate", clip=0.2, normalize_advantages=True)
  learner.step_resident(); learner.objective_state()   # dict: objective, clip, rows_clipped, adv_mean, ...
  learner.set_objective("vtrace")                      # the V-trace step again, bit for bit

This module holds the ctypes table of the header, its two structures, the kernels alone on device
pointers (``surrogate_loss_dev``) and the whole rule in fp64 numpy (``surrogate_reference``, the tests'
reference, and ``near_rows``: the rows where fp32 may decide the clip the other way)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

CLIP, ADV_EPS = 0.2, 1e-8  # FI_SURROGATE_CLIP, FI_SURROGATE_ADV_EPS (as doubles; the ABI carries floats)
STATS_BYTES = 32           # the device block: uint64 rows, rows_clipped; double adv_mean, adv_std
NEAR_RHO, NEAR_ADV = 1e-4, 1e-6


class SurrogateParams(C.Structure):
    _fields_ = [("clip", C.c_float), ("normalize", C.c_uint32), ("adv_eps", C.c_float), ("reserved", C.c_uint32)]


class SurrogateState(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("normalize", C.c_uint32), ("clip", C.c_float), ("adv_eps", C.c_float),
                ("rows", C.c_uint64), ("rows_clipped", C.c_uint64), ("adv_mean", C.c_double), ("adv_std", C.c_double)]

    def as_dict(self) -> dict:
        return dict(enabled=bool(self.enabled), normalize=bool(self.normalize), clip=float(self.clip),
                    adv_eps=float(self.adv_eps), rows=int(self.rows), rows_clipped=int(self.rows_clipped),
                    adv_mean=float(self.adv_mean), adv_std=float(self.adv_std))


_P = C.c_void_p
_I = C.c_int
SIGNATURES = {  # every symbol include/fi_surrogate.h declares
    "fi_surrogate_enable": ([_P, C.POINTER(SurrogateParams)], C.c_int),
    "fi_surrogate_disable": ([_P], C.c_int),
    "fi_surrogate_get_state": ([_P, C.POINTER(SurrogateState)], C.c_int),
    "fi_surrogate_stats_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_surrogate_workspace_bytes": ([_I, _I, _I], C.c_size_t),
    "fi_surrogate_loss_blocks": ([_I, _I, _I], C.c_int),
    "fi_surrogate_loss_fp32": ([_I, _I, _I] + [_P] * 6 + [C.POINTER(_abi.VtraceHparams), C.POINTER(SurrogateParams)] +
                               [_P] * 7 + [C.c_size_t, _P, _P], C.c_int),
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


def params(clip: float = CLIP, normalize: bool = False, adv_eps: float = ADV_EPS) -> SurrogateParams:
    return SurrogateParams(clip, int(bool(normalize)), adv_eps, 0)


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def workspace_bytes(T: int, B: int, A: int) -> int:
    """fi_surrogate_workspace_bytes (needs no device); 0 for a refused shape."""
    return int(lib().fi_surrogate_workspace_bytes(T, B, A))


def loss_blocks(T: int, B: int, A: int) -> int:
    """fi_surrogate_loss_blocks: workgroups of the rows and of the loss kernel (needs no device)."""
    return int(lib().fi_surrogate_loss_blocks(T, B, A))


def scan_blocks(B: int) -> int:
    """Workgroups of the scan kernel: one wave of 64 columns each."""
    return (B + 63) // 64


def surrogate_loss_dev(T: int, B: int, A: int, pi: int, mu: int, act: int, rew: int, disc: int, val: int, hp, prm, vs: int,
                       adv: int, dlogits: int, dvalue: int, losses: int | None, stats: int | None, ws: int, ws_bytes: int,
                       bad: int | None = None, stream=None) -> None:
    """fi_surrogate_loss_fp32 on device pointers: enqueues the kernels; losses, stats and bad may be None."""
    check(lib().fi_surrogate_loss_fp32(T, B, A, pi, mu, act, rew, disc, val, C.byref(hp), C.byref(prm), vs, adv, dlogits,
                                       dvalue, losses, stats, ws, ws_bytes, bad, stream), "fi_surrogate_loss_fp32")


def unpack_stats(raw) -> dict:
    """The 32 bytes of the stats block as a dict."""
    raw = np.ascontiguousarray(raw, np.uint8)
    n, f = raw[:16].view(np.uint64), raw[16:32].view(np.float64)
    return dict(rows=int(n[0]), rows_clipped=int(n[1]), adv_mean=float(f[0]), adv_std=float(f[1]))


# ------------------------------------------------------------------ the rule on the host, in fp64
def _log_softmax(z):
    d = z - z.max(-1, keepdims=True)
    return d - np.log(np.exp(d).sum(-1, keepdims=True))


def _hp(hp) -> dict:
    if isinstance(hp, dict):
        return hp
    return {k: float(getattr(hp, k)) for k in ("rho_bar", "c_bar", "lambda_", "baseline_cost", "entropy_cost")}


def clip_bounds(clip: float) -> tuple[float, float]:
    """lo = 1.0f - clip and hi = 1.0f + clip, as the kernel forms them: in float."""
    c = np.float32(clip)
    with np.errstate(over="ignore"):
        return float(np.float32(1.0) - c), float(np.float32(1.0) + c)


def surrogate_reference(pi, mu, act, rew, disc, val, hp, clip: float = CLIP, normalize: bool = False,
                        adv_eps: float = ADV_EPS) -> dict:
    """The whole rule of include/fi_surrogate.h in fp64. pi, mu (T, B, A); act, rew, disc (T, B); val (T + 1, B);
    hp: a fi_vtrace_hparams or a dict with rho_bar, c_bar, lambda_, baseline_cost, entropy_cost. Returns vs,
    pg_adv (A, unnormalised), adv_used (A~), rho, log_rho, clipped (bool), dlogits, dvalue (T + 1, B),
    losses [L_pg, baseline, entropy], rows, rows_clipped, adv_mean, adv_std and bad (rows whose action was
    outside [0, A) and was clamped)."""
    h = _hp(hp)
    pi, mu = np.asarray(pi, np.float64), np.asarray(mu, np.float64)
    rew, disc, val = np.asarray(rew, np.float64), np.asarray(disc, np.float64), np.asarray(val, np.float64)
    act = np.asarray(act)
    T, B, A = pi.shape
    bad = int(((act < 0) | (act >= A)).sum())
    a = np.clip(act, 0, A - 1).astype(np.int64)[..., None]
    lpi, lmu = _log_softmax(pi), _log_softmax(mu)
    log_rho = np.take_along_axis(lpi, a, -1)[..., 0] - np.take_along_axis(lmu, a, -1)[..., 0]
    rho = np.exp(log_rho)
    rho_hat = np.minimum(h["rho_bar"], rho)
    c = h["lambda_"] * np.minimum(h["c_bar"], rho)
    vs = np.empty((T + 1, B))
    vs[T] = val[T]
    acc = np.zeros(B)
    for t in range(T - 1, -1, -1):
        acc = rho_hat[t] * (rew[t] + disc[t] * val[t + 1] - val[t]) + disc[t] * c[t] * acc
        vs[t] = val[t] + acc
    adv = rew + disc * vs[1:] - val[:T]
    n = T * B
    m = float(adv.sum() / n)
    s = float(np.sqrt(((adv - m) ** 2).sum() / n))
    lo, hi = clip_bounds(clip)
    eps = float(np.float32(adv_eps))
    used = (adv - m) / (s + eps) if normalize else adv
    clipped = ((used > 0) & (rho > hi)) | ((used < 0) & (rho < lo))
    l_pg = -np.minimum(rho * used, np.clip(rho, lo, hi) * used)
    g = np.where(clipped, 0.0, -rho * used)
    p = np.exp(lpi)
    plogp = (p * lpi).sum(-1)
    onehot = np.zeros((T, B, A))
    np.put_along_axis(onehot, a, 1.0, -1)
    dlogits = g[..., None] * (onehot - p) + h["entropy_cost"] * p * (lpi - plogp[..., None])
    dvalue = np.zeros((T + 1, B))
    dvalue[:T] = h["baseline_cost"] * (val[:T] - vs[:T])
    losses = np.array([l_pg.sum(), 0.5 * ((vs[:T] - val[:T]) ** 2).sum(), plogp.sum()])
    return dict(vs=vs[:T], pg_adv=adv, adv_used=used, rho=rho, log_rho=log_rho, clipped=clipped, dlogits=dlogits,
                dvalue=dvalue, losses=losses, rows=n, rows_clipped=int(clipped.sum()), adv_mean=m, adv_std=s, bad=bad)


def near_rows(pi, mu, act, rew, disc, val, hp, clip: float = CLIP, normalize: bool = False, adv_eps: float = ADV_EPS,
              ref: dict | None = None) -> int:
    """The rows where fp32 may decide the clip the other way than fp64: |rho / lo - 1| or |rho / hi - 1| <= 1e-4,
    or |A~| <= 1e-6. ref: a surrogate_reference of the same arguments, when there is one already."""
    r = surrogate_reference(pi, mu, act, rew, disc, val, hp, clip, normalize, adv_eps) if ref is None else ref
    lo, hi = clip_bounds(clip)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        near = (np.abs(r["rho"] / lo - 1.0) <= NEAR_RHO) | (np.abs(r["rho"] / hi - 1.0) <= NEAR_RHO)
    return int((near | (np.abs(r["adv_used"]) <= NEAR_ADV)).sum())
