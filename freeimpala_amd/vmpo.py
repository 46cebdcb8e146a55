"""Host side of the V-MPO objective on the learner (include/fi_vmpo.h): the policy fitted by weighted maximum
likelihood to the top fraction of the batch's advantages, weights softmax(A / eta) over that part, the temperature
eta learned on the device from the dual loss (Song et al. 2020). No importance ratio in the policy term; the value
targets and advantages are V-trace's, the trust region is the KL penalty against the target network.

  learner.enable_target(period=4); learner.enable_kl_penalty("target", coeff=1.0)
  learner.set_objective("vmpo", top_fraction=0.5, eps_eta=0.01, lr_eta=1e-3)
  learner.step_ring(ring, n_fresh=...); learner.vmpo_state()   # dict: eta, selected, threshold, loss_eta, ...
  learner.set_objective("vtrace")                              # the V-trace step again, bit for bit

This module holds the ctypes table of the header, its two structures, the kernels alone on device pointers
(``select_dev``, ``vmpo_loss_dev``, ``eta_step_dev``) and the rule in fp64 numpy (``select_reference``,
``vmpo_reference``, ``eta_step_reference``: the tests' references, and ``near_tau``: the rows where an fp32 advantage
may fall on the other side of the threshold than its fp64 value)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import check

TOP_FRACTION, EPS_ETA, ETA_INIT, ETA_MIN, LR_ETA = 0.5, 0.01, 1.0, 1e-8, 1e-3  # FI_VMPO_*
STATE_BYTES = 88          # the device block, fi_vmpo_state
SELECT_WS_BYTES = 28928   # FI_VMPO_SELECT_WS_BYTES
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
NEAR_TAU = 1e-4


class VmpoParams(C.Structure):
    _fields_ = [("top_fraction", C.c_float), ("eps_eta", C.c_float), ("eta_init", C.c_float), ("eta_min", C.c_float),
                ("lr_eta", C.c_float), ("adapt", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def as_dict(self) -> dict:
        return dict(top_fraction=float(self.top_fraction), eps_eta=float(self.eps_eta), eta_init=float(self.eta_init),
                    eta_min=float(self.eta_min), lr_eta=float(self.lr_eta), adapt=bool(self.adapt))


class VmpoState(C.Structure):
    _fields_ = [("eta", C.c_double), ("m1", C.c_double), ("m2", C.c_double), ("updates", C.c_uint64), ("rows", C.c_uint64),
                ("selected", C.c_uint64), ("threshold", C.c_float), ("adv_max", C.c_float), ("loss_eta", C.c_double),
                ("d_eta", C.c_double), ("sum_e", C.c_double), ("sum_ea", C.c_double)]

    def as_dict(self) -> dict:
        return {k: (int if k in ("updates", "rows", "selected") else float)(getattr(self, k)) for k, _ in self._fields_}


OFFSETS = dict(eta=0, m1=8, m2=16, updates=24, rows=32, selected=40, threshold=48, adv_max=52, loss_eta=56, d_eta=64,
               sum_e=72, sum_ea=80)  # include/fi_vmpo.h

_P = C.c_void_p
_I = C.c_int
_PRM = C.POINTER(VmpoParams)
SIGNATURES = {  # every symbol include/fi_vmpo.h declares
    "fi_vmpo_enable": ([_P, _PRM], C.c_int),
    "fi_vmpo_disable": ([_P], C.c_int),
    "fi_vmpo_set_eta": ([_P, C.c_double], C.c_int),
    "fi_vmpo_get_state": ([_P, _PRM, C.POINTER(VmpoState), C.POINTER(C.c_uint32)], C.c_int),
    "fi_vmpo_state_dev": ([_P, C.POINTER(_P)], C.c_int),
    "fi_vmpo_workspace_bytes": ([_I, _I, _I], C.c_size_t),
    "fi_vmpo_select_blocks": ([C.c_int64], C.c_int),
    "fi_vmpo_select_fp32": ([C.c_int64, _P, _PRM, _P, _P, C.c_size_t, _P], C.c_int),
    "fi_vmpo_loss_fp32": ([_I, _I, _I] + [_P] * 5 + [C.POINTER(_abi.VtraceHparams), _PRM] + [_P] * 5 + [C.c_size_t, _P, _P],
                          C.c_int),
    "fi_vmpo_eta_step": ([_P, _PRM, _P, _P], C.c_int),
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


def params(top_fraction: float = TOP_FRACTION, eps_eta: float = EPS_ETA, eta_init: float = ETA_INIT, eta_min: float = ETA_MIN,
           lr_eta: float = LR_ETA, adapt: bool = True) -> VmpoParams:
    """fi_vmpo_params."""
    return VmpoParams(top_fraction, eps_eta, eta_init, eta_min, lr_eta, int(adapt), (C.c_uint32 * 2)(0, 0))


# ------------------------------------------------------------------ stand-alone kernels on device pointers
def workspace_bytes(T: int, B: int, A: int) -> int:
    """fi_vmpo_workspace_bytes (needs no device); 0 for a refused shape."""
    return int(lib().fi_vmpo_workspace_bytes(T, B, A))


def select_blocks(n: int) -> int:
    """fi_vmpo_select_blocks: workgroups of the histogram and sums kernels; each takes 2,048 rows per trip."""
    return int(lib().fi_vmpo_select_blocks(n))


def _ref(prm):
    return C.byref(prm) if prm is not None else None


def select_dev(n: int, adv: int, prm: VmpoParams, state: int, ws: int, ws_bytes: int, stream=None) -> None:
    """fi_vmpo_select_fp32 on device pointers: rows, selected, threshold, adv_max into the block."""
    check(lib().fi_vmpo_select_fp32(n, adv, _ref(prm), state, ws, ws_bytes, stream), "fi_vmpo_select_fp32")


def vmpo_loss_dev(T: int, B: int, A: int, pi: int, act: int, adv: int, vs: int, val: int, hp, prm: VmpoParams, state: int,
                  dlogits: int, dvalue: int, losses: int | None, ws: int, ws_bytes: int, bad: int | None = None,
                  stream=None) -> None:
    """fi_vmpo_loss_fp32 on device pointers, behind select_dev on the same adv, block and workspace."""
    check(lib().fi_vmpo_loss_fp32(T, B, A, pi, act, adv, vs, val, C.byref(hp), _ref(prm), state, dlogits, dvalue, losses, ws,
                                  ws_bytes, bad, stream), "fi_vmpo_loss_fp32")


def eta_step_dev(state: int, prm: VmpoParams, skip: int | None = None, stream=None) -> None:
    """fi_vmpo_eta_step on device pointers; skip: two device ints (the optimiser's flag words) or None."""
    check(lib().fi_vmpo_eta_step(state, _ref(prm), skip, stream), "fi_vmpo_eta_step")


def unpack_state(raw) -> dict:
    """The 88 bytes of the block as a dict."""
    return VmpoState.from_buffer_copy(np.ascontiguousarray(raw, np.uint8).tobytes()).as_dict()


def pack_state(eta: float = ETA_INIT, **fields) -> np.ndarray:
    """The block's 88 bytes, what a stand-alone launch is given."""
    return np.frombuffer(bytes(VmpoState(eta=eta, **fields)), np.uint8).copy()


# ------------------------------------------------------------------ the rule on the host, in fp64
def keys(adv) -> np.ndarray:
    """Rule 1: the order-preserving uint32 key of each float32 advantage."""
    u = (np.asarray(adv, np.float32).reshape(-1) + np.float32(0.0)).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_float(key) -> np.float32:
    k = np.uint32(key)
    return (k ^ (np.uint32(0x80000000) if k >> 31 else np.uint32(0xFFFFFFFF))).view(np.float32)


def rank(n: int, top_fraction: float) -> int:
    """k = max(1, floor((double)f * n)), f the float the structure holds."""
    return max(1, int(math.floor(float(np.float32(top_fraction)) * n)))


def select_reference(adv, top_fraction: float = TOP_FRACTION) -> dict:
    """Rule 2 on a float32 array: k, key_tau, threshold (its float), m = selected, adv_max and the mask of D."""
    ky = keys(adv)
    n = ky.size
    k = rank(n, top_fraction)
    tau = np.sort(ky)[n - k]
    mask = ky >= tau
    return dict(rows=n, k=k, key_tau=int(tau), threshold=key_float(tau), selected=int(mask.sum()), adv_max=key_float(ky.max()),
                mask=mask.reshape(np.shape(adv)))


def _hp(hp) -> dict:
    if isinstance(hp, dict):
        return hp
    return {k: float(getattr(hp, k)) for k in ("baseline_cost", "entropy_cost")}


def _select64(adv, top_fraction):
    a = np.asarray(adv, np.float64) + 0.0
    n = a.size
    k = rank(n, top_fraction)
    tau = np.partition(a.reshape(-1), n - k)[n - k]
    return a, n, k, tau


def near_tau(adv, top_fraction: float = TOP_FRACTION) -> int:
    """Rows other than tau's own within 1e-4 of tau: there an fp32 advantage may be selected the other way."""
    a, _, _, tau = _select64(adv, top_fraction)
    return int((np.abs(a - tau) <= NEAR_TAU).sum()) - 1


def vmpo_reference(pi, act, adv, vs, val, hp, eta: float = ETA_INIT, top_fraction: float = TOP_FRACTION,
                   eps_eta: float = EPS_ETA) -> dict:
    """Rules 2 to 5's scalars in fp64. pi (T, B, A); act, adv, vs (T, B); val (T + 1, B); hp: a fi_vtrace_hparams or
    a dict with baseline_cost, entropy_cost; eta: the block's double (the weights use it rounded to a float, as the
    kernel does). adv float32: the selection is the kernel's own, value for value; float64 (another reference's):
    see near_tau. Returns dlogits, dvalue (T + 1, B), losses [L_pg, baseline, entropy], psi, mask, rows, selected,
    threshold, adv_max, sum_e, sum_ea, loss_eta, d_eta, x_max (max |x| over D) and bad."""
    h = _hp(hp)
    pi, vs, val = np.asarray(pi, np.float64), np.asarray(vs, np.float64), np.asarray(val, np.float64)
    act = np.asarray(act)
    T, B, A = pi.shape
    a, n, k, tau = _select64(adv, top_fraction)
    a = a.reshape(T, B)
    mask = a >= tau
    amax = a.max()
    eta_f = float(np.float32(eta))
    with np.errstate(all="ignore"):
        x = (a - amax) / eta_f
        e = np.where(mask, np.exp(x), 0.0)
        if not np.isfinite(a).all():
            e = np.full_like(e, np.nan)  # rule 6
        S, W = float(e.sum()), float((e * (a - amax)).sum())
        psi = e / S
        m = int(mask.sum())
        lsm = math.log(S / m) if S > 0 else math.nan
        loss_eta = eta * float(np.float32(eps_eta)) + amax + eta * lsm
        d_eta = float(np.float32(eps_eta)) + lsm - W / (S * eta)
    bad = int(((act < 0) | (act >= A)).sum())
    ai = np.clip(act, 0, A - 1).astype(np.int64)[..., None]
    d = pi - pi.max(-1, keepdims=True)
    lpi = d - np.log(np.exp(d).sum(-1, keepdims=True))
    p = np.exp(lpi)
    plogp = (p * lpi).sum(-1)
    onehot = np.zeros((T, B, A))
    np.put_along_axis(onehot, ai, 1.0, -1)
    g = -n * psi
    dlogits = g[..., None] * (onehot - p) + h["entropy_cost"] * p * (lpi - plogp[..., None])
    dvalue = np.zeros((T + 1, B))
    dvalue[:T] = h["baseline_cost"] * (val[:T] - vs)
    la = np.take_along_axis(lpi, ai, -1)[..., 0]
    losses = np.array([(g * la)[mask].sum(), 0.5 * ((vs - val[:T]) ** 2).sum(), plogp.sum()])
    return dict(dlogits=dlogits, dvalue=dvalue, losses=losses, psi=psi, mask=mask, rows=n, selected=m, threshold=float(tau),
                adv_max=float(amax), sum_e=S, sum_ea=W, loss_eta=float(loss_eta), d_eta=float(d_eta),
                d_eta_terms=(float(np.float32(eps_eta)), lsm, W / (S * eta)), x_max=float(np.abs(x[mask]).max()), bad=bad)


def eta_step_reference(state: dict, d_eta: float, prm, skipped: bool = False) -> dict:
    """Rule 5's update on a block (a dict as unpack_state's): the block behind fi_vmpo_eta_step when the loss kernel
    left d_eta. prm: a VmpoParams or a dict with adapt, lr_eta, eta_min. Python floats are doubles, as the kernel's."""
    p = prm if isinstance(prm, dict) else prm.as_dict()
    s = dict(state)
    s["d_eta"] = float(d_eta)
    if skipped or not p["adapt"] or not math.isfinite(d_eta):
        return s
    t = s["updates"] + 1
    s["m1"] = BETA1 * s["m1"] + (1.0 - BETA1) * d_eta
    s["m2"] = BETA2 * s["m2"] + (1.0 - BETA2) * d_eta * d_eta
    mh, vh = s["m1"] / (1.0 - BETA1 ** t), s["m2"] / (1.0 - BETA2 ** t)
    s["eta"] = max(p["eta_min"], s["eta"] - p["lr_eta"] * mh / (math.sqrt(vh) + ADAM_EPS))
    s["updates"] = t
    return s
