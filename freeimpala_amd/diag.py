"""Host side of the off-policy diagnostics (include/fi_diag.h): how hard V-trace is working on a
learner step -- rho statistics, KL(mu | pi), entropies, the effective sample size, the clip rates
and the value head's explained variance -- reduced on the device from the tensors the step leaves there.

  d = learner.diagnostics(columns=True)     # after a step: enqueue + read, a dict
  learner.enqueue_diagnostics()             # or: enqueue behind the step, no host wait ...
  d = learner.read_diagnostics()            # ... and read later, steps enqueued in between or not

This module holds the ctypes table of the header, the ``OffPolicyDiag`` structure, the kernels alone on
device pointers (``offpolicy_diag_dev``), the launcher's grid (``plan``) and the rule in fp64 numpy
(``offpolicy_reference``, the tests' reference). ``DeviceLearner.diagnostics / enqueue_diagnostics /
read_diagnostics`` (learner.py) bind the handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

COUNTS = ("rows", "rows_used", "rows_bad_action", "rows_nonfinite", "n_rho_clipped", "n_c_clipped", "n_pg_clipped",
          "n_episode_ends")
DOUBLES = ("mean_log_rho", "mean_rho", "kl_mu_pi", "entropy_pi", "entropy_mu", "mean_abs_td", "mean_reward", "max_rho",
           "min_rho", "ess", "explained_variance")


class OffPolicyDiag(C.Structure):
    _fields_ = ([("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(n, C.c_uint64) for n in COUNTS] +
                [(n, C.c_double) for n in DOUBLES])

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n in COUNTS + DOUBLES}


_P = C.c_void_p
_D = C.POINTER(OffPolicyDiag)
SIGNATURES = {  # every symbol include/fi_diag.h declares
    "fi_diag_workspace_bytes": ([C.c_int, C.c_int, C.c_int], C.c_size_t),
    "fi_diag_plan": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "fi_diag_offpolicy": ([C.c_int, C.c_int, C.c_int] + [_P] * 7 + [C.POINTER(_abi.VtraceHparams)] + [_P] * 4 +
                          [C.c_size_t, _P], C.c_int),
    "fi_diag_enqueue": ([_P], C.c_int),
    "fi_diag_read": ([_P, _D, _P, _P, C.c_int32], C.c_int),
    "fi_diag_learner": ([_P, _D, _P, _P, C.c_int32], C.c_int),
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


def hparams(rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar: float = 1.0) -> _abi.VtraceHparams:
    """fi_vtrace_hparams with the three thresholds the diagnostics read (the others at their defaults)."""
    return _abi.VtraceHparams(rho_bar, c_bar, pg_rho_bar, 1.0, 0.5, 0.01)


def workspace_bytes(T: int, B: int, A: int) -> int:
    return int(lib().fi_diag_workspace_bytes(T, B, A))


def plan(T: int, B: int, A: int) -> tuple[int, int]:
    """(column_tiles, time_slices) of the launcher's grid: a workgroup owns 64 columns and one slice of T."""
    ct, ts = C.c_int(0), C.c_int(0)
    check(lib().fi_diag_plan(T, B, A, C.byref(ct), C.byref(ts)), "fi_diag_plan")
    return ct.value, ts.value


def offpolicy_diag_dev(T: int, B: int, A: int, pi: int, mu: int, act: int, rew: int, disc: int, val: int, vs: int, hp,
                       out: int, col_kl: int | None, col_log_rho: int | None, ws: int, ws_bytes: int, stream=None) -> None:
    """fi_diag_offpolicy on device pointers: enqueues the two kernels; the column pointers may be None."""
    check(lib().fi_diag_offpolicy(T, B, A, pi, mu, act, rew, disc, val, vs, C.byref(hp), out, col_kl, col_log_rho, ws,
                                  ws_bytes, stream), "fi_diag_offpolicy")


def brief(d: dict) -> dict:
    """What a training script reports of a summary: the three clip rates (clipped / used rows),
    kl_mu_pi, ess, max_rho and explained_variance; None where there is no number (no used row)."""
    n = d["rows_used"]

    def num(x):
        return None if x != x else float(f"{x:.6g}")
    out = {k: (round(d[f"n_{k}_clipped"] / n, 4) if n else None) for k in ("rho", "c", "pg")}
    out = {f"{k}_clip_rate": v for k, v in out.items()}
    out.update({k: num(d[k]) for k in ("kl_mu_pi", "ess", "max_rho", "explained_variance")})
    return out


def enqueue_every(learner, u: int, every: int) -> int:
    """A training loop's ``--diagnostics K``: behind the step of every K-th unroll u, enqueue and do
    not wait. Returns u when it enqueued, else 0."""
    if not every or u % every:
        return 0
    learner.enqueue_diagnostics()
    return u


def report(learner, tag: str, pending: int, entry: dict) -> int:
    """In front of a report line: the newest enqueued diagnostics (of unroll ``pending``, 0: none) go
    into ``entry["diagnostics"]`` and, as one line, to stderr. Returns 0, the new ``pending``."""
    if pending:
        import sys
        entry["diagnostics"] = dict(unroll=pending, **brief(learner.read_diagnostics()))
        print(f"[{tag}] diagnostics " + " ".join(f"{k}={v}" for k, v in entry["diagnostics"].items()), file=sys.stderr,
              flush=True)
    return 0


def _log_softmax(z):
    m = z.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = z - m
        return d - np.log(np.exp(d).sum(-1, keepdims=True))


def offpolicy_reference(pi, mu, act, rew, disc, values, vs, hp):
    """The rule of fi_diag.h in fp64 numpy on the fp32 inputs: ``(summary dict, col_kl, col_log_rho)``.
    pi, mu (T, B, A) -- of a learner's logits the first T row blocks; act (T, B) int; rew, disc, vs
    (T, B); values (T, B) or (T + 1, B), of which the first T rows count; hp: anything with rho_bar,
    c_bar and pg_rho_bar (fi_vtrace_hparams). The column arrays are fp64, NaN for a column with no
    used row."""
    pi = np.asarray(pi, np.float32).astype(np.float64)
    mu = np.asarray(mu, np.float32).astype(np.float64)
    T, B, A = pi.shape
    act = np.asarray(act).reshape(T, B).astype(np.int64)
    rew = np.asarray(rew, np.float32).astype(np.float64).reshape(T, B)
    disc = np.asarray(disc, np.float32).astype(np.float64).reshape(T, B)
    val = np.asarray(values, np.float32).astype(np.float64).reshape(-1, B)[:T]
    vs = np.asarray(vs, np.float32).astype(np.float64).reshape(T, B)
    bars = [float(np.float32(getattr(hp, k))) for k in ("rho_bar", "c_bar", "pg_rho_bar")]

    bad_action = (act < 0) | (act >= A)
    nonfinite = ~bad_action & ~(np.isfinite(pi).all(-1) & np.isfinite(mu).all(-1))
    used = ~bad_action & ~nonfinite
    a = np.where(bad_action, 0, act)[..., None]
    with np.errstate(all="ignore"):
        lpi, lmu = _log_softmax(pi), _log_softmax(mu)
        lr = np.take_along_axis(lpi, a, -1)[..., 0] - np.take_along_axis(lmu, a, -1)[..., 0]
        rho = np.exp(lr)
        p_mu, p_pi = np.exp(lmu), np.exp(lpi)
        # 0 log 0 = 0: a logit far below the row's maximum has probability 0 in fp64 as in fp32
        kl = np.where(p_mu > 0, p_mu * (lmu - lpi), 0.0).sum(-1)
        h_pi = -np.where(p_pi > 0, p_pi * lpi, 0.0).sum(-1)
        h_mu = -np.where(p_mu > 0, p_mu * lmu, 0.0).sum(-1)
    td = vs - val
    n = int(used.sum())
    out = dict(rows=T * B, rows_used=n, rows_bad_action=int(bad_action.sum()), rows_nonfinite=int(nonfinite.sum()),
               n_rho_clipped=int((used & (rho > bars[0])).sum()), n_c_clipped=int((used & (rho > bars[1])).sum()),
               n_pg_clipped=int((used & (rho > bars[2])).sum()), n_episode_ends=int((disc == 0).sum()))
    if n == 0:
        out.update({k: float("nan") for k in DOUBLES})
    else:
        r = rho[used]
        # shifted by one of its elements (a variance does not depend on the shift): a constant vs gives exactly 0
        var_vs = float(np.var(vs[used] - vs[used][0]))
        out.update(mean_log_rho=float(lr[used].mean()), mean_rho=float(r.mean()), kl_mu_pi=float(kl[used].mean()),
                   entropy_pi=float(h_pi[used].mean()), entropy_mu=float(h_mu[used].mean()),
                   mean_abs_td=float(np.abs(td[used]).mean()), mean_reward=float(rew[used].mean()),
                   max_rho=float(r.max()), min_rho=float(r.min()), ess=float(r.sum() ** 2 / (n * (r * r).sum())),
                   explained_variance=(1.0 - float(np.var(td[used])) / var_vs) if var_vs > 0 else float("nan"))
    cnt = used.sum(0)
    with np.errstate(all="ignore"):
        col_kl = np.where(cnt > 0, np.where(used, kl, 0.0).sum(0) / cnt, np.nan)
        col_lr = np.where(cnt > 0, np.where(used, lr, 0.0).sum(0) / cnt, np.nan)
    return out, col_kl, col_lr
