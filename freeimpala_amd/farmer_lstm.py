"""Host side of FarmerLstm's bf16 LSTM mode (include/fi_farmer_lstm.h): bf16 operands, fp32 accumulation on the
gfx950 bf16 MFMA in batch-tiled recurrences, fp32 cell state (csrc/farmer_lstm_bf16.hip).

  model.set_lstm_precision("bf16")       # before the first step or forward; model.lstm_precision -> "bf16"

This module holds the ctypes table of the header and the rule in fp64 numpy (``lstm_bf16_reference``: the tests'
yardstick, with fp64 sums and activations where the device works in fp32)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .mlp_bf16 import rne

FP32, BF16 = 0, 1  # enum fi_farmer_lstm_precision
NAMES = {"fp32": FP32, "bf16": BF16}
I_IN, HID, G4 = 162, 128, 512

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_farmer_lstm.h declares
    "fi_farmer_set_lstm_precision": ([_P, C.c_int], C.c_int),
    "fi_farmer_lstm_precision": ([_P], C.c_int),
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


def precision(p) -> int:
    if isinstance(p, str):
        if p not in NAMES:
            raise ValueError(f"lstm precision: fp32 | bf16, not {p!r}")
        return NAMES[p]
    return int(p)


def split_lstm_params(params) -> dict:
    """The LSTM's part of the fp32 blob (state_dict order) as fp64 arrays: W_ih (512, 162), W_hh (512, 128) and
    b = b_ih + b_hh, added in fp32 as the device adds them; unrounded."""
    p = np.asarray(params, np.float32)
    o1, o2 = G4 * I_IN, G4 * I_IN + G4 * HID
    return dict(W_ih=p[:o1].reshape(G4, I_IN).astype(np.float64), W_hh=p[o1:o2].reshape(G4, HID).astype(np.float64),
                b=(p[o2:o2 + G4] + p[o2 + G4:o2 + 2 * G4]).astype(np.float64))


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def lstm_bf16_reference(z, params, dcat, rounded: bool = True) -> dict:
    """The rule of fi_farmer_lstm.h in fp64. z (B, T, 162) fp32, params the fp32 blob, dcat (B, >= 128): the
    upstream gradient of h_{T-1} in its first 128 columns. Every product has bf16 operands; every sum and activation
    is fp64 here (fp32 on the device); gates, hprev and dG are rounded to bf16 where the device stores them.
    rounded=False: the same LSTM with no rounding at all. Returns xp (B, T, 512), gates, c (B, T, 128), hprev
    (row t: the handed-on h_{t-1}), h_T (B, 128), dG (B, T, 512), gW_ih, gW_hh and gb."""
    q = rne if rounded else (lambda a: np.asarray(a, np.float64))
    P = split_lstm_params(params)
    W_ih, W_hh = q(P["W_ih"]), q(P["W_hh"])
    zq = q(np.asarray(z, np.float32))
    B, T, _ = zq.shape
    xp = zq @ W_ih.T + P["b"]
    gates, c, hprev = np.zeros((B, T, G4)), np.zeros((B, T, HID)), np.zeros((B, T, HID))
    hq, ct, h = np.zeros((B, HID)), np.zeros((B, HID)), np.zeros((B, HID))
    for t in range(T):
        pre = xp[:, t] + hq @ W_hh.T
        i, f, o = (sigmoid(pre[:, k * HID:(k + 1) * HID]) for k in (0, 1, 3))
        g = np.tanh(pre[:, 2 * HID:3 * HID])
        ct = f * ct + i * g
        h = o * np.tanh(ct)
        gates[:, t], c[:, t], hprev[:, t] = q(np.concatenate([i, f, g, o], 1)), ct, hq
        hq = q(h)
    dG = np.zeros((B, T, G4))
    dh, dc = np.asarray(dcat, np.float64)[:, :HID], np.zeros((B, HID))
    for t in range(T - 1, -1, -1):
        i, f, g, o = (gates[:, t, k * HID:(k + 1) * HID] for k in range(4))
        tc = np.tanh(c[:, t])
        dc = dc + dh * o * (1.0 - tc * tc)
        cp = c[:, t - 1] if t > 0 else 0.0
        dG[:, t] = q(np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g),
                                     dh * tc * o * (1 - o)], 1))
        dc = dc * f
        dh = dG[:, t] @ W_hh
    d2 = dG.reshape(B * T, G4)
    return dict(xp=xp, gates=gates, c=c, hprev=hprev, h_T=h, dG=dG, gW_ih=d2.T @ zq.reshape(B * T, I_IN),
                gW_hh=d2.T @ hprev.reshape(B * T, HID), gb=d2.sum(0))
