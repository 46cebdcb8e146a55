"""Host side of the MLP policy's bf16 mode (include/fi_mlp.h): bf16 operands, fp32 accumulation on the
gfx950 bf16 MFMA, bf16 stored h1 / h2 / dz1 / dz2, fp32 everything else (csrc/mlp_bf16.hip).

  learner.set_mlp_precision("bf16")      # before the first step; learner.mlp_precision -> "bf16"
  actor.set_mlp_precision("bf16")        # the learner's forward kernel: the same logits, bit for bit

This module holds the ctypes table of the header and the rule in fp64 numpy (``mlp_bf16_reference``: the
tests' yardstick, with fp64 sums where the device accumulates in fp32)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .publish import round_params

FP32, BF16 = 0, 1  # enum fi_mlp_precision
NAMES = {"fp32": FP32, "bf16": BF16}

_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_mlp.h declares
    "fi_learner_set_mlp_precision": ([_P, C.c_int], C.c_int),
    "fi_learner_mlp_precision": ([_P], C.c_int),
    "fi_actor_set_mlp_precision": ([_P, C.c_int], C.c_int),
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
            raise ValueError(f"mlp precision: fp32 | bf16, not {p!r}")
        return NAMES[p]
    return int(p)


def supported(D: int, H: int, A: int) -> bool:
    """The widths the bf16 mode takes (fi_mlp.h)."""
    return 1 <= D <= 128 and 32 <= H <= 256 and H % 32 == 0 and 2 <= A <= 64


def rne(x) -> np.ndarray:
    """fp64 of the bf16 nearest (ties to even) to the fp32 value of x: publish.round_params, the rule of
    the published bf16 blob."""
    x32 = np.ascontiguousarray(x, np.float64).astype(np.float32)
    return round_params(x32.ravel(), "bf16").astype(np.float64).reshape(x32.shape)


def split_params(p, D: int, H: int, A: int) -> dict:
    """The fp32 slab as fp64 arrays: W1 (D, H), b1, W2 (H, H), b2, Wh (H, A + 1), bh; unrounded."""
    O = A + 1
    p = np.asarray(p, np.float32).astype(np.float64)
    sizes = [("W1", (D, H)), ("b1", (H,)), ("W2", (H, H)), ("b2", (H,)), ("Wh", (H, O)), ("bh", (O,))]
    out, o = {}, 0
    for nm, sh in sizes:
        n = int(np.prod(sh))
        out[nm] = p[o:o + n].reshape(sh)
        o += n
    assert o == p.size, (o, p.size)
    return out


def mlp_bf16_reference(obs, params, D: int, H: int, A: int, dout=None) -> dict:
    """The rule of fi_mlp.h in fp64. obs (rows, D) fp32, params the fp32 slab; dout (rows, A + 1) fp32 =
    [dlogits | dvalue] for the backward. Every product has bf16 operands; every sum is fp64 here (fp32 on
    the device); h1, h2, dz1, dz2 are rounded to bf16 where the device stores them; the masks come from
    the rounded h1 / h2. Returns h1, h2, logits, values and, with dout, dz2, dz1 and the gradient slab."""
    P = split_params(params, D, H, A)
    x = rne(np.asarray(obs, np.float32).reshape(-1, D))
    h1 = rne(np.maximum(x @ rne(P["W1"]) + P["b1"], 0.0))
    h2 = rne(np.maximum(h1 @ rne(P["W2"]) + P["b2"], 0.0))
    out = h2 @ rne(P["Wh"]) + P["bh"]
    ref = dict(h1=h1, h2=h2, logits=out[:, :A], values=out[:, A])
    if dout is None:
        return ref
    d = rne(np.asarray(dout, np.float32).reshape(-1, A + 1))
    dz2 = rne((d @ rne(P["Wh"]).T) * (h2 > 0))
    dz1 = rne((dz2 @ rne(P["W2"]).T) * (h1 > 0))
    grads = [x.T @ dz1, dz1.sum(0), h1.T @ dz2, dz2.sum(0), h2.T @ d, d.sum(0)]
    ref.update(dz2=dz2, dz1=dz1, grads=np.concatenate([g.ravel() for g in grads]))
    return ref
