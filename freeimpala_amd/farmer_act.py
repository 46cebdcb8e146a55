"""Host side of FarmerLstm's acting branch (include/fi_farmer_act.h, csrc/farmer_act.hip): many decision points per
call, each with its own set of candidate rows that share one history z; one bf16 LSTM pass per decision point, an
inference torso on the gfx950 bf16 MFMA that keeps its activations in LDS, and the pick made on the device.

  actor = FarmerActor(max_states=256, max_rows=4096, seq_length=10, seed=1)
  actor.set_params_from(model)                       # device to device, behind the learner's stream
  out = actor.act(z, x, offsets, epsilon=0.01)       # z (S, T, 162), x (N, 484), offsets (S + 1,)
  out["actions"]                                     # (S,) row inside each decision point, -1 for an empty one

This module holds the ctypes table of the header and the rule in fp64 numpy: ``act_reference`` (LSTM, torso, value)
and ``pick_reference`` (the pick, exact). There is no CPU path: the library missing or no device present raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from . import hip
from .env import philox4
from .farmer import HID, I_IN, X_IN
from .farmer_lstm import lstm_bf16_reference
from .mlp_bf16 import rne

ST_FARMER_ACT = 11  # the Philox stream of the exploration draws (csrc/fi_common.h)
W, CAT = 512, HID + X_IN


class FarmerActorConfig(C.Structure):
    _fields_ = [("max_states", C.c_int32), ("max_rows", C.c_int32), ("seq_len", C.c_int32), ("device", C.c_int32),
                ("seed", C.c_uint64)]


_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_farmer_act.h declares
    "fi_farmer_actor_config_init": ([C.POINTER(FarmerActorConfig)], None),
    "fi_farmer_actor_create": ([C.POINTER(FarmerActorConfig), C.POINTER(_P)], C.c_int),
    "fi_farmer_actor_destroy": ([_P], None),
    "fi_farmer_actor_set_params": ([_P, _P, C.c_size_t], C.c_int),
    "fi_farmer_actor_set_params_from": ([_P, _P], C.c_int),
    "fi_farmer_actor_act": ([_P, _P, _P, C.c_int, _P, C.c_int, C.c_float, _P, _P, _P, _P], C.c_int),
    "fi_farmer_actor_set_trace": ([_P, C.c_int], C.c_int),
    "fi_farmer_actor_tensor": ([_P, C.c_char_p, C.POINTER(_P), C.POINTER(C.c_size_t)], C.c_int),
    "fi_farmer_actor_nonfinite": ([_P, C.POINTER(C.c_uint64)], C.c_int),
    "fi_farmer_actor_stream": ([_P], _P),
    "fi_farmer_actor_set_profiling": ([_P, C.c_int], C.c_int),
    "fi_farmer_actor_kernel_ms": ([_P] + [C.POINTER(C.c_float)] * 3, C.c_int),
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


class FarmerActor:
    """The device actor. ``act`` takes host arrays, or device pointers (ints) with ``on_device=True``."""

    def __init__(self, max_states: int, max_rows: int, seq_length: int = 10, seed: int = 0, device: int = 0):
        cfg = FarmerActorConfig()
        lib().fi_farmer_actor_config_init(C.byref(cfg))
        cfg.max_states, cfg.max_rows, cfg.seq_len, cfg.seed, cfg.device = max_states, max_rows, seq_length, seed, device
        h = _P()
        _abi.check(lib().fi_farmer_actor_create(C.byref(cfg), C.byref(h)), "fi_farmer_actor_create")
        self._h = h
        self.max_states, self.max_rows, self.T, self.seed = max_states, max_rows, seq_length, seed
        self.S = self.N = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().fi_farmer_actor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, p) -> None:
        p = np.ascontiguousarray(p, np.float32)
        _abi.check(lib().fi_farmer_actor_set_params(self._h, p.ctypes.data, p.size), "fi_farmer_actor_set_params")

    def set_params_from(self, model) -> None:
        """The parameters of a FarmerLstmModel on the same device, behind whatever its stream still holds."""
        _abi.check(lib().fi_farmer_actor_set_params_from(self._h, model._h), "fi_farmer_actor_set_params_from")

    def set_trace(self, on: bool = True) -> None:
        _abi.check(lib().fi_farmer_actor_set_trace(self._h, int(on)), "fi_farmer_actor_set_trace")

    def act(self, z, x, offsets, epsilon=0.0, on_device: bool = False) -> dict:
        """One call of the rule: actions, explored (S,) int32, best_value (S,) and values (N,) float32. epsilon is
        one number or one per decision point."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        S = offsets.size - 1
        N = int(offsets[-1]) if S >= 0 else 0
        if on_device:
            zp, xp = int(z), int(x)
        else:
            z, x = (np.ascontiguousarray(a, np.float32) for a in (z, x))
            assert z.shape == (S, self.T, I_IN) and x.shape == (N, X_IN), (z.shape, x.shape, S, N)
            zp, xp = z.ctypes.data, x.ctypes.data
        eps = np.asarray(epsilon, np.float32)
        per = np.ascontiguousarray(eps) if eps.ndim else None
        assert per is None or per.shape == (S,), per.shape
        actions, explored = np.empty(max(S, 0), np.int32), np.empty(max(S, 0), np.int32)
        values = np.empty(max(N, 0), np.float32)
        _abi.check(lib().fi_farmer_actor_act(self._h, zp, xp, int(on_device), offsets.ctypes.data, S,
                                             0.0 if per is not None else float(eps), per.ctypes.data if per is not None else None,
                                             actions.ctypes.data, explored.ctypes.data, values.ctypes.data),
                   "fi_farmer_actor_act")
        self.S, self.N = S, N
        best = self.tensor_array("actions", (3, S))[2].view(np.float32).copy()
        return dict(actions=actions, explored=explored, best_value=best, values=values)

    def tensor(self, name: str):
        p, n = _P(), C.c_size_t()
        _abi.check(lib().fi_farmer_actor_tensor(self._h, name.encode(), C.byref(p), C.byref(n)), "fi_farmer_actor_tensor")
        return p.value, n.value

    def tensor_array(self, name: str, shape=None, dtype=None) -> np.ndarray:
        """A copy of a named device tensor after the last call: "h" (max_states, 612) float32 with h in columns
        0..127, "values" (max_rows,), "actions" (3, S) int32, "trace" (5, N, 512) uint16 (bf16 bits), "params"."""
        kinds = {"h": (np.float32, (self.max_states, CAT)), "values": (np.float32, (self.max_rows,)),
                 "actions": (np.int32, (3, self.S)), "trace": (np.uint16, (5, self.N, W)), "params": (np.float32, (-1,))}
        dt, sh = kinds[name]
        p, n = self.tensor(name)
        dt = dtype or dt
        return hip.download_ptr(p, dt, (n // np.dtype(dt).itemsize,)).reshape(shape or sh)

    def set_profiling(self, on: bool = True) -> None:
        _abi.check(lib().fi_farmer_actor_set_profiling(self._h, int(on)), "fi_farmer_actor_set_profiling")

    def kernel_ms(self) -> dict:
        """Device ms of the last call's LSTM, torso and pick launches (profiling on)."""
        t = [C.c_float() for _ in range(3)]
        _abi.check(lib().fi_farmer_actor_kernel_ms(self._h, *[C.byref(v) for v in t]), "fi_farmer_actor_kernel_ms")
        return dict(zip(("lstm", "torso", "pick"), (v.value for v in t)))

    @property
    def nonfinite(self) -> int:
        n = C.c_uint64(0)
        _abi.check(lib().fi_farmer_actor_nonfinite(self._h, C.byref(n)), "fi_farmer_actor_nonfinite")
        return n.value


# ------------------------------------------------------------------ the rule in fp64
def split_torso_params(params) -> list:
    """[(W_l (512, K), b_l)] for l = 1..5 and (w6 (512,), b6) last, fp64, unrounded."""
    p = np.asarray(params, np.float32).astype(np.float64)
    assert p.size == 1_514_497, p.size
    o, out = 512 * (I_IN + HID) + 1024, []
    for K in (CAT, W, W, W, W):
        out.append((p[o:o + W * K].reshape(W, K), p[o + W * K:o + W * K + W]))
        o += W * K + W
    out.append((p[o:o + W], p[o + W]))
    return out


def layer_terms(a, Wl, b):
    """One layer's sums from its stored input a (rows, K), bf16 values: the pre-activation r = a . rne(W)^T + b and
    S, the sum of the absolute values of the same terms, |b| included."""
    wq = rne(Wl)
    return a @ wq.T + b, np.abs(a) @ np.abs(wq).T + np.abs(b)


def relu(r):
    """0 below 0, r otherwise: a NaN stays a NaN (fi_farmer_act.h 3.)."""
    return np.where(r < 0, 0.0, r)


def row_table(offsets) -> np.ndarray:
    o = np.asarray(offsets, np.int64)
    return np.repeat(np.arange(o.size - 1), np.diff(o))


def act_reference(z, x, offsets, params) -> dict:
    """Steps 1..4 of fi_farmer_act.h in fp64: every product has bf16 operands, every sum is fp64 here (fp32 on the
    device), h, x and a1..a5 are rounded to bf16 where they are handed on. Returns h (S, 128) unrounded, c (N, 612),
    a = [a1..a5] (N, 512), pre = [(r, S)] of the five layers before the ReLU, values (N,) and values_terms."""
    z = np.asarray(z, np.float32)
    h = lstm_bf16_reference(z, params, np.zeros((z.shape[0], HID)))["h_T"]
    P = split_torso_params(params)
    a = np.concatenate([rne(h)[row_table(offsets)], rne(np.asarray(x, np.float32).reshape(-1, X_IN))], 1)
    out = dict(h=h, c=a, a=[], pre=[])
    for Wl, b in P[:5]:
        r, S = layer_terms(a, Wl, b)
        a = rne(relu(r))
        out["pre"].append((r, S))
        out["a"].append(a)
    w6, b6 = P[5]
    out["values_terms"] = (a @ w6 + b6, np.abs(a) @ np.abs(w6) + abs(b6))
    out["values"] = out["values_terms"][0]
    return out


def pick_reference(values, offsets, eps, seed: int, draw: int) -> dict:
    """Step 5 of fi_farmer_act.h from the device's own values, exactly: actions, explored (S,) int32 and best_value
    (S,) float32, and the count of rows whose value is not finite."""
    v, o = np.asarray(values, np.float32), np.asarray(offsets, np.int64)
    S = o.size - 1
    eps = np.broadcast_to(np.asarray(eps, np.float32), (S,)).astype(np.float64)
    words = philox4(seed, np.uint64(draw) * np.uint64(S) + np.arange(S, dtype=np.uint64), ST_FARMER_ACT)
    actions, explored = np.full(S, -1, np.int32), np.zeros(S, np.int32)
    best = np.full(S, -np.inf, np.float32)
    for s in range(S):
        seg = v[o[s]:o[s + 1]]
        ok = np.isfinite(seg)
        if not ok.any():
            continue
        best[s] = seg[ok].max()
        actions[s] = int(np.flatnonzero(ok & (seg == best[s]))[0])
        if float(words[s, 0]) * 2.0 ** -32 < eps[s]:
            j = (int(words[s, 1]) * seg.size) >> 32
            if ok[j]:
                actions[s], explored[s] = j, 1
    return dict(actions=actions, explored=explored, best_value=best, nonfinite=int((~np.isfinite(v[:o[-1]])).sum()))
