"""Host side of parameter publication on the device (include/fi_publish.h): the learner's parameters
reach its actors through stream order alone, with no host copy and no host wait.

  tag = learner.publish()          # enqueued on the learner's stream into snapshot slot k mod 2
  actor.set_params_dev(learner)    # enqueued on the actor's stream behind the publication's event
  learner.published()              # (fp32 array, exact version): waits, for tests and hosts
  learner.publish_state()          # dict: publications, slot, tag, version, dtype, readers

in place of ``blob, version = learner.get_blob(); actor.set_params(blob, version)``: the two leave the
same bits in the actor. This module holds the ctypes table of the header, the kernel alone on device
pointers (``publish_copy``) and the host form of the rounding rule in numpy (``round_params``, the
tests' reference). ``DeviceLearner.publish / publish_state / published`` (learner.py) and
``Actor.set_params_dev / set_params_ptr / read_params`` (actor.py) bind the rest."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

FI_PUBLISH_MAX_READERS = 64
DTYPES = {_abi.FI_PUBLISH_FP32: "fp32", _abi.FI_PUBLISH_BF16: "bf16"}


class PublishState(C.Structure):
    _fields_ = [("publications", C.c_uint64), ("tag", C.c_uint64), ("version", C.c_uint64), ("slot", C.c_uint32),
                ("dtype", C.c_uint32), ("readers", C.c_uint32 * 2)]

    def as_dict(self) -> dict:
        return dict(publications=int(self.publications), tag=int(self.tag), version=int(self.version), slot=int(self.slot),
                    dtype=DTYPES.get(int(self.dtype), int(self.dtype)), readers=[int(self.readers[0]), int(self.readers[1])])


_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_publish.h declares
    "fi_publish_params": ([_P, C.POINTER(C.c_uint64)], C.c_int),
    "fi_publish_read": ([_P, _P, C.c_size_t, C.POINTER(C.c_uint64)], C.c_int),
    "fi_publish_get_state": ([_P, C.POINTER(PublishState)], C.c_int),
    "fi_publish_event": ([_P], _P),
    "fi_actor_set_params_ptr": ([_P, _P, C.c_size_t, C.c_uint64, _P, C.POINTER(_P)], C.c_int),
    "fi_actor_set_params_dev": ([_P, _P], C.c_int),
    "fi_actor_read_params": ([_P, _P, C.c_size_t], C.c_int),
    "fi_publish_copy": ([_P, _P, C.c_size_t, C.c_int, _P], C.c_int),
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


def _dtype(dtype) -> int:
    if isinstance(dtype, str):
        if dtype not in ("fp32", "bf16"):
            raise ValueError(f"dtype: fp32 | bf16, not {dtype!r}")
        return _abi.FI_PUBLISH_FP32 if dtype == "fp32" else _abi.FI_PUBLISH_BF16
    return int(dtype)


# ------------------------------------------------------------------ the rule on the host
def round_params(p, dtype) -> np.ndarray:
    """The published form of fp32 parameters, as a new fp32 array of p's shape. "fp32": p's bits.
    "bf16": every value rounded to bf16 and widened again -- round-to-nearest-even on the upper 16
    bits; where all exponent bits are set (Inf, NaN) the upper half is kept and its bit 6 is set when
    any of the lower 16 bits is, so a NaN stays a NaN with its sign; the lower 16 bits are zero."""
    u = np.ascontiguousarray(p, np.float32).view(np.uint32)
    if _dtype(dtype) == _abi.FI_PUBLISH_FP32:
        return u.copy().view(np.float32)
    special = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    kept = (u & np.uint32(0xffff0000)) | np.where((u & np.uint32(0xffff)) != 0, np.uint32(0x400000), np.uint32(0))
    # no carry leaves 32 bits: the largest u that takes the sum is 0xff7fffff
    rounded = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return np.where(special, kept, rounded).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ the kernel alone on device pointers
def publish_copy(dst_ptr: int, src_ptr: int, n: int, dtype, stream=None) -> None:
    """fi_publish_copy: dst[i] = the published form of src[i], i < n; both pointers 16-byte aligned."""
    check(lib().fi_publish_copy(dst_ptr, src_ptr, n, _dtype(dtype), stream), "fi_publish_copy")
