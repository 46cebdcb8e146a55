"""Host side of the device entry ring (include/fi_ring.h): the reference's SharedBuffer in device
memory, between recording ``Actor`` handles and a ``DeviceLearner`` on the same device.

  ring = EntryRing(learner.entry_bytes, capacity=4 * learner.B, seed=1)
  ... every actor acts and records at its own pace ...
  if actor.rollout_ready():
      ring.push_rollout(actor)                 # copy into slots, release: the actor runs on
  if ring.info()["head"] - ring.info()["tail"] >= learner.B:
      learner.step_ring(ring)                  # FIFO: the reference's readBatch(B)
      learner.step_ring(ring, n_fresh=B // 2)  # half fresh, half replayed from what is resident
      ring.last_entries(learner.B)             # the entry indices the step chose

This module holds the ctypes table of the header, the handle, the standalone kernels on device
pointers and ``ring_batch_entries``, the host form of the batch rule (the tests' reference).
``DeviceLearner.step_ring`` lives in learner.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import StepStats, check

ST_REPLAY = 7  # the Philox counter stream of the replay draws (csrc/fi_common.h)
MAX_CAPACITY = 2 ** 31 - 1


class RingState(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("entry_bytes", C.c_uint64), ("head", C.c_uint64), ("tail", C.c_uint64),
                ("draw", C.c_uint64), ("seed", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_P = C.c_void_p
_U64 = C.c_uint64
SIGNATURES = {  # every symbol include/fi_ring.h declares
    "fi_ring_create": ([C.c_int32, C.c_size_t, C.c_int64, _U64, C.POINTER(_P)], C.c_int),
    "fi_ring_destroy": ([_P], None),
    "fi_ring_info": ([_P, C.POINTER(RingState)], C.c_int),
    "fi_ring_seed": ([_P, _U64, _U64], C.c_int),
    "fi_ring_push": ([_P, _P, C.c_size_t, C.c_int32, _P], C.c_int),
    "fi_ring_pushed_event": ([_P], _P),
    "fi_ring_stream": ([_P], _P),
    "fi_ring_push_rollout": ([_P, _P], C.c_int),
    "fi_ring_read_slots": ([_P, C.c_int64, C.c_int32, _P, C.c_size_t], C.c_int),
    "fi_ring_last_entries": ([_P, _P, C.c_int32], C.c_int),
    "fi_learner_step_ring": ([_P, _P, C.c_int32, C.POINTER(StepStats)], C.c_int),
    "fi_learner_step_ring_async": ([_P, _P, C.c_int32], C.c_int),
    "fi_ring_copy_entries": ([_P, C.c_size_t, C.c_int64, _U64, _P, C.c_size_t, C.c_int32, _P], C.c_int),
    "fi_ring_fill_columns": ([_P, _P, _P, _P, C.c_size_t, C.c_int64, C.c_int32, C.c_int32] + [_U64] * 5 + [_P], C.c_int),
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


def ring_batch_entries(philox4, seed: int, draw: int, B: int, n_fresh: int, head: int, tail: int,
                       capacity: int) -> list[int]:
    """The batch rule on the host: the entry index of every column of a step with n_fresh fresh
    columns, from the ring's numbers before the call. ``philox4(seed, counter, stream)`` returns the
    four words of Philox4x32-10 (the oracle's). Column c < n_fresh is entry tail + c; column
    c >= n_fresh is lo + ((x_c * n_valid) >> 32), x_c = philox4(seed, draw * B + c, 7)[0], over the
    entries already read that are still resident: [lo, tail), lo = max(0, head - capacity)."""
    if not 0 <= n_fresh <= B:
        raise ValueError(f"n_fresh {n_fresh} outside 0 .. {B}")
    if n_fresh > head - tail:
        raise ValueError(f"{head - tail} entries unread, n_fresh = {n_fresh}")
    lo = head - capacity if head > capacity else 0
    n_valid = tail - lo
    if n_fresh < B and n_valid <= 0:
        raise ValueError("nothing to replay")
    out = [tail + c for c in range(n_fresh)]
    for c in range(n_fresh, B):
        x = int(philox4(seed, (draw * B + c) & (2 ** 64 - 1), ST_REPLAY)[0])
        out.append(lo + ((x * n_valid) >> 32))
    return out


class EntryRing:
    """One fi_ring handle: `capacity` slots of `entry_bytes` bytes in device memory."""

    def __init__(self, entry_bytes: int, capacity: int, seed: int = 0, device: int = 0):
        self._h = C.c_void_p()
        check(lib().fi_ring_create(device, entry_bytes, capacity, seed, C.byref(self._h)), "fi_ring_create")
        self.entry_bytes, self.capacity, self.device = int(entry_bytes), int(capacity), device

    def info(self) -> dict:
        """dict(capacity, entry_bytes, head, tail, draw, seed)."""
        st = RingState()
        check(lib().fi_ring_info(self._h, C.byref(st)), "fi_ring_info")
        return st.as_dict()

    def seed(self, seed: int, draw: int = 0) -> None:
        check(lib().fi_ring_seed(self._h, seed, draw), "fi_ring_seed")

    def push(self, ptr: int, stride: int, n: int, event=None) -> None:
        """n entries in device memory, `stride` bytes apart, once `event` has completed."""
        check(lib().fi_ring_push(self._h, ptr, stride, n, event), "fi_ring_push")

    def push_rollout(self, actor) -> None:
        """Acquire the actor's completed unroll, push it, release it with the pushed event."""
        check(lib().fi_ring_push_rollout(self._h, actor._h), "fi_ring_push_rollout")

    @property
    def pushed_event(self) -> int | None:
        return lib().fi_ring_pushed_event(self._h)

    @property
    def stream(self) -> int:
        return lib().fi_ring_stream(self._h)

    def read_slots(self, first_slot: int = 0, n: int | None = None) -> np.ndarray:
        """(n, entry_bytes) uint8: the slots first_slot .. first_slot + n - 1 (all by default)."""
        n = self.capacity - first_slot if n is None else n
        out = np.empty((max(n, 0), self.entry_bytes), np.uint8)
        check(lib().fi_ring_read_slots(self._h, first_slot, n, out.ctypes.data, out.nbytes), "fi_ring_read_slots")
        return out

    def read_entries(self, entries) -> np.ndarray:
        """(len(entries), entry_bytes) uint8: the slots that hold the given entry indices now."""
        slots = self.read_slots()
        return slots[[int(e) % self.capacity for e in entries]]

    def last_entries(self, B: int) -> list[int]:
        """The entry indices the last step_ring chose, column by column (B: that learner's batch)."""
        out = np.empty(max(B, 1), np.uint64)
        check(lib().fi_ring_last_entries(self._h, out.ctypes.data, B), "fi_ring_last_entries")
        return [int(e) for e in out[:B]]

    # --- prioritised replay (include/fi_prio.h; prio.py)
    def enable_priorities(self, eta: float = 0.9, init_priority: float = 1.0) -> None:
        """A u32 priority per slot: ``DeviceLearner.step_ring(prioritized=True)`` draws its replayed
        columns in proportion to it and refreshes it from the step's TD magnitudes."""
        from . import prio
        prio.enable(self, eta, init_priority)

    def priority_info(self) -> dict:
        """dict(enabled, eta, q_init, prio_hi, table_bytes)."""
        from . import prio
        return prio.info(self)

    def priorities(self, first_entry: int | None = None, n: int | None = None) -> np.ndarray:
        """(n,) uint32: the priorities of the entries first_entry .. first_entry + n - 1 (by default
        the whole replayable window [lo, tail))."""
        from . import prio
        i = self.info()
        lo = max(0, i["head"] - i["capacity"])
        first = lo if first_entry is None else first_entry
        return prio.read(self, first, i["tail"] - first if n is None else n)

    def set_priorities(self, first_entry: int, q) -> None:
        """The priorities of the entries first_entry .. first_entry + len(q) - 1, inside [lo, tail)."""
        from . import prio
        prio.write(self, first_entry, q)

    # --- exponents and importance weights (include/fi_weights.h; weights.py)
    def set_priority_exponents(self, alpha: float = 1.0, beta: float = 0.0) -> None:
        """alpha in [0, 1]: later refreshes store p^alpha. beta in [0, 1]: later prioritised steps weigh
        every replayed column's loss by (n_valid q / Q)^-beta over the batch's maximum."""
        from . import weights
        weights.set_exponents(self, alpha, beta)

    def priority_exponents(self) -> dict:
        """dict(alpha, beta, weights_valid)."""
        from . import weights
        return weights.exponents(self)

    def last_weights(self, B: int) -> np.ndarray:
        """(B,) float32: the importance weights of the last prioritised step (B: that learner's batch);
        all 1 when it computed none."""
        from . import weights
        return weights.last_weights(self, B)

    def close(self) -> None:
        if self._h:
            lib().fi_ring_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def copy_entries(dst_ptr: int, entry_bytes: int, capacity: int, first_entry: int, src_ptr: int, src_stride: int, n: int,
                 stream=None) -> None:
    """fi_ring_copy_entries on device pointers."""
    check(lib().fi_ring_copy_entries(dst_ptr, entry_bytes, capacity, first_entry, src_ptr, src_stride, n, stream),
          "fi_ring_copy_entries")


def fill_columns(cols_ptr: int, entries_ptr, versions_ptr, base_ptr: int, entry_bytes: int, capacity: int, B: int,
                 n_fresh: int, tail: int, lo: int, n_valid: int, seed: int, draw: int, stream=None) -> None:
    """fi_ring_fill_columns on device pointers."""
    check(lib().fi_ring_fill_columns(cols_ptr, entries_ptr, versions_ptr, base_ptr, entry_bytes, capacity, B, n_fresh,
                                     tail, lo, n_valid, seed, draw, stream), "fi_ring_fill_columns")
