"""Host side of a learner batch gathered from several device buffers (include/fi_gather.h).

Several recording ``Actor`` handles, each with its own ``num_envs``, stream and parameter version,
fill the columns of one ``DeviceLearner`` batch; their ``num_envs`` sum to the learner's batch:

  actors = [Actor("atari", n, ...) for n in sizes]          # sum(sizes) == learner.B
  ... every actor acts and records at its own pace ...
  if all(a.rollout_ready() for a in actors):
      learner.step_rollouts(actors)                         # gathering ingest, step, release
      learner.batch_versions                                # dict(min, max, mean, count)

This module holds the ctypes table of the header and the standalone gathering ingests on device
pointers. The methods live on ``DeviceLearner``."""
from __future__ import annotations

import ctypes as C

from . import _abi
from ._abi import StepStats, check

FI_MAX_SEGMENTS = 64


class EntrySegment(C.Structure):
    _fields_ = [("entries_dev", C.c_void_p), ("entry_stride", C.c_size_t), ("num_entries", C.c_int32),
                ("ready_event", C.c_void_p)]


class BatchVersions(C.Structure):
    _fields_ = [("min_version", C.c_uint32), ("max_version", C.c_uint32), ("sum_versions", C.c_uint64),
                ("count", C.c_uint64)]

    def as_dict(self) -> dict:
        return dict(min=int(self.min_version), max=int(self.max_version),
                    mean=self.sum_versions / self.count if self.count else 0.0, count=int(self.count))


_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_gather.h declares
    "fi_learner_step_segments_dev": ([_P, C.POINTER(EntrySegment), C.c_int32, C.POINTER(StepStats)], C.c_int),
    "fi_learner_step_segments_dev_async": ([_P, C.POINTER(EntrySegment), C.c_int32], C.c_int),
    "fi_learner_batch_versions": ([_P, C.POINTER(BatchVersions)], C.c_int),
    "fi_learner_step_rollouts": ([_P, C.POINTER(_P), C.c_int32, C.POINTER(StepStats)], C.c_int),
    "fi_learner_step_rollouts_async": ([_P, C.POINTER(_P), C.c_int32], C.c_int),
    "fi_ingest_atari_planes_gather": ([_P, C.c_int, C.c_int, C.c_int] + [_P] * 8, C.c_int),
    "fi_ingest_records_gather": ([_P, C.c_int, C.c_int, C.c_int, C.c_int] + [_P] * 8, C.c_int),
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


def segment_array(segments):
    """(ptr, stride, n, event) tuples -> a C array of fi_entry_segment."""
    segs = (EntrySegment * max(1, len(segments)))()
    for s, (ptr, stride, n, event) in zip(segs, segments):
        s.entries_dev, s.entry_stride, s.num_entries, s.ready_event = ptr, stride, n, event
    return segs


def actor_array(actors):
    return (_P * max(1, len(actors)))(*[a._h for a in actors])


def ingest_atari_planes_gather(cols_ptr: int, T: int, B: int, A: int, frames_ptr, mu_ptr, act_ptr, rew_ptr, disc_ptr,
                               bad_ptr=None, versions_ptr=None, stream=None) -> None:
    """fi_ingest_atari_planes_gather on device pointers (cols_ptr: B entry addresses in device memory)."""
    check(lib().fi_ingest_atari_planes_gather(cols_ptr, T, B, A, frames_ptr, mu_ptr, act_ptr, rew_ptr, disc_ptr,
                                              bad_ptr, versions_ptr, stream), "fi_ingest_atari_planes_gather")


def ingest_records_gather(cols_ptr: int, T: int, B: int, A: int, D: int, obs_ptr, mu_ptr, act_ptr, rew_ptr, disc_ptr,
                          bad_ptr=None, versions_ptr=None, stream=None) -> None:
    """fi_ingest_records_gather on device pointers."""
    check(lib().fi_ingest_records_gather(cols_ptr, T, B, A, D, obs_ptr, mu_ptr, act_ptr, rew_ptr, disc_ptr, bad_ptr,
                                         versions_ptr, stream), "fi_ingest_records_gather")
