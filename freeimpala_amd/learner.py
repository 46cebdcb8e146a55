"""Python handle over the HIP learner (C ABI ``fi_learner_*``).

Mirrors the surface freeimpala's C++ ``Learner`` exposes for the hot path
(reference include/freeimpala/learner.h): ``step(player_batch)`` is the body of
``Learner::trainModel(player_index, batch)`` (learner.h:32-49) where ``batch`` is what
``SharedBuffer::readBatch(M)`` returns (data_structures.h:267-300): M entries of
``entry_size * 1024`` bytes. The C++ Learner in include/freeimpala/learner.h calls the same
ABI; this module is the binding tests and bench.py use.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _abi
from ._abi import check, lib
from . import hip


class HostBatch:
    """M host entries pinned down once as a C pointer table (what Learner::step hands the ABI:
    `const void* const* entries`). Building the table costs ~1 us per entry in Python, so a
    caller that steps the same buffers repeatedly builds it once."""

    def __init__(self, batch: Sequence[bytes | bytearray | np.ndarray]):
        self.bufs = [np.frombuffer(e, dtype=np.uint8) if not isinstance(e, np.ndarray)
                     else np.ascontiguousarray(e).view(np.uint8).ravel() for e in batch]
        self.n = len(self.bufs)
        self.entry_bytes = min(b.nbytes for b in self.bufs) if self.bufs else 0
        self.ptrs = (C.c_void_p * self.n)(*[b.ctypes.data for b in self.bufs])


def _as_host_batch(batch) -> HostBatch:
    return batch if isinstance(batch, HostBatch) else HostBatch(batch)


class DeviceLearner:
    def __init__(self, arch: str = "mlp", seq_len: int = 100, batch: int = 32,
                 num_actions: int = 18, obs_dim: int = 128, hidden: int = 256,
                 optimizer: str = "adam", publish: str = "fp32", device: int = 0,
                 records: str = "stacked", **kw):
        if records not in ("stacked", "planes"):
            raise ValueError(f"records: stacked | planes, not {records!r}")
        self.cfg = _abi.default_config(
            arch=_abi.FI_ARCH_MLP if arch == "mlp" else _abi.FI_ARCH_ATARI, seq_len=seq_len,
            batch=batch, num_actions=num_actions, obs_dim=obs_dim, hidden=hidden,
            optimizer=_abi.FI_OPT_ADAM if optimizer == "adam" else _abi.FI_OPT_SGD,
            publish_dtype=_abi.FI_PUBLISH_FP32 if publish == "fp32" else _abi.FI_PUBLISH_BF16,
            device=device, **kw)
        self._h = C.c_void_p()
        check(lib().fi_learner_create(C.byref(self.cfg), C.byref(self._h)), "fi_learner_create")
        self.T, self.B, self.A = seq_len, batch, num_actions
        self.D, self.H = obs_dim, hidden
        self.arch = arch
        self.records = records
        try:
            if records == "planes":  # host entries carry single planes
                self.set_record_format(_abi.FI_RECORDS_PLANES)
            if optimizer == "rmsprop":  # created as "sgd" is, then switched (include/fi_train.h)
                self.set_rmsprop()
        except Exception:
            self.close()
            raise

    # --- sizes
    @property
    def param_count(self) -> int:
        return int(lib().fi_learner_param_count(self._h))

    @property
    def param_bytes(self) -> int:
        return int(lib().fi_learner_param_bytes(self._h))

    @property
    def entry_bytes(self) -> int:
        return int(lib().fi_learner_entry_bytes(self._h))

    @property
    def record_bytes(self) -> int:
        """Bytes of one step's record in a host entry: 1024 (MLP), 28672 (Atari), 7168 (Atari
        plane records)."""
        return int(lib().fi_learner_record_bytes(self._h))

    def set_record_format(self, fmt: int) -> None:
        """fi_learner_set_record_format: _abi.FI_RECORDS_STACKED | FI_RECORDS_PLANES, before the
        first host batch."""
        check(lib().fi_learner_set_record_format(self._h, fmt), "fi_learner_set_record_format")

    # --- the step
    def step(self, batch: Sequence[bytes | bytearray | np.ndarray] | HostBatch,
             stats: bool = True) -> dict:
        """Learner::step(player, batch): batch = M SharedBuffer entries (host bytes)."""
        hb = _as_host_batch(batch)
        st = _abi.StepStats()
        check(lib().fi_learner_step(self._h, hb.ptrs, hb.n, hb.entry_bytes,
                                    C.byref(st) if stats else None), "fi_learner_step")
        return st.as_dict() if stats else {}

    def step_async(self, batch: Sequence[bytes | bytearray | np.ndarray] | HostBatch) -> None:
        """Stage the entries (copied before return) and enqueue the step; see wait()."""
        hb = _as_host_batch(batch)
        check(lib().fi_learner_step_async(self._h, hb.ptrs, hb.n, hb.entry_bytes),
              "fi_learner_step_async")

    def acquire_staging(self) -> np.ndarray:
        """The next pinned staging buffer as a writable (B, entry_bytes) uint8 view
        (SharedBuffer::readBatchInto's destination); valid until it is submitted."""
        dst, stride = C.c_void_p(), C.c_size_t()
        check(lib().fi_learner_acquire_staging(self._h, C.byref(dst), C.byref(stride)),
              "fi_learner_acquire_staging")
        buf = (C.c_uint8 * (self.B * stride.value)).from_address(dst.value)
        return np.frombuffer(buf, np.uint8).reshape(self.B, stride.value)

    def step_staged(self, stats: bool = True) -> dict:
        st = _abi.StepStats()
        check(lib().fi_learner_step_staged(self._h, C.byref(st) if stats else None),
              "fi_learner_step_staged")
        return st.as_dict() if stats else {}

    def step_staged_async(self) -> None:
        check(lib().fi_learner_step_staged_async(self._h), "fi_learner_step_staged_async")

    def wait(self) -> dict:
        st = _abi.StepStats()
        check(lib().fi_learner_wait(self._h, C.byref(st)), "fi_learner_wait")
        return st.as_dict()

    def save_state(self) -> bytes:
        n = lib().fi_learner_state_bytes(self._h)
        buf = (C.c_char * n)()
        check(lib().fi_learner_save_state(self._h, buf, n), "fi_learner_save_state")
        return bytes(buf)

    def load_state(self, blob: bytes) -> None:
        check(lib().fi_learner_load_state(self._h, blob, len(blob)), "fi_learner_load_state")

    def step_resident(self, stats: bool = True) -> dict | None:
        st = _abi.StepStats()
        check(lib().fi_learner_step_resident(self._h, C.byref(st) if stats else None),
              "fi_learner_step_resident")
        return st.as_dict() if stats else None

    # --- entries already in device memory (include/fi_rollout.h)
    def step_rollout(self, actor, stats: bool = True) -> dict:
        """Acquire the actor's completed unroll, step from it in place, release it."""
        from . import rollout
        st = _abi.StepStats()
        check(rollout.lib().fi_learner_step_rollout(self._h, actor._h, C.byref(st) if stats else None),
              "fi_learner_step_rollout")
        return st.as_dict() if stats else {}

    def step_entries_dev(self, ptr: int, stride: int, event=None, stats: bool = True) -> dict:
        """Step from B entries in device memory, `stride` bytes apart, once `event` has completed."""
        from . import rollout
        st = _abi.StepStats()
        check(rollout.lib().fi_learner_step_entries_dev(self._h, ptr, stride, event, C.byref(st) if stats else None),
              "fi_learner_step_entries_dev")
        return st.as_dict() if stats else {}

    @property
    def entries_consumed_event(self) -> int | None:
        from . import rollout
        return rollout.lib().fi_learner_entries_consumed_event(self._h)

    @property
    def staging_bytes(self) -> int:
        """Pinned plus device bytes of the host-entry staging buffers (0 until a host batch came)."""
        from . import rollout
        return int(rollout.lib().fi_learner_staging_bytes(self._h))

    # --- a batch gathered from several device buffers (include/fi_gather.h)
    def step_rollouts(self, actors, stats: bool = True) -> dict:
        """Acquire every actor's completed unroll, step from them in place (actor k fills the next
        num_envs columns of the batch), release them all."""
        from . import gather
        st = _abi.StepStats()
        check(gather.lib().fi_learner_step_rollouts(self._h, gather.actor_array(actors), len(actors),
                                                    C.byref(st) if stats else None), "fi_learner_step_rollouts")
        return st.as_dict() if stats else {}

    def step_rollouts_async(self, actors) -> None:
        """The same, enqueued only: the unrolls are released at once, see wait()."""
        from . import gather
        check(gather.lib().fi_learner_step_rollouts_async(self._h, gather.actor_array(actors), len(actors)),
              "fi_learner_step_rollouts_async")

    # --- a batch chosen from a device entry ring (include/fi_ring.h)
    def step_ring(self, ring, n_fresh: int | None = None, wait: bool = True, prioritized: bool = False) -> dict | None:
        """Step from an ``EntryRing``: the first n_fresh columns (default: all B, the reference's
        readBatch(B)) take the oldest unread entries, the others are replayed from the entries read
        before that are still resident. wait=False: enqueued only, see wait(). prioritized=True
        (after ``ring.enable_priorities()``): the replayed columns are drawn in proportion to the
        entries' priorities, which the step refreshes (include/fi_prio.h)."""
        from . import ring as ring_mod
        n = self.B if n_fresh is None else n_fresh
        if prioritized:
            from . import prio
            if not wait:
                check(prio.lib().fi_learner_step_ring_prioritized_async(self._h, ring._h, n),
                      "fi_learner_step_ring_prioritized_async")
                return None
            st = _abi.StepStats()
            check(prio.lib().fi_learner_step_ring_prioritized(self._h, ring._h, n, C.byref(st)),
                  "fi_learner_step_ring_prioritized")
            return st.as_dict()
        if not wait:
            check(ring_mod.lib().fi_learner_step_ring_async(self._h, ring._h, n), "fi_learner_step_ring_async")
            return None
        st = _abi.StepStats()
        check(ring_mod.lib().fi_learner_step_ring(self._h, ring._h, n, C.byref(st)), "fi_learner_step_ring")
        return st.as_dict()

    # --- per-column loss weights (include/fi_weights.h)
    def set_column_weights(self, w) -> None:
        """(B,) finite weights >= 0: every later step's loss is sum_b w_b L_b, on every path, until
        ``set_column_weights(None)`` clears them. The reported losses stay the unweighted sums."""
        from . import weights
        weights.set_column_weights(self, w)

    def column_weights(self) -> np.ndarray:
        """(B,) float32: the weights that hold; all 1 when none are set."""
        from . import weights
        return weights.column_weights(self)

    # --- the training recipe (include/fi_train.h)
    def set_rmsprop(self, decay: float = 0.99, momentum: float = 0.0, eps: float = 0.01,
                    eps_in_sqrt: bool = False) -> None:
        """Switch the handle to RMSProp, before its first step (the defaults are monobeast's). The
        mean square lives in "adam_v" and the momentum buffer in "adam_m"."""
        from . import train
        check(train.lib().fi_train_set_rmsprop(self._h, decay, momentum, eps, int(bool(eps_in_sqrt))),
              "fi_train_set_rmsprop")

    def set_lr(self, lr: float) -> None:
        """Replace the base learning rate; between any two steps."""
        from . import train
        check(train.lib().fi_train_set_lr(self._h, lr), "fi_train_set_lr")

    def set_lr_schedule(self, lr_end: float, n_steps: int) -> None:
        """Anneal linearly from the base rate at update 1 to lr_end at update n_steps + 1 and beyond
        (``train.lr_at``)."""
        from . import train
        if n_steps < 0:
            raise ValueError(f"n_steps {n_steps} is negative")
        check(train.lib().fi_train_set_lr_schedule(self._h, lr_end, n_steps), "fi_train_set_lr_schedule")

    def clear_lr_schedule(self) -> None:
        from . import train
        check(train.lib().fi_train_clear_lr_schedule(self._h), "fi_train_clear_lr_schedule")

    def set_reward_clip(self, c: float) -> None:
        """Clamp the rewards of every later step to [-c, c] on the device, in front of V-trace; 0: off."""
        from . import train
        check(train.lib().fi_train_set_reward_clip(self._h, c), "fi_train_set_reward_clip")

    def train_state(self) -> dict:
        """fi_train_get_state as a dict: the optimiser and its numbers, the schedule, ``lr_next`` and
        ``next_update`` (the rate and the number the next enqueued update gets), the reward clip."""
        from . import train
        st = train.TrainState()
        check(train.lib().fi_train_get_state(self._h, C.byref(st)), "fi_train_get_state")
        return st.as_dict()

    # --- PopArt value normalisation (include/fi_popart.h; the rule: freeimpala_amd/popart.py)
    def enable_popart(self, beta: float = 3e-4, sigma_min: float = 1e-4, sigma_max: float = 1e6) -> None:
        """Every later step denormalises the value head's output with the statistics on the device,
        divides the value gradient by sigma and, behind the optimiser, moves mu, sigma towards the
        step's V-trace targets and rewrites the value column so that sigma n + mu is preserved. A
        second call changes the three numbers and keeps the statistics; there is no disable."""
        from . import popart
        check(popart.lib().fi_popart_enable(self._h, beta, sigma_min, sigma_max), "fi_popart_enable")

    def popart_state(self) -> dict:
        """Wait for the stream and return enabled, beta, sigma_min, sigma_max, mu, nu, sigma, updates."""
        from . import popart
        st = popart.PopartState()
        check(popart.lib().fi_popart_get_state(self._h, C.byref(st)), "fi_popart_get_state")
        return st.as_dict()

    def set_popart_state(self, mu: float, nu: float) -> None:
        """Resume: store mu, nu and the sigma they imply; no weight is rewritten. Call order of a
        resuming process: ``enable_popart``, ``set_popart_state``, ``load_state``."""
        from . import popart
        check(popart.lib().fi_popart_set_state(self._h, mu, nu), "fi_popart_set_state")

    def popart_state_ptr(self) -> int:
        """The device address of the 32-byte block {double mu, nu, sigma; uint64 updates}."""
        from . import popart
        p = C.c_void_p()
        check(popart.lib().fi_popart_state_dev(self._h, C.byref(p)), "fi_popart_state_dev")
        return int(p.value)

    # --- the learner's objective (include/fi_surrogate.h; the rule: freeimpala_amd/surrogate.py)
    def set_objective(self, name: str = "vtrace", clip: float = 0.2, normalize_advantages: bool = False,
                      adv_eps: float = 1e-8) -> None:
        """"surrogate": every later step runs the clipped surrogate -min(rho A, clip(rho, 1 - clip, 1 + clip) A)
        on V-trace's targets in place of the V-trace policy gradient, with the advantages normalised over the
        batch when asked; a second call replaces the numbers. "vtrace": the V-trace step again, bit for bit.
        Between any two steps."""
        from . import surrogate
        if name == "vtrace":
            check(surrogate.lib().fi_surrogate_disable(self._h), "fi_surrogate_disable")
        elif name == "surrogate":
            prm = surrogate.params(clip, normalize_advantages, adv_eps)
            check(surrogate.lib().fi_surrogate_enable(self._h, C.byref(prm)), "fi_surrogate_enable")
        else:
            raise ValueError(f"objective: vtrace | surrogate, not {name!r}")

    def objective_state(self) -> dict:
        """Wait for the stream and return objective ("vtrace" | "surrogate"), clip, normalize, adv_eps and the
        last surrogate step's stats block: rows, rows_clipped, adv_mean, adv_std."""
        from . import surrogate
        st = surrogate.SurrogateState()
        check(surrogate.lib().fi_surrogate_get_state(self._h, C.byref(st)), "fi_surrogate_get_state")
        d = st.as_dict()
        d["objective"] = "surrogate" if d.pop("enabled") else "vtrace"
        return d

    def surrogate_stats_ptr(self) -> int:
        """The device address of the 32-byte block {uint64 rows, rows_clipped; double adv_mean, adv_std}."""
        from . import surrogate
        p = C.c_void_p()
        check(surrogate.lib().fi_surrogate_stats_dev(self._h, C.byref(p)), "fi_surrogate_stats_dev")
        return int(p.value)

    # --- the target network (include/fi_target.h; the rule: freeimpala_amd/target.py)
    def enable_target(self, period: int = 4, tau: float = 1.0) -> None:
        """A slowly moving copy theta- of the parameters: a surrogate step takes V-trace's importance weights
        against it and its trust region around it (IMPACT); every ``period``-th update moves theta- by ``tau``
        towards the parameters (1.0: a copy). The first call copies the parameters; a later one replaces the two
        numbers. Between any two steps."""
        from . import target
        prm = target.params(period, tau)
        check(target.lib().fi_target_enable(self._h, C.byref(prm)), "fi_target_enable")

    def disable_target(self) -> None:
        """The next step is the plain surrogate (or V-trace) step again, bit for bit; theta- stays as it is."""
        from . import target
        check(target.lib().fi_target_disable(self._h), "fi_target_disable")

    def sync_target(self) -> None:
        """Enqueue theta- <- parameters now: after ``set_params`` / ``load_state``, which do not touch theta-."""
        from . import target
        check(target.lib().fi_target_sync(self._h), "fi_target_sync")

    def target_state(self) -> dict:
        """Wait for the stream and return enabled, period, tau and the block: updates, rows, mean_log_r,
        mean_sq_log_r of the last target step."""
        from . import target
        prm, st, on = target.TargetParams(), target.TargetStats(), C.c_uint32()
        check(target.lib().fi_target_get_state(self._h, C.byref(prm), C.byref(st), C.byref(on)), "fi_target_get_state")
        return dict(enabled=bool(on.value), period=int(prm.period), tau=float(prm.tau), **st.as_dict())

    def target_params(self) -> np.ndarray:
        """theta- as fp32 (waits for the stream). Not part of ``save_state``: a checkpoint keeps it beside the blob,
        and a resuming process calls ``enable_target``, ``set_target_params``, ``load_state``."""
        from . import target
        out = np.empty(self.param_count, np.float32)
        check(target.lib().fi_target_get_params(self._h, out.ctypes.data, out.size), "fi_target_get_params")
        return out

    def set_target_params(self, p: np.ndarray) -> None:
        from . import target
        a = np.ascontiguousarray(p, np.float32).reshape(-1)
        check(target.lib().fi_target_set_params(self._h, a.ctypes.data, a.size), "fi_target_set_params")

    def _target_ptr(self, name: str) -> int:
        from . import target
        p = C.c_void_p()
        check(getattr(target.lib(), name)(self._h, C.byref(p)), name)
        return int(p.value)

    def target_params_dev(self) -> int:
        """The device address of theta- (fp32, ``param_count`` floats): what an evaluation actor reads through
        ``set_params_ptr``."""
        return self._target_ptr("fi_target_params_dev")

    def target_logits_dev(self) -> int:
        """The device address of the target logits (T + 1, B, A) of the last target step."""
        return self._target_ptr("fi_target_logits_dev")

    def target_stats_dev(self) -> int:
        """The device address of the 32-byte block {uint64 updates, rows; double mean_log_r, mean_sq_log_r}."""
        return self._target_ptr("fi_target_stats_dev")

    # --- the adaptive KL penalty (include/fi_kl.h; the rule: freeimpala_amd/kl.py)
    def enable_kl_penalty(self, reference: str = "behaviour", coeff: float = 1.0, kl_target: float = 0.01,
                          adapt: bool = True, band: float = 1.5, factor: float = 2.0, coeff_min: float = 2.0 ** -20,
                          coeff_max: float = 2.0 ** 20) -> None:
        """Add coeff * KL(q || pi) to the loss, q the batch's behaviour policy ("behaviour") or the target network's
        policy of the batch ("target": penalised are the surrogate steps that run a target forward). With ``adapt``
        the coefficient doubles (``factor``) when a step's mean KL passes ``band * kl_target`` and halves below
        ``kl_target / band``, on the device. A second call replaces the parameters and keeps the coefficient."""
        from . import kl
        if reference not in kl.REFERENCES:
            raise ValueError(f"reference {reference!r}: one of {sorted(kl.REFERENCES)}")
        prm = kl.params(reference, adapt, coeff, kl_target, band, factor, coeff_min, coeff_max)
        check(kl.lib().fi_kl_enable(self._h, C.byref(prm)), "fi_kl_enable")

    def disable_kl_penalty(self) -> None:
        """The next step is the step without the penalty again, bit for bit; the block stays as it is."""
        from . import kl
        check(kl.lib().fi_kl_disable(self._h), "fi_kl_disable")

    def set_kl_coeff(self, c: float) -> None:
        """The coefficient <- c, behind the steps already enqueued (a resuming process: enable, this, load_state)."""
        from . import kl
        check(kl.lib().fi_kl_set_coeff(self._h, c), "fi_kl_set_coeff")

    def kl_state(self) -> dict:
        """Wait for the stream and return the parameters (reference, adapt, kl_target, band, factor, coeff_min,
        coeff_max), enabled and the block: coeff, mean_kl, kl_sum, rows, updates, raised, lowered."""
        from . import kl
        prm, st, on = kl.KlParams(), kl.KlStats(), C.c_uint32()
        check(kl.lib().fi_kl_get_state(self._h, C.byref(prm), C.byref(st), C.byref(on)), "fi_kl_get_state")
        return dict(enabled=bool(on.value), **prm.as_dict(), **st.as_dict())

    def kl_state_dev(self) -> int:
        """The device address of the 48-byte block (freeimpala_amd.kl.unpack_state reads its bytes)."""
        from . import kl
        p = C.c_void_p()
        check(kl.lib().fi_kl_state_dev(self._h, C.byref(p)), "fi_kl_state_dev")
        return int(p.value)

    # --- parameters published on the device (include/fi_publish.h)
    def publish(self) -> int:
        """Enqueue a publication of the parameters as they are at this point of the learner's stream
        (the published form: ``publish.round_params``); nothing waits. Returns the tag: the count of
        updates enqueued so far. ``actor.set_params_dev(learner)`` takes it."""
        from . import publish
        tag = C.c_uint64(0)
        check(publish.lib().fi_publish_params(self._h, C.byref(tag)), "fi_publish_params")
        return tag.value

    def publish_state(self) -> dict:
        """fi_publish_get_state as a dict: publications, slot, tag, version (exact: waits), dtype and
        the readers recorded against each slot."""
        from . import publish
        st = publish.PublishState()
        check(publish.lib().fi_publish_get_state(self._h, C.byref(st)), "fi_publish_get_state")
        return st.as_dict()

    def published(self) -> tuple[np.ndarray, int]:
        """(the newest snapshot as fp32, its exact version); waits for the publication."""
        from . import publish
        out = np.empty(self.param_count, np.float32)
        ver = C.c_uint64(0)
        check(publish.lib().fi_publish_read(self._h, out.ctypes.data, out.size, C.byref(ver)), "fi_publish_read")
        return out, ver.value

    @property
    def publish_event(self) -> int | None:
        """The newest publication's hipEvent_t, None before the first."""
        from . import publish
        return publish.lib().fi_publish_event(self._h)

    # --- off-policy diagnostics of the most recent step (include/fi_diag.h; the rule: freeimpala_amd/diag.py)
    def enqueue_diagnostics(self) -> None:
        """Enqueue the diagnostics of the most recently enqueued step behind it on the learner's stream,
        with the handle's thresholds; nothing waits. Steps enqueued afterwards do not disturb it."""
        from . import diag
        check(diag.lib().fi_diag_enqueue(self._h), "fi_diag_enqueue")

    def _diag_call(self, fn, name: str, columns: bool) -> dict:
        from . import diag
        d = diag.OffPolicyDiag()
        kl = np.empty(self.B, np.float32) if columns else None
        lr = np.empty(self.B, np.float32) if columns else None
        check(fn(self._h, C.byref(d), kl.ctypes.data if columns else None, lr.ctypes.data if columns else None, self.B),
              name)
        out = d.as_dict()
        if columns:
            out["col_kl"], out["col_log_rho"] = kl, lr
        return out

    def read_diagnostics(self, columns: bool = False) -> dict:
        """Wait for the last ``enqueue_diagnostics`` alone and return its summary as a dict (the fields of
        fi_offpolicy_diag); columns=True adds ``col_kl`` and ``col_log_rho``, (B,) float32."""
        from . import diag
        return self._diag_call(diag.lib().fi_diag_read, "fi_diag_read", columns)

    def diagnostics(self, columns: bool = False) -> dict:
        """``enqueue_diagnostics`` and ``read_diagnostics`` in one call."""
        from . import diag
        return self._diag_call(diag.lib().fi_diag_learner, "fi_diag_learner", columns)

    def step_segments_dev(self, segments, stats: bool = True) -> dict:
        """Step from segments of entries in device memory: (ptr, stride, n, event) tuples whose n sum
        to the batch; segment k fills the next n columns once its event (or None) has completed."""
        from . import gather
        st = _abi.StepStats()
        check(gather.lib().fi_learner_step_segments_dev(self._h, gather.segment_array(segments), len(segments),
                                                        C.byref(st) if stats else None),
              "fi_learner_step_segments_dev")
        return st.as_dict() if stats else {}

    @property
    def batch_versions(self) -> dict:
        """dict(min, max, mean, count) of the parameter versions (the records' flags words) in the
        batch of the last step_rollouts / step_segments_dev."""
        from . import gather
        bv = gather.BatchVersions()
        check(gather.lib().fi_learner_batch_versions(self._h, C.byref(bv)), "fi_learner_batch_versions")
        return bv.as_dict()

    def synth(self, seed: int = 42, b_global: int = 0, b_offset: int = 0) -> None:
        check(lib().fi_learner_synth_batch(self._h, seed, b_global, b_offset), "synth")

    def sync(self) -> None:
        check(lib().fi_learner_sync(self._h), "sync")

    @property
    def stream(self) -> int:
        return lib().fi_learner_stream(self._h)

    # --- params
    def get_params(self) -> np.ndarray:
        out = np.empty(self.param_count, np.float32)
        check(lib().fi_learner_get_params_fp32(self._h, out.ctypes.data, out.size), "get_params")
        return out

    def get_blob(self) -> tuple[bytes, int]:
        buf = (C.c_char * self.param_bytes)()
        ver = C.c_uint64(0)
        check(lib().fi_learner_get_params(self._h, buf, self.param_bytes, C.byref(ver)),
              "get_params")
        return bytes(buf), ver.value

    def set_params(self, p: np.ndarray | bytes, version: int = 0) -> None:
        a = np.frombuffer(p, np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p)
        check(lib().fi_learner_set_params(self._h, a.ctypes.data, a.nbytes, version), "set_params")

    # --- tensors
    def tensor_ptr(self, name: str) -> tuple[int, int]:
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib().fi_learner_tensor(self._h, name.encode(), C.byref(p), C.byref(n)), name)
        return p.value, n.value

    def tensor(self, name: str, dtype=np.float32, shape=None) -> np.ndarray:
        p, n = self.tensor_ptr(name)
        self.sync()
        a = hip.download_ptr(p, dtype, (n // np.dtype(dtype).itemsize,))
        return a.reshape(shape) if shape is not None else a

    def upload(self, name: str, a: np.ndarray) -> None:
        p, n = self.tensor_ptr(name)
        assert np.ascontiguousarray(a).nbytes == n, (name, a.nbytes, n)
        self.sync()
        hip.upload_ptr(p, a)

    def replay_vtrace(self, n: int = 20, sets: int = 1) -> float:
        """Mean device ms of the fused V-trace kernel alone: n back-to-back launches of
        fi_vtrace_loss_fp32 (no loss finalisation), HIP events around the burst.

        sets = 1: every launch reads this learner's resident tensors (~100 MB at T=100,
        B=4096), which stay in the 256 MB Infinity Cache between launches -- a WARM figure.
        sets = k > 1: launches rotate over k disjoint copies of the inputs and outputs
        (k x ~100 MB, > 256 MB for k >= 3), so each launch finds its tensors evicted by the
        k-1 launches before it -- the COLD (HBM) figure. Inputs are read-only and the
        learner's own outputs are rewritten with identical values: its state is unchanged."""
        T, B, A = self.T, self.B, self.A
        names = ("logits", "mu", "actions", "rewards", "discounts", "values", "vs", "pg_adv",
                 "dlogits", "dvalue")
        base = {k: self.tensor_ptr(k) for k in names}
        hp = self.cfg.hp
        wsb = lib().fi_vtrace_workspace_bytes(T, B, A)
        stream = self.stream
        self.sync()
        owned = []
        sets_ptr = [{k: v[0] for k, v in base.items()}]
        for _ in range(1, max(1, sets)):
            d = {}
            for k, (ptr, nb) in base.items():
                buf = hip.DeviceBuffer(nb)
                hip.copy_d2d(buf.ptr, ptr, nb)
                owned.append(buf)
                d[k] = buf.ptr
            sets_ptr.append(d)
        ws = [hip.DeviceBuffer(wsb) for _ in sets_ptr]

        def launch(i):
            ptr, w = sets_ptr[i % len(sets_ptr)], ws[i % len(sets_ptr)]
            check(lib().fi_vtrace_loss_fp32(
                T, B, A, ptr["logits"], ptr["mu"], ptr["actions"], ptr["rewards"], ptr["discounts"],
                ptr["values"], C.byref(hp), ptr["vs"], ptr["pg_adv"], ptr["dlogits"], ptr["dvalue"],
                None, w.ptr, wsb, stream), "fi_vtrace_loss_fp32")

        for i in range(max(3, len(sets_ptr))):
            launch(i)
        e0, e1 = hip.Event(), hip.Event()
        e0.record(stream)
        for i in range(n):
            launch(i)
        e1.record(stream)
        self.sync()
        ms = e0.elapsed_ms(e1) / n
        for b in owned + ws:
            b.free()
        return ms

    # --- data parallel
    @staticmethod
    def comm_unique_id() -> bytes:
        n = lib().fi_comm_unique_id_bytes()
        buf = (C.c_char * n)()
        check(lib().fi_comm_get_unique_id(buf, n), "comm_unique_id")
        return bytes(buf)

    def attach_comm(self, uid: bytes, rank: int, nranks: int) -> None:
        check(lib().fi_learner_attach_comm(self._h, uid, len(uid), rank, nranks), "attach_comm")

    def comm_info(self) -> dict:
        """RCCL's view of this handle's communicator and the gradient buckets of its last step."""
        n, r, b = C.c_int(), C.c_int(), C.c_int()
        check(lib().fi_learner_comm_info(self._h, C.byref(n), C.byref(r), C.byref(b)), "comm_info")
        return {"nranks": n.value, "rank": r.value, "buckets_last_step": b.value}

    @staticmethod
    def comm_init_all(learners) -> None:
        """One process, several devices: all handles join one communicator (rank = list index)."""
        arr = (C.c_void_p * len(learners))(*[x._h for x in learners])
        check(lib().fi_comm_init_all(arr, len(learners)), "comm_init_all")

    # --- profiling
    def set_profiling(self, on: bool) -> None:
        check(lib().fi_learner_set_profiling(self._h, int(on)), "set_profiling")

    def phase_times(self) -> dict:
        ms = (C.c_float * len(_abi.PHASES))()
        n = C.c_int(0)
        check(lib().fi_learner_phase_times(self._h, ms, len(_abi.PHASES), C.byref(n)), "phases")
        d = dict(zip(_abi.PHASES, list(ms)))
        d["steps"] = n.value
        return d

    def close(self) -> None:
        if self._h:
            lib().fi_learner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_records(obs, mu, actions, rewards, discounts, entry_size=None) -> list[bytes]:
    """Build SharedBuffer entries from time-major arrays (inverse of the ingest kernel).
    obs (T+1,B,D), mu (T,B,A), actions/rewards/discounts (T,B). Returns B entries of
    entry_size*1024 bytes (default T+1 elements)."""
    T1, B, D = obs.shape
    T = T1 - 1
    A = mu.shape[-1]
    S = entry_size or T1
    out = []
    for b in range(B):
        e = np.zeros((S, 1024), np.uint8)
        rec = e[:T1]
        rec[:, 0:4 * D] = np.ascontiguousarray(obs[:, b, :], np.float32).view(np.uint8)
        rec[:T, 512:512 + 4 * A] = np.ascontiguousarray(mu[:, b, :], np.float32).view(np.uint8)
        rec[:T, 768:772] = np.ascontiguousarray(actions[:, b], np.int32).view(np.uint8).reshape(T, 4)
        rec[:T, 772:776] = np.ascontiguousarray(rewards[:, b], np.float32).view(np.uint8).reshape(T, 4)
        rec[:T, 776:780] = np.ascontiguousarray(discounts[:, b], np.float32).view(np.uint8).reshape(T, 4)
        out.append(e.tobytes())
    return out


def pack_atari_records(frames, mu, actions, rewards, discounts, entry_size=None) -> list[bytes]:
    """Build SharedBuffer entries of Atari records from time-major arrays (inverse of the Atari
    ingest kernel). frames (T+1,B,84,84,4) uint8, mu (T,B,A), actions/rewards/discounts (T,B).
    Returns B entries of entry_size*1024 bytes (entry_size in 1 KiB elements, default
    28*(T+1)); record T carries the bootstrap frame only."""
    frames = np.asarray(frames, np.uint8)
    T1, B = frames.shape[:2]
    T = T1 - 1
    A = mu.shape[-1]
    R, FB = _abi.ATARI_RECORD_BYTES, _abi.ATARI_FRAME_BYTES
    S = entry_size or _abi.ATARI_RECORD_ELEMENTS * T1
    if S * 1024 < T1 * R:
        raise ValueError(f"entry_size {S} < {_abi.ATARI_RECORD_ELEMENTS * T1} = 28*(T+1)")
    fr = frames.reshape(T1, B, FB)
    out = []
    for b in range(B):
        e = np.zeros(S * 1024, np.uint8)
        rec = e[:T1 * R].reshape(T1, R)
        rec[:, :FB] = fr[:, b]
        h = rec[:T]
        h[:, _abi.ATARI_REC_MU:_abi.ATARI_REC_MU + 4 * A] = \
            np.ascontiguousarray(mu[:, b, :], np.float32).view(np.uint8).reshape(T, 4 * A)
        for off, a, dt in ((_abi.ATARI_REC_ACT, actions, np.int32), (_abi.ATARI_REC_REW, rewards, np.float32),
                           (_abi.ATARI_REC_DISC, discounts, np.float32)):
            h[:, off:off + 4] = np.ascontiguousarray(a[:, b], dt).view(np.uint8).reshape(T, 4)
        out.append(e.tobytes())
    return out


def unpack_atari_records(batch_bytes, T, B, A):
    """Inverse of pack_atari_records: B entries (a sequence of byte strings / uint8 arrays of
    equal length, or one buffer holding them back to back) -> (frames (T+1,B,84,84,4) uint8,
    mu (T,B,A) float32, actions (T,B) int32, rewards (T,B), discounts (T,B) float32)."""
    if isinstance(batch_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        buf = np.frombuffer(batch_bytes, np.uint8) if not isinstance(batch_bytes, np.ndarray) \
            else np.ascontiguousarray(batch_bytes).view(np.uint8).ravel()
    else:
        buf = np.concatenate([np.frombuffer(e, np.uint8) if not isinstance(e, np.ndarray)
                              else np.ascontiguousarray(e).view(np.uint8).ravel() for e in batch_bytes])
    R, FB = _abi.ATARI_RECORD_BYTES, _abi.ATARI_FRAME_BYTES
    if buf.size % B or buf.size // B < (T + 1) * R:
        raise ValueError(f"{buf.size} bytes do not hold {B} entries of >= {(T + 1) * R} bytes")
    rec = buf.reshape(B, -1)[:, :(T + 1) * R].reshape(B, T + 1, R)
    frames = np.ascontiguousarray(rec[:, :, :FB].transpose(1, 0, 2)).reshape(T + 1, B, 84, 84, 4)
    h = rec[:, :T]

    def field(off, n, dt):
        return np.ascontiguousarray(h[:, :, off:off + 4 * n].transpose(1, 0, 2)).view(dt)

    mu = field(_abi.ATARI_REC_MU, A, np.float32)
    act = field(_abi.ATARI_REC_ACT, 1, np.int32)[..., 0]
    rew = field(_abi.ATARI_REC_REW, 1, np.float32)[..., 0]
    disc = field(_abi.ATARI_REC_DISC, 1, np.float32)[..., 0]
    return frames, mu, np.ascontiguousarray(act), np.ascontiguousarray(rew), np.ascontiguousarray(disc)


def _u8_rows(batch_bytes, B):
    if isinstance(batch_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        buf = np.frombuffer(batch_bytes, np.uint8) if not isinstance(batch_bytes, np.ndarray) \
            else np.ascontiguousarray(batch_bytes).view(np.uint8).ravel()
    else:
        buf = np.concatenate([np.frombuffer(e, np.uint8) if not isinstance(e, np.ndarray)
                              else np.ascontiguousarray(e).view(np.uint8).ravel() for e in batch_bytes])
    if buf.size % B:
        raise ValueError(f"{buf.size} bytes are not {B} entries of equal length")
    return buf.reshape(B, -1)


def plane_entry_elements(T: int) -> int:
    """--entry-size of a plane-record entry: 7 per record, T+1 records, the 21-element history."""
    return _abi.ATARI_PLANE_RECORD_ELEMENTS * (T + 1) + _abi.ATARI_HISTORY_ELEMENTS


def pack_atari_plane_records(planes, history, episode_start, mu, actions, rewards, discounts,
                             entry_size=None) -> list[bytes]:
    """Build SharedBuffer entries of single-plane Atari records (inverse of the planes ingest's
    header and plane reads). planes (T+1,B,84,84) uint8: the newest observation of every step;
    history (3,B,84,84) uint8: the planes preceding record 0, oldest first; episode_start (T+1,B)
    bool; mu (T,B,A<=18), actions/rewards/discounts (T,B). Returns B entries of entry_size*1024
    bytes (default 7*(T+1)+21): T+1 records, then the history block at (T+1)*7168."""
    planes = np.asarray(planes, np.uint8)
    T1, B = planes.shape[:2]
    T = T1 - 1
    A = mu.shape[-1]
    if A > _abi.ATARI_PLANE_MAX_ACTIONS:
        raise ValueError(f"the plane record's header holds mu[18]: A = {A}")
    R, PB = _abi.ATARI_PLANE_RECORD_BYTES, _abi.ATARI_PLANE_BYTES
    S = entry_size or plane_entry_elements(T)
    if S < plane_entry_elements(T):
        raise ValueError(f"entry_size {S} < {plane_entry_elements(T)} = 7*(T+1)+21")
    pl = planes.reshape(T1, B, PB)
    hi = np.asarray(history, np.uint8).reshape(3, B, PB)
    es = np.asarray(episode_start).reshape(T1, B) != 0
    out = []
    for b in range(B):
        e = np.zeros(S * 1024, np.uint8)
        rec = e[:T1 * R].reshape(T1, R)
        rec[:, :PB] = pl[:, b]
        rec[:, _abi.PLANE_REC_START:_abi.PLANE_REC_START + 4] = es[:, b].astype(np.uint32).view(np.uint8).reshape(T1, 4)
        h = rec[:T]
        h[:, _abi.PLANE_REC_MU:_abi.PLANE_REC_MU + 4 * A] = \
            np.ascontiguousarray(mu[:, b, :], np.float32).view(np.uint8).reshape(T, 4 * A)
        for off, a, dt in ((_abi.PLANE_REC_ACT, actions, np.int32), (_abi.PLANE_REC_REW, rewards, np.float32),
                           (_abi.PLANE_REC_DISC, discounts, np.float32)):
            h[:, off:off + 4] = np.ascontiguousarray(a[:, b], dt).view(np.uint8).reshape(T, 4)
        e[T1 * R:T1 * R + 3 * PB] = hi[:, b].reshape(-1)
        out.append(e.tobytes())
    return out


def unpack_atari_plane_records(batch_bytes, T, B, A):
    """Inverse of pack_atari_plane_records: B entries (a sequence, or one buffer holding them back
    to back) -> (planes (T+1,B,84,84) uint8, history (3,B,84,84) uint8, episode_start (T+1,B) bool,
    mu (T,B,A) float32, actions (T,B) int32, rewards (T,B), discounts (T,B) float32)."""
    rows = _u8_rows(batch_bytes, B)
    R, PB = _abi.ATARI_PLANE_RECORD_BYTES, _abi.ATARI_PLANE_BYTES
    need = (T + 1) * R + _abi.ATARI_HISTORY_BYTES
    if rows.shape[1] < need:
        raise ValueError(f"{rows.size} bytes do not hold {B} entries of >= {need} bytes")
    rec = rows[:, :(T + 1) * R].reshape(B, T + 1, R)
    planes = np.ascontiguousarray(rec[:, :, :PB].transpose(1, 0, 2)).reshape(T + 1, B, 84, 84)
    history = np.ascontiguousarray(
        rows[:, (T + 1) * R:(T + 1) * R + 3 * PB].reshape(B, 3, PB).transpose(1, 0, 2)).reshape(3, B, 84, 84)

    def field(r, off, n, dt):
        return np.ascontiguousarray(r[:, :, off:off + 4 * n].transpose(1, 0, 2)).view(dt)

    start = field(rec, _abi.PLANE_REC_START, 1, np.uint32)[..., 0] != 0
    h = rec[:, :T]
    mu = field(h, _abi.PLANE_REC_MU, A, np.float32)
    act = field(h, _abi.PLANE_REC_ACT, 1, np.int32)[..., 0]
    rew = field(h, _abi.PLANE_REC_REW, 1, np.float32)[..., 0]
    disc = field(h, _abi.PLANE_REC_DISC, 1, np.float32)[..., 0]
    return (planes, history, start, mu, np.ascontiguousarray(act), np.ascontiguousarray(rew),
            np.ascontiguousarray(disc))


def stack_planes(planes, history, episode_start) -> np.ndarray:
    """The frame-stack wrapper, step by step: frames (T+1,B,84,84,4) uint8 from planes
    (T+1,B,84,84), history (3,B,84,84; oldest first) and episode_start (T+1,B). A four-deep
    window per entry slides one plane per step; the first observation of an episode fills the
    whole window. Channel 3 is the newest plane."""
    planes = np.asarray(planes, np.uint8)
    history = np.asarray(history, np.uint8)
    start = np.asarray(episode_start) != 0
    T1, B = planes.shape[:2]
    frames = np.empty((T1, B, 84, 84, 4), np.uint8)
    for b in range(B):
        window = [history[0, b], history[1, b], history[2, b], None]
        for t in range(T1):
            if start[t, b]:
                window = [planes[t, b]] * 4
            else:
                window[3] = planes[t, b]
            for c in range(4):
                frames[t, b, :, :, c] = window[c]
            window = window[1:] + [None]
    return frames
