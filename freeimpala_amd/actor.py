"""Host side of batched policy inference with action sampling (include/fi_actor.h).

An ``Actor`` evaluates the policy a learner publishes on ``num_envs`` environments per call and
draws their actions on the device:

  a = Actor("atari", num_envs=256, num_actions=6)
  a.set_params(blob, version)                 # the bytes of DeviceLearner.get_blob() / get_params()
  out = a.act_planes(planes, episode_start)   # dict(actions (N,), logits (N, A), values (N,))

The logits returned are the policy's own: they are what an actor writes into a record's mu field,
unless exploration is set (``set_exploration``, include/fi_explore.h): then the draw has a temperature
and per-environment epsilons, the dicts gain ``behaviour_logits`` and those go into mu.
An Atari handle keeps every environment's 4-frame stack on the device (``act_planes`` sends one
84x84 plane per environment; ``stacks()`` reads them back); ``act_frames`` takes whole stacks.
Everything runs in HIP kernels of libfi_learner.so; there is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

FI_ACT_SAMPLE, FI_ACT_GREEDY = 0, 1
FI_ERR_STATE, FI_ERR_NONFINITE = -4, -7  # include/fi_learner.h
MODES = {"sample": FI_ACT_SAMPLE, "greedy": FI_ACT_GREEDY}
PHASES = ["h2d", "push", "forward", "sample", "d2h"]
PLANE_BYTES = 84 * 84
STACK_BYTES = 4 * PLANE_BYTES


class ActorConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("arch", C.c_int32), ("num_envs", C.c_int32),
                ("num_actions", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32),
                ("device", C.c_int32), ("mode", C.c_int32), ("seed", C.c_uint64)]


_P = C.c_void_p
SIGNATURES = {  # every symbol include/fi_actor.h declares
    "fi_actor_config_init": ([C.POINTER(ActorConfig)], None),
    "fi_actor_create": ([C.POINTER(ActorConfig), C.POINTER(_P)], C.c_int),
    "fi_actor_destroy": ([_P], None),
    "fi_actor_param_count": ([_P], C.c_size_t),
    "fi_actor_set_params": ([_P, _P, C.c_size_t, C.c_uint64], C.c_int),
    "fi_actor_version": ([_P], C.c_uint64),
    "fi_actor_set_mode": ([_P, C.c_int], C.c_int),
    "fi_actor_seed": ([_P, C.c_uint64, C.c_uint64], C.c_int),
    "fi_actor_act_obs": ([_P, _P, _P, _P, _P], C.c_int),
    "fi_actor_act_frames": ([_P, _P, _P, _P, _P], C.c_int),
    "fi_actor_act_planes": ([_P, _P, _P, _P, _P, _P], C.c_int),
    "fi_actor_reset_stacks": ([_P], C.c_int),
    "fi_actor_read_stacks": ([_P, _P, C.c_size_t], C.c_int),
    "fi_actor_set_profiling": ([_P, C.c_int], C.c_int),
    "fi_actor_phase_times": ([_P, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)], C.c_int),
    "fi_push_planes": ([_P, _P, _P, C.c_int, _P], C.c_int),
    "fi_sample_actions": ([_P, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _P, _P, _P], C.c_int),
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


def _mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode: sample | greedy, not {mode!r}")
        return MODES[mode]
    return int(mode)


class Actor:
    def __init__(self, arch: str = "mlp", num_envs: int = 1, num_actions: int = 18, obs_dim: int = 128,
                 hidden: int = 256, mode: str = "sample", seed: int = 0, device: int = 0):
        if arch not in ("mlp", "atari"):
            raise ValueError(f"arch: mlp | atari, not {arch!r}")
        cfg = ActorConfig()
        lib().fi_actor_config_init(C.byref(cfg))
        cfg.arch = _abi.FI_ARCH_MLP if arch == "mlp" else _abi.FI_ARCH_ATARI
        cfg.num_envs, cfg.num_actions, cfg.obs_dim, cfg.hidden = num_envs, num_actions, obs_dim, hidden
        cfg.device, cfg.mode, cfg.seed = device, _mode(mode), seed
        self._h = _P()
        check(lib().fi_actor_create(C.byref(cfg), C.byref(self._h)), "fi_actor_create")
        self.arch, self.N, self.A, self.D, self.H = arch, num_envs, num_actions, obs_dim, hidden
        self._explore_used = False  # set_exploration was called: act calls look for behaviour logits

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().fi_actor_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- parameters
    @property
    def param_count(self) -> int:
        return int(lib().fi_actor_param_count(self._h))

    def set_params(self, p: np.ndarray | bytes, version: int = 0) -> None:
        """The published blob (bytes: fp32 or bf16) or an fp32 array of param_count values."""
        a = np.frombuffer(p, np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p)
        check(lib().fi_actor_set_params(self._h, a.ctypes.data, a.nbytes, version), "fi_actor_set_params")

    # --- parameters from device memory, in stream order (include/fi_publish.h)
    def set_params_dev(self, learner) -> None:
        """The learner's newest publication (``learner.publish()``), enqueued on this handle's stream:
        no host copy, no wait. ``version`` becomes the publication's tag. May be called on this
        actor's thread while another thread drives the learner."""
        from . import publish
        check(publish.lib().fi_actor_set_params_dev(self._h, learner._h), "fi_actor_set_params_dev")

    def set_params_ptr(self, params_ptr: int, count: int, version: int = 0, ready_event=None) -> int | None:
        """``count`` fp32 parameters from device memory, behind ``ready_event``; returns the handle's
        "params read" event, recorded behind the copy."""
        from . import publish
        ev = _P()
        check(publish.lib().fi_actor_set_params_ptr(self._h, params_ptr, count, version, ready_event, C.byref(ev)),
              "fi_actor_set_params_ptr")
        return ev.value

    def read_params(self) -> np.ndarray:
        """Waits for the stream: the handle's fp32 parameters."""
        from . import publish
        out = np.empty(self.param_count, np.float32)
        check(publish.lib().fi_actor_read_params(self._h, out.ctypes.data, out.size), "fi_actor_read_params")
        return out

    @property
    def version(self) -> int:
        return int(lib().fi_actor_version(self._h))

    def set_mode(self, mode) -> None:
        check(lib().fi_actor_set_mode(self._h, _mode(mode)), "fi_actor_set_mode")

    def seed(self, seed: int, draw: int = 0) -> None:
        """Key of the action draws and the index the next act call uses."""
        check(lib().fi_actor_seed(self._h, seed, draw), "fi_actor_seed")

    # --- acting
    def _outputs(self):
        return (np.empty(self.N, np.int32), np.empty((self.N, self.A), np.float32), np.empty(self.N, np.float32))

    def _input(self, a, dtype, shape, what):
        a = np.ascontiguousarray(a, dtype)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{what}: {a.shape} does not hold {shape}")
        return a

    def _finish(self, rc, what, out):
        """A call that reports NaN / Inf rows has still filled its outputs: they ride on the error."""
        err = None
        try:
            check(rc, what)  # first: it reads fi_last_error(), which the probe below may overwrite
        except _abi.FiError as e:
            err = e
        if rc in (_abi.FI_OK, FI_ERR_NONFINITE):
            mu = self._behaviour()
            if mu is not None:
                out["behaviour_logits"] = mu
        if err is not None:
            err.outputs = out
            raise err
        return out

    def act_obs(self, obs) -> dict:
        obs = self._input(obs, np.float32, (self.N, self.D), "obs")
        act, log, val = self._outputs()
        rc = lib().fi_actor_act_obs(self._h, obs.ctypes.data, act.ctypes.data, log.ctypes.data, val.ctypes.data)
        return self._finish(rc, "fi_actor_act_obs", dict(actions=act, logits=log, values=val))

    def act_frames(self, frames) -> dict:
        frames = self._input(frames, np.uint8, (self.N, 84, 84, 4), "frames")
        act, log, val = self._outputs()
        rc = lib().fi_actor_act_frames(self._h, frames.ctypes.data, act.ctypes.data, log.ctypes.data,
                                       val.ctypes.data)
        return self._finish(rc, "fi_actor_act_frames", dict(actions=act, logits=log, values=val))

    def act_planes(self, planes, episode_start) -> dict:
        planes = self._input(planes, np.uint8, (self.N, 84, 84), "planes")
        start = self._input(np.asarray(episode_start) != 0, np.uint8, (self.N,), "episode_start")
        act, log, val = self._outputs()
        rc = lib().fi_actor_act_planes(self._h, planes.ctypes.data, start.ctypes.data, act.ctypes.data,
                                       log.ctypes.data, val.ctypes.data)
        return self._finish(rc, "fi_actor_act_planes", dict(actions=act, logits=log, values=val))

    def reset_stacks(self) -> None:
        check(lib().fi_actor_reset_stacks(self._h), "fi_actor_reset_stacks")

    def stacks(self) -> np.ndarray:
        """The stacks the last act_planes ran the policy on: (N, 84, 84, 4) uint8."""
        out = np.empty((self.N, 84, 84, 4), np.uint8)
        check(lib().fi_actor_read_stacks(self._h, out.ctypes.data, out.nbytes), "fi_actor_read_stacks")
        return out

    # --- rollout recording (include/fi_rollout.h; the rule: freeimpala_amd/rollout.py)
    def begin_rollout(self, T: int) -> None:
        """From here on every act_planes / act_obs call records its step on the device, T steps to
        an unroll; two buffers of N entries are allocated."""
        from . import rollout
        check(rollout.lib().fi_rollout_begin(self._h, T), "fi_rollout_begin")

    def outcome(self, rewards, discounts) -> None:
        """The rewards and discounts (N each) the environments returned for the last act call's actions."""
        from . import rollout
        rew = self._input(rewards, np.float32, (self.N,), "rewards")
        disc = self._input(discounts, np.float32, (self.N,), "discounts")
        check(rollout.lib().fi_rollout_outcome(self._h, rew.ctypes.data, disc.ctypes.data), "fi_rollout_outcome")

    def rollout_ready(self) -> bool:
        from . import rollout
        return bool(rollout.lib().fi_rollout_ready(self._h))

    @property
    def rollout_entry_bytes(self) -> int:
        from . import rollout
        return int(rollout.lib().fi_rollout_entry_bytes(self._h))

    def acquire_rollout(self) -> tuple[int, int, int]:
        """(device pointer, entry stride, ready event) of the completed unroll."""
        from . import rollout
        ptr, stride, ev = _P(), C.c_size_t(), _P()
        check(rollout.lib().fi_rollout_acquire(self._h, C.byref(ptr), C.byref(stride), C.byref(ev)),
              "fi_rollout_acquire")
        return ptr.value, stride.value, ev.value

    def release_rollout(self, consumed_event=None) -> None:
        from . import rollout
        check(rollout.lib().fi_rollout_release(self._h, consumed_event), "fi_rollout_release")

    def read_rollout(self) -> np.ndarray:
        """The completed unroll's entries, (N, entry_bytes) uint8; it stays unreleased."""
        from . import rollout
        out = np.empty((self.N, self.rollout_entry_bytes), np.uint8)
        check(rollout.lib().fi_rollout_read(self._h, out.ctypes.data, out.nbytes), "fi_rollout_read")
        return out

    def end_rollout(self) -> None:
        from . import rollout
        check(rollout.lib().fi_rollout_end(self._h), "fi_rollout_end")

    # --- device pointers in, nothing waits (include/fi_env.h). Pointers and events travel as ints.
    def act_planes_dev(self, planes_ptr: int, episode_start_ptr: int, ready_event=None) -> None:
        """Enqueue an act call on N*7056 plane bytes and N start flags in device memory."""
        from . import env
        check(env.lib().fi_actor_act_planes_dev(self._h, planes_ptr, episode_start_ptr, ready_event),
              "fi_actor_act_planes_dev")

    def act_obs_dev(self, obs_ptr: int, ready_event=None) -> None:
        """Enqueue an act call on N*obs_dim floats in device memory (MLP)."""
        from . import env
        check(env.lib().fi_actor_act_obs_dev(self._h, obs_ptr, ready_event), "fi_actor_act_obs_dev")

    def outputs_dev(self) -> dict:
        """Device pointers of the handle's actions int32[N], logits float[N*A], values float[N] and
        the event behind the last device call (None before the first)."""
        from . import env
        p = [_P() for _ in range(4)]
        check(env.lib().fi_actor_outputs_dev(self._h, *[C.byref(x) for x in p]), "fi_actor_outputs_dev")
        return dict(zip(("actions", "logits", "values", "done_event"), [x.value for x in p]))

    def read_outputs(self) -> dict:
        """Waits for the stream and copies the last act call's outputs to the host."""
        from . import hip
        self.sync()
        o = self.outputs_dev()
        out = dict(actions=hip.download_ptr(o["actions"], np.int32, (self.N,)),
                   logits=hip.download_ptr(o["logits"], np.float32, (self.N, self.A)),
                   values=hip.download_ptr(o["values"], np.float32, (self.N,)))
        mu = self._behaviour()
        if mu is not None:
            out["behaviour_logits"] = mu
        return out

    # --- exploration (include/fi_explore.h; the rule: freeimpala_amd/explore.py)
    def set_exploration(self, temperature: float = 1.0, epsilon=None) -> None:
        """Draw with a temperature and epsilon (None: 0, a scalar, or N values); the behaviour logits
        go into the records' mu. Allowed between any two act calls. temperature 1 with every epsilon
        0 is ``clear_exploration``. Greedy mode ignores both."""
        from . import explore
        eps = None
        if epsilon is not None:
            e = np.asarray(epsilon, np.float32)
            if e.ndim > 0 and e.size != self.N:
                raise ValueError(f"epsilon: {e.shape} is neither a scalar nor {self.N} values")
            eps = np.ascontiguousarray(np.broadcast_to(e.reshape(-1) if e.ndim else e, (self.N,)))
        check(explore.lib().fi_explore_set(self._h, temperature, eps.ctypes.data if eps is not None else None),
              "fi_explore_set")
        self._explore_used = True

    def clear_exploration(self) -> None:
        from . import explore
        check(explore.lib().fi_explore_clear(self._h), "fi_explore_clear")

    def exploration(self) -> dict:
        """dict(temperature, epsilon (N,) fp32, active); inactive: temperature 1, epsilon 0."""
        from . import explore
        t, act = C.c_float(0), C.c_int(0)
        eps = np.empty(self.N, np.float32)
        check(explore.lib().fi_explore_get(self._h, C.byref(t), eps.ctypes.data, C.byref(act)), "fi_explore_get")
        return dict(temperature=float(t.value), epsilon=eps, active=bool(act.value))

    def behaviour_ptr(self) -> int:
        """Device pointer of the last act call's behaviour logits float[N*A], behind
        ``outputs_dev()["done_event"]``; FiError (rc = FI_ERR_STATE) unless that call explored."""
        from . import explore
        p = _P()
        check(explore.lib().fi_explore_behaviour_dev(self._h, C.byref(p)), "fi_explore_behaviour_dev")
        return p.value

    def _behaviour(self):
        """The last act call's behaviour logits (waits), or None when it drew by the plain rule."""
        if not self._explore_used or not self.exploration()["active"]:  # fi_explore_get never fails
            return None
        from . import explore
        mu = np.empty((self.N, self.A), np.float32)
        rc = explore.lib().fi_explore_read_behaviour(self._h, mu.ctypes.data, mu.size)
        if rc == FI_ERR_STATE:  # greedy mode, or set since the last act call
            return None
        check(rc, "fi_explore_read_behaviour")
        return mu

    def outcome_dev(self, rewards_ptr: int, discounts_ptr: int, ready_event=None) -> None:
        """``outcome`` from N rewards and N discounts in device memory."""
        from . import env
        check(env.lib().fi_rollout_outcome_dev(self._h, rewards_ptr, discounts_ptr, ready_event),
              "fi_rollout_outcome_dev")

    @property
    def stream(self) -> int | None:
        """The handle's hipStream_t (where the device calls are enqueued)."""
        from . import env
        return env.lib().fi_actor_stream(self._h)

    def sync(self) -> int:
        """Wait for the handle's stream. Rows with NaN / Inf logits in the device act calls since the
        last sync raise FiError (rc = FI_ERR_NONFINITE) with the count in ``nonfinite_rows``."""
        from . import env
        n = C.c_int64(0)
        rc = env.lib().fi_actor_sync(self._h, C.byref(n))
        try:
            check(rc, "fi_actor_sync")
        except _abi.FiError as e:
            e.nonfinite_rows = n.value
            raise
        return n.value

    # --- profiling
    def set_profiling(self, on: bool) -> None:
        check(lib().fi_actor_set_profiling(self._h, int(on)), "fi_actor_set_profiling")

    def phase_times(self) -> dict:
        """Mean device ms per act call since profiling was switched on (or last read), by phase."""
        ms = (C.c_float * len(PHASES))()
        n = C.c_int(0)
        check(lib().fi_actor_phase_times(self._h, ms, len(PHASES), C.byref(n)), "fi_actor_phase_times")
        d = dict(zip(PHASES, [float(x) for x in ms]))
        d["calls"] = n.value
        return d


def push_planes(stacks_ptr: int, planes_ptr: int, start_ptr: int, n: int, stream=None) -> None:
    """fi_push_planes on device pointers."""
    check(lib().fi_push_planes(stacks_ptr, planes_ptr, start_ptr, n, stream), "fi_push_planes")


def sample_actions(logits_ptr: int, n: int, a: int, mode, seed: int, draw: int, actions_ptr: int,
                   nonfinite_ptr: int | None = None, stream=None) -> None:
    """fi_sample_actions on device pointers."""
    check(lib().fi_sample_actions(logits_ptr, n, a, _mode(mode), seed, draw, actions_ptr, nonfinite_ptr, stream),
          "fi_sample_actions")
