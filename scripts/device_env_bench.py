#!/usr/bin/env python3
"""First measurements of the loop with a device-resident environment (include/fi_env.h): one
recording Atari actor, one learner and N = B Catch environments on one device, A = 18, N in
{256, 1024}, T = 20, driven two ways that alternate unroll by unroll in one session:

  host-stepped  per step: planes and start flags D2H -> act_planes from the host -> the actions H2D ->
                fi_env_step -> rewards and discounts D2H -> outcome from the host; the environment
                itself still runs on the device, so the difference is the crossings alone
  rollout       fi_env_rollout(T): the T steps are enqueued on the actor's stream, nothing waits

and DeviceLearner.step_rollout after each unroll. Per N: `--warmup` unrolls of each way, then
`--unrolls` timed ones. Reported per way: wall ms per unroll (everything the caller waits for, the
learner step included; median, min, max) and env-steps/s from the median; the actor's device ms per
step (rollout: HIP events on the actor's stream around one enqueued unroll / T, a pass of its own;
host-stepped: the sum of the act call's profiled phases). For the environment: device ms of a step
(update + render) and of the render alone, by events around `--env-steps` launches, against the
render's store floor N * 7056 B / 6.3 TB/s. Prints one JSON line and writes it to
profiles/device_env_loop.json.

    python scripts/device_env_bench.py [--out profiles/device_env_loop.json] [--unrolls 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, env, hip  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
GAMMA = 0.99


def now() -> float:
    return time.perf_counter()


class Loop:
    def __init__(self, n: int, T: int, A: int, params: np.ndarray, rollout: bool):
        self.n, self.T, self.rollout = n, T, rollout
        self.L = DeviceLearner("atari", seq_len=T, batch=n, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.a = Actor("atari", n, num_actions=A, seed=1)
        self.a.set_params(params)
        self.a.begin_rollout(T)
        self.e = env.CatchEnv(n, GAMMA, seed=1)
        self.t = self.e.tensors()
        self.d_act = hip.DeviceBuffer(n * 4)
        self.steps(1)  # step 0 of the first unroll

    def steps(self, k: int) -> None:
        if self.rollout:
            assert self.e.rollout(self.a, k) == k
            return
        for _ in range(k):
            planes = hip.download_ptr(self.t["planes"], np.uint8, (self.n, 84, 84))
            start = hip.download_ptr(self.t["episode_start"], np.uint8, (self.n,))
            out = self.a.act_planes(planes, start)
            self.d_act.upload(out["actions"])
            self.e.step(self.d_act.ptr)  # the null stream; the copies below follow it
            rew = hip.download_ptr(self.t["rewards"], np.float32, (self.n,))
            disc = hip.download_ptr(self.t["discounts"], np.float32, (self.n,))
            self.a.outcome(rew, disc)

    def unroll(self) -> float:
        """T steps and the learner step of the unroll they complete: wall ms."""
        t0 = now()
        self.steps(self.T)
        self.L.step_rollout(self.a)
        return (now() - t0) * 1e3

    def actor_device_ms_per_step(self) -> float:
        if self.rollout:
            self.a.sync()
            e0, e1 = hip.Event(), hip.Event()
            e0.record(self.a.stream)
            self.steps(self.T)
            e1.record(self.a.stream)
            ms = e0.elapsed_ms(e1) / self.T
        else:
            self.a.set_profiling(True)
            self.steps(self.T)
            ph = self.a.phase_times()
            self.a.set_profiling(False)
            ms = sum(v for k, v in ph.items() if k != "calls")
        self.L.step_rollout(self.a)
        return ms

    def close(self):
        self.a.sync()
        self.a.end_rollout()
        for h in (self.a, self.e, self.L):
            h.close()
        self.d_act.free()


def env_kernel_ms(n: int, launches: int) -> dict:
    """Device ms per environment step (update + render) and per render alone, on the null stream."""
    e = env.CatchEnv(n, GAMMA, seed=2)
    d_act = hip.DeviceBuffer.from_array((np.arange(n) % 3).astype(np.int32))
    state, planes = hip.DeviceBuffer(n * 16), hip.DeviceBuffer(n * 7056)
    state.zero()
    out = {}
    for name, call in (("step", lambda: e.step(d_act.ptr)), ("render", lambda: env.env_render(state.ptr, planes.ptr, n))):
        for _ in range(10):
            call()
        hip.synchronize()
        e0, e1 = hip.Event(), hip.Event()
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        out[name] = e0.elapsed_ms(e1) / launches
    e.close()
    for b in (d_act, state, planes):
        b.free()
    return out


def measure(n: int, T: int, A: int, params: np.ndarray, unrolls: int, warmup: int, env_steps: int) -> dict:
    loops = dict(host_stepped=Loop(n, T, A, params, False), rollout=Loop(n, T, A, params, True))
    for _ in range(warmup):
        for lp in loops.values():
            lp.unroll()
    wall = {k: [] for k in loops}
    for _ in range(unrolls):  # alternating
        for k, lp in loops.items():
            wall[k].append(lp.unroll())
    actor_ms = {k: lp.actor_device_ms_per_step() for k, lp in loops.items()}
    stats = {k: lp.e.stats() for k, lp in loops.items()}
    staging = {k: lp.L.staging_bytes for k, lp in loops.items()}
    for lp in loops.values():
        lp.close()
    km = env_kernel_ms(n, env_steps)
    floor_ms = n * 7056 / HBM_BYTES_PER_S * 1e3
    med = lambda v: float(np.median(v))  # noqa: E731
    return dict(num_envs=n, seq_len=T,
                wall_ms_per_unroll={k: dict(median=round(med(v), 3), min=round(min(v), 3), max=round(max(v), 3))
                                    for k, v in wall.items()},
                env_steps_per_s={k: round(n * T / med(v) * 1e3, 1) for k, v in wall.items()},
                actor_device_ms_per_step={k: round(v, 4) for k, v in actor_ms.items()},
                env_step_ms=round(km["step"], 5), env_render_ms=round(km["render"], 5),
                render_store_floor_ms=round(floor_ms, 6),
                render_share_of_floor=round(floor_ms / km["render"], 4),
                learner_staging_bytes=staging, episodes=stats)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_env_loop.json"))
    ap.add_argument("--unrolls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--env-steps", type=int, default=200)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("device_env_bench: no HIP device; nothing is measured without one")
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=args.num_actions, seed=1)
    params = L.get_params()
    L.close()
    rows = [measure(n, args.seq_len, args.num_actions, params, args.unrolls, args.warmup, args.env_steps)
            for n in args.envs]
    res = dict(what="one recording actor, one learner and N Catch environments on one device, Atari policy: "
                    "host-stepped loop vs fi_env_rollout",
               unrolls=args.unrolls, warmup=args.warmup, num_actions=args.num_actions,
               source_hash=build_info.source_hash(), rows=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
