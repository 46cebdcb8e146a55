#!/usr/bin/env python3
"""First measurement of the exploring draw (include/fi_explore.h): sample_behaviour_kernel beside
sample_actions_kernel, alternated in one session, at N = 256 and 1,024 rows of A = 18 logits.

Per N: after a warm-up, `--rounds` rounds; a round times `--launches` back-to-back launches of the plain
sampler between two HIP events, then as many of the new kernel (tau = 2, Ape-X's epsilon ladder), and
reports microseconds per launch (median / min / max over the rounds). At these N either kernel is one
to four workgroups: the plain sampler is a launch, like the other small kernels here (3-5 us); the
new one does more per lane behind the same launch (A IEEE divisions, A expf and A + 1 logf, one
lane per row, then the turn through LDS and N * A * 4 bytes of stores), and what that adds is the
measurement. The launches are issued through ctypes, so a per-launch figure is an upper bound on the
kernel's device time (it may be the host's submission rate). Then the `sample` phase of an Atari actor's act call (fi_actor_phase_times: the counter
reset and the draw between two events) with exploration off and on, alternated in blocks of `--calls`
calls. A first measurement with no bar. Prints one JSON line and writes it to
profiles/explore_sampler.json.

    python scripts/explore_bench.py [--out profiles/explore_sampler.json] [--rounds 20] [--launches 200] [--calls 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import actor, build_info, explore, hip  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

A, TAU = 18, 2.0


def spread(us: list[float]) -> dict:
    return dict(median=round(statistics.median(us), 3), min=round(min(us), 3), max=round(max(us), 3))


def kernels(n: int, rounds: int, launches: int) -> dict:
    rs = np.random.RandomState(n)
    logits = hip.DeviceBuffer.from_array((3.0 * rs.standard_normal((n, A))).astype(np.float32))
    eps = hip.DeviceBuffer.from_array(explore.epsilon_ladder(n))
    act, mu, bad = hip.DeviceBuffer(4 * n), hip.DeviceBuffer(4 * n * A), hip.DeviceBuffer.from_array(np.zeros(1, np.int32))

    def plain(draw):
        actor.sample_actions(logits.ptr, n, A, "sample", 1, draw, act.ptr, bad.ptr)

    def behaviour(draw):
        explore.sample_behaviour(logits.ptr, n, A, TAU, eps.ptr, 1, draw, act.ptr, mu.ptr, bad.ptr)

    t0, t1 = hip.Event(), hip.Event()
    out = dict(plain=[], behaviour=[])
    for r in range(rounds + 1):  # round 0 warms both kernels up
        for name, fn in (("plain", plain), ("behaviour", behaviour)):
            t0.record()
            for d in range(launches):
                fn(d)
            t1.record()
            us = t0.elapsed_ms(t1) * 1e3 / launches
            if r:
                out[name].append(us)
    hip.synchronize()
    for b in (logits, eps, act, mu, bad):
        b.free()
    return dict(num_envs=n, num_actions=A, mu_bytes_per_launch=4 * n * A,
                us_per_launch=dict(sample_actions=spread(out["plain"]), sample_behaviour=spread(out["behaviour"])))


def phases(n: int, params: np.ndarray, calls: int, blocks: int = 3) -> dict:
    rs = np.random.RandomState(n + 1)
    a = Actor("atari", n, num_actions=A, seed=1)
    a.set_params(params)
    planes = [rs.randint(0, 256, (n, 84, 84)).astype(np.uint8) for _ in range(2)]
    start = np.zeros(n, np.uint8)
    eps = explore.epsilon_ladder(n)
    for i in range(5):
        a.act_planes(planes[i % 2], start)
    a.set_exploration(TAU, eps)
    for i in range(5):
        a.act_planes(planes[i % 2], start)
    out = dict(off=[], on=[])
    for _ in range(blocks):
        for name in ("off", "on"):
            if name == "on":
                a.set_exploration(TAU, eps)
            else:
                a.clear_exploration()
            a.set_profiling(True)
            for i in range(calls):
                a.act_planes(planes[i % 2], start)
            out[name].append(a.phase_times()["sample"] * 1e3)
            a.set_profiling(False)
    a.close()
    return dict(num_envs=n, num_actions=A, calls_per_block=calls,
                sample_phase_us=dict(exploration_off=spread(out["off"]), exploration_on=spread(out["on"])))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_sampler.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("explore_bench: no HIP device; nothing is measured without one")
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=A, seed=1)
    params = L.get_params()
    L.close()
    res = dict(what="sample_actions_kernel and sample_behaviour_kernel (fi_explore.h) alternated in one session: us per "
                    "launch from HIP events around back-to-back launches, and the sample phase of an Atari act call "
                    "with exploration off and on; one to four workgroups either way, so the difference is one lane's "
                    "arithmetic per row behind the same launch; first measurement, no bar",
               temperature=TAU, epsilon="epsilon_ladder(N)", rounds=args.rounds, launches_per_round=args.launches,
               kernels=[kernels(n, args.rounds, args.launches) for n in args.envs],
               act_call=[phases(n, params, args.calls) for n in args.envs], source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
