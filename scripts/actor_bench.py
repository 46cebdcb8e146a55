#!/usr/bin/env python3
"""First measurements of the acting path (include/fi_actor.h): the Atari policy on N
environments per act call, N in {64, 256, 1024}, fed single planes (the stacks stay on the device)
and whole frames.

Per (N, input): 5 warm-up calls, then 20 timed calls for the wall time per call (host copy into
the pinned buffer, H2D, kernels, D2H, host copy out: what a caller waits for), then 20 calls with
the handle's profiling on for the device time per phase (HIP events between the phases: H2D, stack
push, forward, sampling, D2H). Prints one JSON line and writes it to profiles/actor_act.json.

    python scripts/actor_bench.py [--out profiles/actor_act.json] [--calls 20] [--warmup 5]
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

from freeimpala_amd import build_info  # noqa: E402
from freeimpala_amd.actor import PHASES, Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402


def measure(n_envs: int, kind: str, params: np.ndarray, calls: int, warmup: int, actions: int) -> dict:
    rs = np.random.RandomState(n_envs)
    a = Actor("atari", n_envs, num_actions=actions, seed=1)
    a.set_params(params)
    if kind == "planes":
        sets = [rs.randint(0, 256, (n_envs, 84, 84)).astype(np.uint8) for _ in range(4)]
        start = [(rs.rand(n_envs) < 0.01).astype(np.uint8) for _ in range(4)]
        start[0][:] = 1

        def call(i):
            return a.act_planes(sets[i % 4], start[i % 4] if i else start[0])
    else:
        sets = [rs.randint(0, 256, (n_envs, 84, 84, 4)).astype(np.uint8) for _ in range(2)]

        def call(i):
            return a.act_frames(sets[i % 2])
    for i in range(warmup):
        call(i)
    t0 = time.perf_counter()
    for i in range(calls):
        call(warmup + i)
    wall_ms = (time.perf_counter() - t0) * 1e3 / calls
    a.set_profiling(True)
    for i in range(calls):
        call(warmup + calls + i)
    ph = a.phase_times()
    a.set_profiling(False)
    a.close()
    dev_ms = sum(ph[k] for k in PHASES)
    return dict(num_envs=n_envs, input=kind, input_bytes_per_call=int(sets[0].nbytes + (n_envs if kind == "planes" else 0)),
                wall_ms_per_call=round(wall_ms, 4), env_steps_per_s=round(n_envs / wall_ms * 1e3, 1),
                device_ms_per_call=round(dev_ms, 4), phase_ms={k: round(ph[k], 4) for k in PHASES},
                dominant_phase=max(PHASES, key=lambda k: ph[k]), profiled_calls=ph["calls"])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_act.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 256, 1024])
    args = ap.parse_args()
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=args.num_actions, seed=1)
    params = L.get_params()
    L.close()
    rows = [measure(n, kind, params, args.calls, args.warmup, args.num_actions)
            for n in args.envs for kind in ("planes", "frames")]
    res = dict(what="fi_actor act call, Atari policy", calls=args.calls, warmup=args.warmup,
               num_actions=args.num_actions, source_hash=build_info.source_hash(), rows=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
