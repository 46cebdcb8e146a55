#!/usr/bin/env python3
"""First measurements of one learner batch filled by several recording actors on one device
(include/fi_gather.h): Atari policy, A = 18, T = 20, B = 1024, K in {1, 4, 16} actors of N = B / K,
driven round-robin from one thread (every actor's act call and outcome, step by step; then
DeviceLearner.step_rollouts over all K). One process.

Per K: 1 warm-up unroll, then `--unrolls` timed ones: wall ms per unroll (everything the caller
waits for, the learner step included) and env-steps/s, the learner's step_ms, and from a second
pass with the learner's profiling on the device ms of its ingest phase (HIP events: the column
table, the gathering ingest). At K = 1 the same actor also feeds the plain step_rollout (the
contiguous ingest) in the same session, the two alternating unroll by unroll, so the gathering
ingest is compared with the contiguous one on one box; every ingest reading is kept, so the
contiguous ingest's own run-to-run spread stands beside the difference. Prints one JSON line and
writes it to profiles/rollout_multi_actor.json.

    python scripts/multi_actor_bench.py [--out profiles/rollout_multi_actor.json] [--unrolls 6]
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
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402


def now() -> float:
    return time.perf_counter()


class Loop:
    def __init__(self, K: int, B: int, T: int, A: int, params: np.ndarray):
        self.K, self.n, self.T = K, B // K, T
        self.L = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.actors = [Actor("atari", self.n, num_actions=A, seed=1 + k) for k in range(K)]
        rs = np.random.RandomState(K)
        n = self.n
        self.sets = [(rs.randint(0, 256, (n, 84, 84)).astype(np.uint8), (rs.rand(n) < 0.01).astype(np.uint8),
                      rs.randint(-1, 2, n).astype(np.float32), (0.99 * (rs.rand(n) > 0.01)).astype(np.float32))
                     for _ in range(4)]
        self.calls = 0
        for k, a in enumerate(self.actors):
            a.set_params(params, version=k)
            a.begin_rollout(T)
        self.act_all()  # step 0 of the first unroll

    def act_all(self):
        for k, a in enumerate(self.actors):
            planes, start, rew, disc = self.sets[(self.calls + k) % len(self.sets)]
            if self.calls == 0:
                start = np.ones_like(start)
            a.act_planes(planes, start)
            a.outcome(rew, disc)
        self.calls += 1

    def unroll(self, plain: bool = False) -> tuple[float, float]:
        """T rounds of act calls and the learner step of the unrolls they complete: (wall ms, step_ms).
        plain (K = 1): fi_learner_step_rollout, the contiguous ingest."""
        t0 = now()
        for _ in range(self.T):
            self.act_all()
        st = self.L.step_rollout(self.actors[0]) if plain else self.L.step_rollouts(self.actors)
        return (now() - t0) * 1e3, st["step_ms"]

    def close(self):
        for a in self.actors:
            a.end_rollout()
            a.close()
        self.L.close()


def med(v) -> float:
    return float(np.median(v))


def measure(K: int, B: int, T: int, A: int, params: np.ndarray, unrolls: int) -> dict:
    lp = Loop(K, B, T, A, params)
    kinds = ["gather", "contiguous"] if K == 1 else ["gather"]
    for kind in kinds:  # warm-up
        lp.unroll(kind == "contiguous")
    wall = {k: [] for k in kinds}
    step = {k: [] for k in kinds}
    for _ in range(unrolls):  # alternating
        for kind in kinds:
            w, s = lp.unroll(kind == "contiguous")
            wall[kind].append(w)
            step[kind].append(s)
    ingest = {k: [] for k in kinds}
    lp.L.set_profiling(True)
    for _ in range(unrolls):
        for kind in kinds:
            lp.unroll(kind == "contiguous")
            ingest[kind].append(lp.L.phase_times()["ingest"])  # one step since the last read
    lp.L.set_profiling(False)
    versions = lp.L.batch_versions
    staging = lp.L.staging_bytes
    lp.close()
    row = dict(actors=K, num_envs_per_actor=B // K, batch=B, seq_len=T, learner_staging_bytes=staging,
               batch_versions=versions,
               wall_ms_per_unroll={k: round(med(v), 3) for k, v in wall.items()},
               wall_ms_per_unroll_all={k: [round(x, 3) for x in v] for k, v in wall.items()},
               env_steps_per_s={k: round(B * T / med(v) * 1e3, 1) for k, v in wall.items()},
               learner_step_ms={k: round(med(v), 3) for k, v in step.items()},
               learner_ingest_ms={k: round(med(v), 4) for k, v in ingest.items()},
               learner_ingest_ms_all={k: [round(x, 4) for x in v] for k, v in ingest.items()})
    if K == 1:
        c = ingest["contiguous"]
        row["ingest_gather_minus_contiguous_ms"] = round(med(ingest["gather"]) - med(c), 4)
        row["ingest_contiguous_spread_ms"] = round(max(c) - min(c), 4)
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_multi_actor.json"))
    ap.add_argument("--unrolls", type=int, default=6)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--actors", type=int, nargs="+", default=[1, 4, 16])
    args = ap.parse_args()
    for K in args.actors:
        if K < 1 or K > 64 or args.batch % K:
            ap.error(f"--actors {K}: 1 .. 64 actors that divide --batch {args.batch}")
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=args.num_actions, seed=1)
    params = L.get_params()
    L.close()
    rows = [measure(K, args.batch, args.seq_len, args.num_actions, params, args.unrolls) for K in args.actors]
    res = dict(what="K recording actors of N = B / K fill one learner batch on one device, Atari policy, round-robin "
                    "from one thread; at K = 1 also the plain step_rollout, alternating",
               unrolls=args.unrolls, num_actions=args.num_actions, source_hash=build_info.source_hash(), rows=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
