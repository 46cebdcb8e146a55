#!/usr/bin/env python3
"""First measurements of the closed loop on one device (include/fi_rollout.h): one Atari actor and
one learner, A = 18, N = B in {256, 1024}, T = 20, fed two ways that alternate unroll by unroll in
one session:

  host loop    act_planes x T -> the stacks read back for the history -> pack_atari_plane_records
               -> DeviceLearner.step (pinned copy, H2D, ingest, step)
  device loop  recording act_planes + outcome x T -> DeviceLearner.step_rollout (the ingest reads the
               actor's device buffer in place)

Per N: 1 warm-up unroll of each, then `--unrolls` timed ones: wall ms per unroll (everything the
caller waits for, the learner step included), the act call's wall ms without and with recording
(the recording one includes its fi_rollout_outcome), the learner's step_ms, and from a second pass
with the learners' profiling on the device ms of their ingest phase (HIP events; on the host path
it starts when the step is enqueued, so it includes what is left of the H2D copy). Prints one JSON
line and writes it to profiles/rollout_loop.json.

    python scripts/rollout_bench.py [--out profiles/rollout_loop.json] [--unrolls 5]
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
from freeimpala_amd.learner import DeviceLearner, pack_atari_plane_records  # noqa: E402


def now() -> float:
    return time.perf_counter()


class Loop:
    def __init__(self, n: int, T: int, A: int, params: np.ndarray, device_side: bool, sets):
        self.n, self.T, self.device_side, self.sets = n, T, device_side, sets
        self.L = DeviceLearner("atari", seq_len=T, batch=n, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.a = Actor("atari", n, num_actions=A, seed=1)
        self.a.set_params(params)
        self.calls = 0
        self.act_s, self.act_n = 0.0, 0
        self.steps = []  # (planes, start, logits, actions, rew, disc) of the unroll being acted (host loop)
        if device_side:
            self.a.begin_rollout(T)
        self.act()  # step 0 of the first unroll

    def act(self):
        planes, start, rew, disc = self.sets[self.calls % len(self.sets)]
        if self.calls == 0:
            start = np.ones_like(start)
        t0 = now()
        out = self.a.act_planes(planes, start)
        if self.device_side:
            self.a.outcome(rew, disc)
        self.act_s += now() - t0
        self.act_n += 1
        self.calls += 1
        if not self.device_side:
            self.steps.append((planes, start, out["logits"], out["actions"], rew, disc))

    def unroll(self) -> tuple[float, float]:
        """T act calls and the learner step of the unroll they complete: (wall ms, step_ms)."""
        t0 = now()
        history = None
        if not self.device_side:  # the stacks the unroll's step 0 ran on hold its history
            history = np.ascontiguousarray(np.moveaxis(self.a.stacks()[..., :3], -1, 0))
        for _ in range(self.T):
            self.act()
        if self.device_side:
            st = self.L.step_rollout(self.a)
        else:
            s = self.steps
            batch = pack_atari_plane_records(np.stack([x[0] for x in s]), history, np.stack([x[1] for x in s]),
                                             np.stack([x[2] for x in s[:-1]]), np.stack([x[3] for x in s[:-1]]),
                                             np.stack([x[4] for x in s[:-1]]), np.stack([x[5] for x in s[:-1]]))
            st = self.L.step(batch)
            self.steps = s[-1:]
        return (now() - t0) * 1e3, st["step_ms"]

    def take_act_ms(self) -> float:
        ms = self.act_s * 1e3 / max(1, self.act_n)
        self.act_s, self.act_n = 0.0, 0
        return ms

    def close(self):
        if self.device_side:
            self.a.end_rollout()
        self.a.close()
        self.L.close()


def measure(n: int, T: int, A: int, params: np.ndarray, unrolls: int) -> dict:
    rs = np.random.RandomState(n)
    sets = [(rs.randint(0, 256, (n, 84, 84)).astype(np.uint8), (rs.rand(n) < 0.01).astype(np.uint8),
             rs.randint(-1, 2, n).astype(np.float32), (0.99 * (rs.rand(n) > 0.01)).astype(np.float32))
            for _ in range(4)]
    loops = dict(host=Loop(n, T, A, params, False, sets), device=Loop(n, T, A, params, True, sets))
    for lp in loops.values():  # warm-up
        lp.unroll()
        lp.take_act_ms()
    wall = dict(host=[], device=[])
    step = dict(host=[], device=[])
    for _ in range(unrolls):  # alternating
        for k, lp in loops.items():
            w, s = lp.unroll()
            wall[k].append(w)
            step[k].append(s)
    act_ms = {k: lp.take_act_ms() for k, lp in loops.items()}
    ingest = {}
    for k, lp in loops.items():
        lp.L.set_profiling(True)
        for _ in range(max(2, unrolls // 2)):
            lp.unroll()
        ingest[k] = lp.L.phase_times()["ingest"]
        lp.L.set_profiling(False)
    staging = {k: lp.L.staging_bytes for k, lp in loops.items()}
    entry = loops["device"].a.rollout_entry_bytes
    for lp in loops.values():
        lp.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    return dict(num_envs=n, seq_len=T, entry_bytes=entry, rollout_buffer_bytes=2 * n * entry,
                learner_staging_bytes=staging,
                wall_ms_per_unroll={k: round(med(v), 3) for k, v in wall.items()},
                wall_ms_per_unroll_all={k: [round(x, 3) for x in v] for k, v in wall.items()},
                learner_step_ms={k: round(med(v), 3) for k, v in step.items()},
                learner_ingest_ms={k: round(v, 4) for k, v in ingest.items()},
                act_wall_ms=dict(plain=round(act_ms["host"], 4), recording_with_outcome=round(act_ms["device"], 4)),
                env_steps_per_s={k: round(n * T / med(v) * 1e3, 1) for k, v in wall.items()})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_loop.json"))
    ap.add_argument("--unrolls", type=int, default=5)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=args.num_actions, seed=1)
    params = L.get_params()
    L.close()
    rows = [measure(n, args.seq_len, args.num_actions, params, args.unrolls) for n in args.envs]
    res = dict(what="one actor and one learner on one device, Atari policy: host loop vs device loop",
               unrolls=args.unrolls, num_actions=args.num_actions, source_hash=build_info.source_hash(), rows=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
