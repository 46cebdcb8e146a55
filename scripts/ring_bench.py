#!/usr/bin/env python3
"""First measurements of the device entry ring (include/fi_ring.h) between recording actors and a
learner on one device: Atari policy, A = 18, T = 20, B = 1024, K = 4 actors of N = 256, a ring of
C = 4 B entries. Three ways to feed the learner, each with its own learner, actors (and ring),
alternated unroll by unroll in one session and driven from one thread:

  rollouts   T rounds of act calls, then step_rollouts over the four actors (no ring)
  ring_fifo  the same rounds, push_rollout x 4, then step_ring(n_fresh = B)
  ring_half  the same rounds and pushes; after every second round step_ring(n_fresh = B / 2),
             four times: half of every batch fresh, half replayed. Two rounds push 2 B entries
             and four such steps take 2 B as fresh, so the learner keeps up: two steps per unroll,
             twice the learner work of the other ways, which is what replaying one entry per
             fresh one costs. (One such step per two rounds takes B / 2 of 2 B: the ring is full
             of unread entries after six rounds, and since an unread entry is never overwritten
             nothing read is resident any more -- the replay set is empty and the step refused.)
             A push the ring refuses ("full", the reference's try_write) is counted and that
             unroll dropped; none is expected here.

Before every unroll each actor is given the parameters again with the unroll's number as their
version, so batch_versions shows the lag of what a step reads. Per way: 2 warm-up unrolls, then
`--unrolls` timed ones -- wall ms per unroll (everything the caller waits for) -- and a second pass
of as many unrolls with the learner's profiling on: the device ms of its ingest phase (the column
table and the gathering ingest) and of every accepted push, by HIP events on the ring's stream
around the call with the device idle before it, beside the copy's floor 2 N entry_bytes / 6.3 TB/s.
Prints one JSON line and writes it to profiles/ring_replay.json.

    python scripts/ring_bench.py [--out profiles/ring_replay.json] [--unrolls 8]
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

from freeimpala_amd import build_info, hip  # noqa: E402
from freeimpala_amd._abi import FiError  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from freeimpala_amd.ring import EntryRing  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
WAYS = ("rollouts", "ring_fifo", "ring_half")


def now() -> float:
    return time.perf_counter()


class Loop:
    def __init__(self, way: str, K: int, B: int, T: int, A: int, capacity: int, params: np.ndarray):
        self.way, self.K, self.n, self.T, self.B = way, K, B // K, T, B
        self.params = params
        self.L = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.actors = [Actor("atari", self.n, num_actions=A, seed=1 + k) for k in range(K)]
        self.ring = EntryRing(self.L.entry_bytes, capacity, seed=1) if way != "rollouts" else None
        rs = np.random.RandomState(K)
        n = self.n
        self.sets = [(rs.randint(0, 256, (n, 84, 84)).astype(np.uint8), (rs.rand(n) < 0.01).astype(np.uint8),
                      rs.randint(-1, 2, n).astype(np.float32), (0.99 * (rs.rand(n) > 0.01)).astype(np.float32))
                     for _ in range(4)]
        self.calls = self.unrolls = self.refused = self.pushes = self.steps = 0
        self.push_ms, self.ingest_ms = [], []
        self.timed = False
        for a in self.actors:
            a.set_params(params, version=0)
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

    def push_all(self):
        for a in self.actors:
            if self.timed:
                hip.synchronize()  # the push waits for nothing: the events bracket the copy alone
                e0, e1 = hip.Event(), hip.Event()
                e0.record(self.ring.stream)
            try:
                self.ring.push_rollout(a)
                self.pushes += 1
            except FiError as e:
                if "full" not in str(e):
                    raise
                a.release_rollout()  # try_write failed: the unroll is dropped
                self.refused += 1
                continue
            if self.timed:
                e1.record(self.ring.stream)
                self.push_ms.append(e0.elapsed_ms(e1))

    def unroll(self) -> float:
        """One unroll of every actor and what this way does behind it: wall ms."""
        t0 = now()
        self.unrolls += 1
        for a in self.actors:
            a.set_params(self.params, version=self.unrolls)
        for _ in range(self.T):
            self.act_all()
        if self.way == "rollouts":
            self.L.step_rollouts(self.actors)
            self.stepped()
        else:
            self.push_all()
            if self.way == "ring_fifo":
                self.L.step_ring(self.ring)
                self.stepped()
            elif self.unrolls % 2 == 0:
                fresh = 0
                while fresh < 2 * self.B:
                    # the very first step has nothing to replay yet: it is read FIFO (a warm-up unroll)
                    n = self.B // 2 if self.ring.info()["tail"] else self.B
                    self.L.step_ring(self.ring, n_fresh=n)
                    self.stepped()
                    fresh += n
        return (now() - t0) * 1e3

    def stepped(self):
        self.steps += 1
        if self.timed:
            self.ingest_ms.append(self.L.phase_times()["ingest"])  # one step since the last read

    def close(self):
        for a in self.actors:
            a.end_rollout()
            a.close()
        if self.ring:
            self.ring.close()
        self.L.close()


def med(v) -> float:
    return float(np.median(v)) if len(v) else float("nan")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_replay.json"))
    ap.add_argument("--unrolls", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--actors", type=int, default=4)
    ap.add_argument("--capacity-batches", type=int, default=4)
    args = ap.parse_args()
    K, B, T, A = args.actors, args.batch, args.seq_len, args.num_actions
    if K < 1 or K > 64 or B % K or B % 2 or args.unrolls % 2:
        ap.error("--actors must divide --batch, --batch and --unrolls must be even")
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=A, seed=1)
    params = L.get_params()
    L.close()
    loops = {w: Loop(w, K, B, T, A, args.capacity_batches * B, params) for w in WAYS}
    for _ in range(2):  # warm-up, alternating
        for w in WAYS:
            loops[w].unroll()
    wall = {w: [] for w in WAYS}
    for _ in range(args.unrolls):
        for w in WAYS:
            wall[w].append(loops[w].unroll())
    for w in WAYS:
        loops[w].L.set_profiling(True)
        loops[w].timed = True
    for _ in range(args.unrolls):
        for w in WAYS:
            loops[w].unroll()
    entry = loops["ring_fifo"].L.entry_bytes
    floor_us = 2 * (B // K) * entry / HBM_BYTES_PER_S * 1e6
    rows = {}
    for w in WAYS:
        lp = loops[w]
        lp.L.set_profiling(False)
        row = dict(wall_ms_per_unroll=round(float(np.mean(wall[w])), 3),
                   wall_ms_per_unroll_median=round(med(wall[w]), 3),
                   wall_ms_per_unroll_all=[round(x, 3) for x in wall[w]],
                   env_steps_per_s=round(B * T / float(np.mean(wall[w])) * 1e3, 1),
                   learner_steps=lp.steps, unrolls=lp.unrolls,
                   learner_ingest_ms=round(med(lp.ingest_ms), 4),
                   learner_ingest_ms_all=[round(x, 4) for x in lp.ingest_ms],
                   batch_versions=lp.L.batch_versions, learner_staging_bytes=lp.L.staging_bytes)
        if lp.ring:
            row.update(push_ms_per_actor=round(med(lp.push_ms), 4),
                       push_ms_per_actor_all=[round(x, 4) for x in lp.push_ms],
                       push_floor_ms=round(floor_us / 1e3, 4),
                       push_bytes=2 * (B // K) * entry,
                       push_share_of_floor=round(floor_us / 1e3 / med(lp.push_ms), 3) if lp.push_ms else None,
                       pushes_accepted=lp.pushes, pushes_refused_full=lp.refused, ring=lp.ring.info())
        rows[w] = row
    for lp in loops.values():
        lp.close()
    res = dict(what="one device, Atari policy: K recording actors and one learner fed by step_rollouts, by a device "
                    "entry ring read FIFO, and by the ring with half of every batch replayed; alternated unroll by "
                    "unroll, one thread",
               actors=K, num_envs_per_actor=B // K, batch=B, seq_len=T, num_actions=A, capacity=args.capacity_batches * B,
               entry_bytes=entry, unrolls=args.unrolls, hbm_bytes_per_s=HBM_BYTES_PER_S,
               source_hash=build_info.source_hash(), rows=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
