#!/usr/bin/env python3
"""First measurement of prioritised replay (include/fi_prio.h) beside the uniform rule it stands
next to: one device, Atari policy, A = 18, T = 20, B = 1024, K = 4 recording actors of N = 256 that
push into a device entry ring, and a learner that takes half of every batch fresh and half replayed
(the ring_half way of scripts/ring_bench.py: after every second unroll four steps at n_fresh = B / 2).

  uniform      step_ring(n_fresh = B / 2)
  prioritized  step_ring(n_fresh = B / 2, prioritized=True) on a ring with priorities enabled

Each way has its own learner, actors and ring; the two alternate unroll by unroll in one session,
driven from one thread. Per capacity (C = 4 B and C = 64 B): capacity / B + 2 warm-up unrolls, so
the window of replayable entries is as full as this schedule makes it, then `--unrolls` timed ones
-- wall ms per unroll, everything the caller waits for -- and a second pass of as many unrolls with
the learner's profiling on: the device ms of its ingest phase (for the prioritised way: the q_init
fill, the chunk sums, the draw and the gathering ingest). The refresh runs behind the step inside
the same call, so its device time is taken apart from it: its three launches (priorities from vs /
values, the two scatter passes) on the learner's stream, idle before, between HIP events, on a
scratch table of the ring's capacity with the entries of the learner's last batch.
Prints one JSON line and writes it to profiles/ring_prioritized.json.

    python scripts/prio_bench.py [--out profiles/ring_prioritized.json] [--unrolls 8]
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

from freeimpala_amd import build_info, hip, prio  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from freeimpala_amd.ring import EntryRing  # noqa: E402

WAYS = ("uniform", "prioritized")
ETA = 0.9


class Loop:
    def __init__(self, way: str, K: int, B: int, T: int, A: int, capacity: int, params: np.ndarray):
        self.way, self.K, self.n, self.T, self.B, self.C = way, K, B // K, T, B, capacity
        self.params = params
        self.L = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.actors = [Actor("atari", self.n, num_actions=A, seed=1 + k) for k in range(K)]
        self.ring = EntryRing(self.L.entry_bytes, capacity, seed=1)
        if way == "prioritized":
            self.ring.enable_priorities(ETA, 1.0)
        rs = np.random.RandomState(K)
        n = self.n
        self.sets = [(rs.randint(0, 256, (n, 84, 84)).astype(np.uint8), (rs.rand(n) < 0.01).astype(np.uint8),
                      rs.randint(-1, 2, n).astype(np.float32), (0.99 * (rs.rand(n) > 0.01)).astype(np.float32))
                     for _ in range(4)]
        self.calls = self.unrolls = self.steps = 0
        self.ingest_ms, self.windows = [], []
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

    def unroll(self) -> float:
        """One unroll of every actor, its pushes and, behind every second one, four steps: wall ms."""
        t0 = time.perf_counter()
        self.unrolls += 1
        for a in self.actors:
            a.set_params(self.params, version=self.unrolls)
        for _ in range(self.T):
            self.act_all()
        for a in self.actors:
            self.ring.push_rollout(a)
        if self.unrolls % 2 == 0:
            fresh = 0
            while fresh < 2 * self.B:
                i = self.ring.info()
                # the very first step has nothing to replay yet: it is read FIFO (a warm-up unroll)
                n = self.B // 2 if i["tail"] else self.B
                self.L.step_ring(self.ring, n_fresh=n, prioritized=self.way == "prioritized")
                self.steps += 1
                fresh += n
                if self.timed:
                    self.ingest_ms.append(self.L.phase_times()["ingest"])  # one step since the last read
                    self.windows.append(i["tail"] - max(0, i["head"] - self.C))
        return (time.perf_counter() - t0) * 1e3

    def refresh_ms(self, reps: int) -> list[float]:
        """Device ms of the refresh's three launches on the learner's stream, idle before each."""
        vs, _ = self.L.tensor_ptr("vs")
        values, _ = self.L.tensor_ptr("values")
        table = hip.DeviceBuffer.from_array(np.ones(self.C, np.uint32))
        entries = hip.DeviceBuffer.from_array(np.array(self.ring.last_entries(self.B), np.uint64))
        q = hip.DeviceBuffer(4 * self.B)
        out = []
        for k in range(reps + 2):
            hip.synchronize()
            e0, e1 = hip.Event(), hip.Event()
            e0.record(self.L.stream)
            prio.from_td(vs, values, self.T, self.B, ETA, q.ptr, self.L.stream)
            prio.scatter(table.ptr, self.C, entries.ptr, q.ptr, self.B, self.L.stream)
            e1.record(self.L.stream)
            if k >= 2:  # two warm-up repetitions
                out.append(e0.elapsed_ms(e1))
            else:
                e0.elapsed_ms(e1)
        for b in (table, entries, q):
            b.free()
        return out

    def close(self):
        for a in self.actors:
            a.end_rollout()
            a.close()
        self.ring.close()
        self.L.close()


def spread(v) -> dict:
    a = np.asarray(v, np.float64)
    return dict(mean=round(float(a.mean()), 4), median=round(float(np.median(a)), 4), min=round(float(a.min()), 4),
                max=round(float(a.max()), 4), std=round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), n=int(a.size))


def measure(K, B, T, A, capacity, unrolls, params) -> dict:
    loops = {w: Loop(w, K, B, T, A, capacity, params) for w in WAYS}
    warm = capacity // B + 2
    warm += warm % 2
    for _ in range(warm):
        for w in WAYS:
            loops[w].unroll()
    wall = {w: [] for w in WAYS}
    for _ in range(unrolls):
        for w in WAYS:
            wall[w].append(loops[w].unroll())
    for w in WAYS:
        loops[w].L.set_profiling(True)
        loops[w].timed = True
    for _ in range(unrolls):
        for w in WAYS:
            loops[w].unroll()
    rows = {}
    for w in WAYS:
        lp = loops[w]
        lp.L.set_profiling(False)
        rows[w] = dict(wall_ms_per_unroll=spread(wall[w]), wall_ms_per_unroll_all=[round(x, 3) for x in wall[w]],
                       learner_ingest_ms=spread(lp.ingest_ms), learner_ingest_ms_all=[round(x, 4) for x in lp.ingest_ms],
                       window_entries=spread(lp.windows), learner_steps=lp.steps, unrolls=lp.unrolls,
                       batch_versions=lp.L.batch_versions, ring=lp.ring.info())
    lp = loops["prioritized"]
    rows["prioritized"].update(refresh_ms=spread(lp.refresh_ms(16)), priorities=lp.ring.priority_info())
    q = lp.ring.priorities().astype(np.float64)
    rows["prioritized"]["priority_quantiles"] = [float(x) for x in np.quantile(q, (0.0, 0.25, 0.5, 0.75, 1.0))]
    pairs = np.asarray(wall["prioritized"]) - np.asarray(wall["uniform"])  # unroll by unroll, same session
    diff = dict(wall_ms_per_unroll=spread(pairs),
                learner_ingest_ms=round(rows["prioritized"]["learner_ingest_ms"]["median"] -
                                        rows["uniform"]["learner_ingest_ms"]["median"], 4))
    for lp in loops.values():
        lp.close()
    return dict(capacity=capacity, capacity_batches=capacity // B, warmup_unrolls=warm, rows=rows,
                prioritized_minus_uniform=diff)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_prioritized.json"))
    ap.add_argument("--unrolls", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--actors", type=int, default=4)
    ap.add_argument("--capacity-batches", type=int, nargs="+", default=[4, 64])
    args = ap.parse_args()
    K, B, T, A = args.actors, args.batch, args.seq_len, args.num_actions
    if K < 1 or K > 64 or B % K or B % 2 or args.unrolls % 2:
        ap.error("--actors must divide --batch, --batch and --unrolls must be even")
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=A, seed=1)
    params = L.get_params()
    entry = DeviceLearner("atari", seq_len=T, batch=1, num_actions=A, records="planes", seed=1)
    entry_bytes = entry.entry_bytes
    entry.close()
    L.close()
    runs = [measure(K, B, T, A, cb * B, args.unrolls, params) for cb in args.capacity_batches]
    res = dict(what="first measurement: one device, Atari policy, K recording actors push into a device entry ring and "
                    "one learner takes half of every batch fresh and half replayed, drawn uniformly or by priority; "
                    "the two alternate unroll by unroll, one thread",
               actors=K, num_envs_per_actor=B // K, batch=B, seq_len=T, num_actions=A, eta=ETA, entry_bytes=entry_bytes,
               unrolls=args.unrolls, source_hash=build_info.source_hash(), runs=runs)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
