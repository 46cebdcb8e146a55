#!/usr/bin/env python3
"""First measurement of the column-weight kernels (include/fi_weights.h) on one device.

  scale   fi_weights_scale_columns alone at T = 100, B = 4096, A = 18 (the bench shape's dlogits and
          dvalue, 31 MB), by HIP events around bursts of launches after warm-up, beside its floor of
          2 * 4 * T * B * (A + 1) bytes / 6.3 TB/s. One set of buffers stays in the 256 MB Infinity
          Cache between launches (a warm figure); `--sets` disjoint copies, taken in turn, push every
          launch's tensors out of it before their turn comes again (the HBM figure).
  steps   the prioritised loop of scripts/prio_bench.py (Atari policy, A = 18, T = 20, B = 1024, K = 4
          recording actors of N = 256 push into a device entry ring of 4 B slots, the learner takes half
          of every batch fresh and half replayed by priority) with beta = 0 and with beta = 0.4, each
          with its own learner, actors and ring, alternated unroll by unroll in one session: wall ms
          per unroll, and in a second pass with the learner's profiling on the device ms of its ingest
          phase (with beta > 0: plus prio_is_weights_kernel) and of its V-trace phase (with beta > 0:
          plus scale_columns_kernel).

Prints one JSON line and writes it to profiles/is_weights.json.

    python scripts/is_weights_bench.py [--out profiles/is_weights.json] [--unrolls 8]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from freeimpala_amd import build_info, hip, weights  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from prio_bench import Loop, spread  # noqa: E402

HBM_TBS = 6.3
BETAS = (0.0, 0.4)


def scale_alone(T: int, B: int, A: int, sets: int, bursts: int, per_burst: int) -> dict:
    """us per launch of the scale kernel: `bursts` event pairs around `per_burst` launches each."""
    rs = np.random.RandomState(0)
    dlog = rs.standard_normal(T * B * A).astype(np.float32)
    dval = rs.standard_normal((T + 1) * B).astype(np.float32)
    w = hip.DeviceBuffer.from_array(np.ones(B, np.float32))  # ones: the values stay what they are over any number of launches
    bufs = [(hip.DeviceBuffer.from_array(dlog), hip.DeviceBuffer.from_array(dval)) for _ in range(sets)]
    n = 0

    def launch():
        nonlocal n
        a, b = bufs[n % sets]
        weights.scale_columns(a.ptr, b.ptr, w.ptr, T, B, A)
        n += 1

    for _ in range(max(3, sets)):
        launch()
    hip.synchronize()
    us = []
    for _ in range(bursts):
        e0, e1 = hip.Event(), hip.Event()
        e0.record()
        for _ in range(per_burst):
            launch()
        e1.record()
        us.append(e0.elapsed_ms(e1) * 1e3 / per_burst)
    for a, b in bufs:
        a.free()
        b.free()
    w.free()
    return dict(sets=sets, set_bytes=4 * (dlog.size + dval.size), launches_per_burst=per_burst, us_per_launch=spread(us),
                us_per_launch_all=[round(x, 3) for x in us])


class WeightedLoop(Loop):
    """prio_bench's prioritised loop on a ring with exponents (1, beta); the timed pass keeps the
    learner's ingest and V-trace phases of every step."""

    def __init__(self, beta: float, *args):
        super().__init__("prioritized", *args)
        self.ring.set_priority_exponents(1.0, beta)
        self.vtrace_ms = []

    def unroll(self) -> float:
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
                n = self.B // 2 if self.ring.info()["tail"] else self.B  # the very first step has nothing to replay
                self.L.step_ring(self.ring, n_fresh=n, prioritized=True)
                self.steps += 1
                fresh += n
                if self.timed:
                    ph = self.L.phase_times()  # one step since the last read
                    self.ingest_ms.append(ph["ingest"])
                    self.vtrace_ms.append(ph["vtrace"])
        return (time.perf_counter() - t0) * 1e3


def steps(K, B, T, A, capacity, unrolls, params) -> dict:
    loops = {b: WeightedLoop(b, K, B, T, A, capacity, params) for b in BETAS}
    warm = capacity // B + 2
    warm += warm % 2
    for _ in range(warm):
        for b in BETAS:
            loops[b].unroll()
    wall = {b: [] for b in BETAS}
    for _ in range(unrolls):
        for b in BETAS:
            wall[b].append(loops[b].unroll())
    for b in BETAS:
        loops[b].L.set_profiling(True)
        loops[b].timed = True
    for _ in range(unrolls):
        for b in BETAS:
            loops[b].unroll()
    rows = {}
    for b in BETAS:
        lp = loops[b]
        lp.L.set_profiling(False)
        w = lp.ring.last_weights(B)
        rows[f"beta_{b}"] = dict(
            wall_ms_per_unroll=spread(wall[b]), wall_ms_per_unroll_all=[round(x, 3) for x in wall[b]],
            learner_ingest_ms=spread(lp.ingest_ms), learner_ingest_ms_all=[round(x, 4) for x in lp.ingest_ms],
            learner_vtrace_ms=spread(lp.vtrace_ms), learner_vtrace_ms_all=[round(x, 4) for x in lp.vtrace_ms],
            learner_steps=lp.steps, unrolls=lp.unrolls, exponents=lp.ring.priority_exponents(),
            last_weight_quantiles=[float(x) for x in np.quantile(w, (0.0, 0.25, 0.5, 0.75, 1.0))])
    lo, hi = (rows[f"beta_{b}"] for b in BETAS)
    pairs = np.asarray(wall[BETAS[1]]) - np.asarray(wall[BETAS[0]])  # unroll by unroll, same session
    diff = dict(wall_ms_per_unroll=spread(pairs),
                learner_ingest_ms=round(hi["learner_ingest_ms"]["median"] - lo["learner_ingest_ms"]["median"], 4),
                learner_vtrace_ms=round(hi["learner_vtrace_ms"]["median"] - lo["learner_vtrace_ms"]["median"], 4))
    for lp in loops.values():
        lp.close()
    return dict(capacity=capacity, capacity_batches=capacity // B, warmup_unrolls=warm, rows=rows,
                weighted_minus_unweighted=diff)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "is_weights.json"))
    ap.add_argument("--unrolls", type=int, default=8)
    ap.add_argument("--sets", type=int, default=10, help="disjoint buffer sets of the HBM figure (10 x 31 MB > 256 MB)")
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    if args.unrolls % 2:
        ap.error("--unrolls must be even")
    T, B, A = 100, 4096, 18
    floor_us = 2 * 4 * T * B * (A + 1) / (HBM_TBS * 1e12) * 1e6
    scale = dict(seq_len=T, batch=B, num_actions=A, bytes_moved=2 * 4 * T * B * (A + 1), hbm_tbs=HBM_TBS,
                 floor_us=round(floor_us, 3), warm=scale_alone(T, B, A, 1, args.bursts, 20),
                 rotating=scale_alone(T, B, A, args.sets, args.bursts, 2 * args.sets))
    res = dict(what="first measurement: the column-scale kernel alone beside its HBM floor, and prio_bench's prioritised "
                    "loop with beta = 0 and beta = 0.4, alternated unroll by unroll, one thread",
               source_hash=build_info.source_hash(), scale_columns=scale)
    if not args.skip_steps:
        K, Bs, Ts = 4, 1024, 20
        L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=A, seed=1)
        params = L.get_params()
        L.close()
        res["steps"] = dict(actors=K, num_envs_per_actor=Bs // K, batch=Bs, seq_len=Ts, num_actions=A, eta=0.9, alpha=1.0,
                            betas=list(BETAS), unrolls=args.unrolls, run=steps(K, Bs, Ts, A, 4 * Bs, args.unrolls, params))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
