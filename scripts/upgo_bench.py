#!/usr/bin/env python3
"""First measurement of the UPGO term (include/fi_upgo.h) on one device, on the Atari policy at T = 100, B = 4096,
A = 18.

  step     ms per step with and without the term: two learners of the same seed and batch (surrogate objective, KL
           penalty on the behaviour policy) stepped in turn, median / min / max over `--pairs` alternated pairs of
           unprofiled steps, and the pairwise difference. The "off" handle never calls fi_upgo_*.
  kernels  every launch by itself, from the step's own launch tags: upgo_scan, upgo_grad and upgo_finalize beside
           surrogate_scan (the serial chain over T that upgo_scan's suffix scan stands against) and kl_penalty (the
           row stream upgo_grad copies) of the same steps, each with the bytes it moves, that at 6.3 TB/s, and the ratio
           of its time to it.

Prints one JSON line and writes it to profiles/upgo_kernels.json.

    python scripts/upgo_bench.py [--out profiles/upgo_kernels.json] [--pairs 20] [--steps 5] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, hip, upgo  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from kl_bench import profiled  # noqa: E402
from surrogate_bench import HBM_BYTES_PER_S, bytes_per_row, spread  # noqa: E402

T, B, A = 100, 4096, 18
TAGS = ("surrogate_scan", "kl_penalty", "upgo_scan", "upgo_grad", "upgo_finalize")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upgo_kernels.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("upgo_bench: no HIP device; nothing is measured without one")
    P = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    Q = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    for L in (P, Q):
        L.set_objective("surrogate")
        L.enable_kl_penalty("behaviour")
        L.synth(seed=1)
    Q.enable_upgo()
    for _ in range(3):  # warm both up
        for L in (P, Q):
            L.step_resident()
    ms = dict(off=[], on=[])
    for _ in range(args.pairs):
        for L, name in ((P, "off"), (Q, "on")):
            ms[name].append(L.step_resident()["step_ms"])
    us = {k: [] for k in TAGS}
    for _ in range(args.rounds):
        profiled(Q, args.steps, TAGS, us)
    state = Q.upgo_state()
    for L in (P, Q):
        L.close()
    n = T * B * A
    moved = dict(upgo_scan=(4 * T + 1) * B * 4, upgo_grad=16 * n + 8 * T * B, kl_penalty=16 * n,
                 surrogate_scan=bytes_per_row(A)["surrogate_scan"] * T * B)

    def entry(v, k):
        e = dict(us_per_launch=spread(v))
        if k in moved:
            floor = moved[k] / HBM_BYTES_PER_S * 1e6
            e.update(bytes_moved=moved[k], floor_us=round(floor, 3), over_floor=round(statistics.median(v) / floor, 3))
        return e

    extra = [b - a for a, b in zip(ms["off"], ms["on"])]
    step = dict(policy="atari", objective="surrogate, KL penalty on the behaviour policy", pairs=args.pairs,
                off_ms_per_step=spread(ms["off"]), on_ms_per_step=spread(ms["on"]), on_minus_off_ms=spread(extra))
    res = dict(what="the UPGO term (fi_upgo.h) on the Atari policy at T = 100, B = 4096, A = 18: the step with and without "
                    "it in alternated pairs, and every launch by itself from the step's launch tags beside surrogate_scan "
                    "and kl_penalty of the same steps; first measurement, no threshold",
               T=T, B=B, A=A, hbm_bytes_per_s=HBM_BYTES_PER_S, workspace_bytes=upgo.workspace_bytes(T, B, A), step=step,
               kernels={k: entry(v, k) for k, v in us.items() if v}, upgo_state=state, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
