#!/usr/bin/env python3
"""First measurement of the learner's adaptive KL penalty (include/fi_kl.h) on one device, on the Atari policy at
T = 100, B = 4096, A = 18.

  step     ms per surrogate-with-target step with and without the penalty (reference "target"): two learners of the
           same seed and batch stepped in turn, median / min / max over `--pairs` alternated pairs of unprofiled
           steps, and the pairwise difference. The "off" handle never calls fi_kl_*: its step is the step as it was
           before there was a penalty.
  kernels  every launch by itself, from the step's own launch tags, the handles profiled in turn: kl_penalty (three
           reads and one write of T * B * A floats) and kl_adapt beside target_loss of the same steps, and beside
           surrogate_loss and scale_columns of the "off" handle with its target disabled and column weights set,
           each with the bytes it moves at 6.3 TB/s and the ratio of its time to that.
  burst    fi_kl_penalty_fp32 alone on the handle's own tensors in bursts of `--launches`: back to back, warm.

Prints one JSON line and writes it to profiles/kl_penalty.json.

    python scripts/kl_bench.py [--out profiles/kl_penalty.json] [--pairs 20] [--steps 5] [--rounds 5] [--launches 50]
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

from freeimpala_amd import build_info, hip, kl  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from surrogate_bench import HBM_BYTES_PER_S, bytes_per_row, kernel_times, spread  # noqa: E402
from target_bench import burst_us  # noqa: E402

T, B, A = 100, 4096, 18
ON_TAGS = ("target_loss", "kl_penalty", "kl_adapt")
OFF_TAGS = ("surrogate_loss", "scale_columns")


def profiled(L: DeviceLearner, steps: int, tags, into: dict) -> None:
    L.set_profiling(True)
    for _ in range(steps):
        L.step_resident()
    kt = kernel_times(L)
    L.set_profiling(False)
    for k in tags:
        if k in kt:
            into[k].append(kt[k])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_penalty.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("kl_bench: no HIP device; nothing is measured without one")
    P = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    Q = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    for L in (P, Q):
        L.set_objective("surrogate")
        L.enable_target(period=1)
        L.synth(seed=1)
    Q.enable_kl_penalty("target")
    for _ in range(3):  # warm both up
        for L in (P, Q):
            L.step_resident()
    ms = dict(off=[], on=[])
    for _ in range(args.pairs):
        for L, name in ((P, "off"), (Q, "on")):
            ms[name].append(L.step_resident()["step_ms"])
    us = {k: [] for k in ON_TAGS + OFF_TAGS}
    for _ in range(args.rounds):
        profiled(Q, args.steps, ON_TAGS, us)
    state = Q.kl_state()
    # the penalty kernel alone, back to back on the handle's own tensors (the coefficient is read from the block)
    n = T * B * A
    ws_bytes = kl.workspace_bytes(T, B, A)
    ws = hip.DeviceBuffer(ws_bytes)
    pi, q, dl = Q.tensor_ptr("logits")[0], Q.target_logits_dev(), Q.tensor_ptr("dlogits")[0]
    took = [burst_us(Q, args.launches, lambda: kl.kl_penalty_dev(T, B, A, pi, q, dl, Q.kl_state_dev(), ws.ptr, ws_bytes, Q.stream))
            for _ in range(args.rounds + 1)][1:]
    ws.free()
    # the two older streams of the same session: the plain surrogate's loss kernel and the column scaling
    P.disable_target()
    P.set_column_weights(np.full(B, 0.5, np.float32))
    P.step_resident()
    for _ in range(args.rounds):
        profiled(P, args.steps, OFF_TAGS, us)
    for L in (P, Q):
        L.close()
    bpr = bytes_per_row(A)
    moved = dict(kl_penalty=16 * n, target_loss=(bpr["surrogate_loss"] + 4 * A) * T * B, surrogate_loss=bpr["surrogate_loss"] * T * B,
                 scale_columns=8 * n + 8 * T * B)

    def entry(v, k):
        e = dict(us_per_launch=spread(v))
        if k in moved:
            floor = moved[k] / HBM_BYTES_PER_S * 1e6
            e.update(bytes_moved=moved[k], floor_us=round(floor, 3), over_floor=round(statistics.median(v) / floor, 3))
        return e

    kernels = {k: entry(v, k) for k, v in us.items() if v}
    extra = [b - a for a, b in zip(ms["off"], ms["on"])]
    step = dict(policy="atari", objective="surrogate, target period 1", reference="target", pairs=args.pairs,
                off_ms_per_step=spread(ms["off"]), on_ms_per_step=spread(ms["on"]), on_minus_off_ms=spread(extra))
    res = dict(what="the adaptive KL penalty (fi_kl.h) on the Atari policy at T = 100, B = 4096, A = 18: the "
                    "surrogate-with-target step with and without it in alternated pairs, every launch by itself from the "
                    "step's launch tags beside the older streams of the same session, and the penalty kernel alone in "
                    "bursts; first measurement, no threshold",
               T=T, B=B, A=A, hbm_bytes_per_s=HBM_BYTES_PER_S, workspace_bytes=ws_bytes, step=step, kernels=kernels,
               burst=dict(kl_penalty=entry(took, "kl_penalty")), kl_state=state, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
