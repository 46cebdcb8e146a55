#!/usr/bin/env python3
"""First measurement of the learner's target network (include/fi_target.h) on one device, on the Atari policy at
T = 100, B = 4096, A = 18.

  step     ms per surrogate step with and without the target: two learners of the same seed and batch stepped in
           turn, median / min / max over `--pairs` alternated pairs of unprofiled steps, and the pairwise
           difference. Beside it the same session's forward phase time of the target-less handle
           (fi_learner_phase_times over `--steps` profiled steps): a target step adds one forward, two
           weights_bf16 launches and the loss kernel's own difference, so `extra_over_forward` is the yardstick.
  kernels  every launch by itself, from the step's own launch tags, the two handles profiled in turn: target_loss
           beside surrogate_loss (one more T * B * A stream), the target forward's three tags, target_update
           (period 1 on the target's handle, so every step has one) beside the bytes each moves at 6.3 TB/s.
  update   fi_target_update on the handle's own slabs in bursts, tau = 1 (read once, write once) and tau = 0.5
           (read twice, write once), beside a burst of publications (publish_params_kernel, the same count).

Prints one JSON line and writes it to profiles/target_network.json.

    python scripts/target_bench.py [--out profiles/target_network.json] [--pairs 20] [--steps 5] [--launches 50]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, hip, target  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from surrogate_bench import HBM_BYTES_PER_S, bytes_per_row, kernel_times, spread  # noqa: E402

T, B, A = 100, 4096, 18
TAGS = ("surrogate_rows", "surrogate_scan", "surrogate_loss", "surrogate_stats", "target_weights_bf16", "target_forward",
        "target_weights_back", "target_loss", "target_stats", "target_update", "weights_bf16")


def burst_us(L: DeviceLearner, n: int, launch) -> float:
    e0, e1 = hip.Event(), hip.Event()
    e0.record(L.stream)
    for _ in range(n):
        launch()
    e1.record(L.stream)
    L.sync()
    return e0.elapsed_ms(e1) * 1e3 / n


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_network.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("target_bench: no HIP device; nothing is measured without one")
    P = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    Q = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    for L in (P, Q):
        L.set_objective("surrogate")
        L.synth(seed=1)
    Q.enable_target(period=1)
    for _ in range(3):  # warm both up
        for L in (P, Q):
            L.step_resident()
    ms = dict(surrogate=[], target=[])
    for _ in range(args.pairs):
        for L, name in ((P, "surrogate"), (Q, "target")):
            ms[name].append(L.step_resident()["step_ms"])
    us = {k: [] for k in TAGS}
    fwd = []
    for _ in range(args.rounds):
        for L in (P, Q):
            L.set_profiling(True)
            for _ in range(args.steps):
                L.step_resident()
            kt = kernel_times(L)
            if L is P:
                fwd.append(L.phase_times()["forward"])
            L.set_profiling(False)
            for k in us:
                if k in kt and (L is Q) != (k == "surrogate_loss"):  # the plain handle gives surrogate_loss alone
                    us[k].append(kt[k])
    n = P.param_count
    bpr = bytes_per_row(A)
    moved = dict(surrogate_loss=bpr["surrogate_loss"] * T * B, target_loss=(bpr["surrogate_loss"] + 4 * A) * T * B,
                 target_update=8 * n)
    kernels = {}
    for k, v in us.items():
        if v:
            kernels[k] = dict(us_per_launch=spread(v))
            if k in moved:
                kernels[k].update(bytes_moved=moved[k], floor_us=round(moved[k] / HBM_BYTES_PER_S * 1e6, 3))
    src, dst = P.tensor_ptr("params")[0], Q.target_params_dev()  # two slabs of the same count on one device
    upd = {}
    for name, tau, nb in (("tau_1", 1.0, 8 * n), ("tau_half", 0.5, 12 * n)):
        took = [burst_us(Q, args.launches, lambda: target.target_update_dev(src, dst, n, tau, None, Q.stream))
                for _ in range(args.rounds + 1)][1:]
        upd[name] = dict(us_per_launch=spread(took), bytes_moved=nb, floor_us=round(nb / HBM_BYTES_PER_S * 1e6, 3))
    took = [burst_us(P, args.launches, P.publish) for _ in range(args.rounds + 1)][1:]
    upd["publish_params"] = dict(us_per_launch=spread(took), bytes_moved=8 * n, floor_us=round(8 * n / HBM_BYTES_PER_S * 1e6, 3))
    state = Q.target_state()
    for L in (P, Q):
        L.close()
    extra = [t - s for s, t in zip(ms["surrogate"], ms["target"])]
    f = statistics.median(fwd)
    step = dict(policy="atari", pairs=args.pairs, surrogate_ms_per_step=spread(ms["surrogate"]),
                target_ms_per_step=spread(ms["target"]), target_minus_surrogate_ms=spread(extra),
                forward_phase_ms=spread(fwd), extra_over_forward=round(statistics.median(extra) / f, 4),
                loss_kernel_difference_us=(round(statistics.median(us["target_loss"]) - statistics.median(us["surrogate_loss"]), 3)
                                           if us["target_loss"] and us["surrogate_loss"] else None))
    res = dict(what="the target network (fi_target.h) on the Atari policy at T = 100, B = 4096, A = 18: the surrogate step "
                    "with and without it in alternated pairs beside the forward phase time of the same session, every "
                    "launch by itself from the step's launch tags, and the update kernel beside a publication; first "
                    "measurement, no threshold",
               T=T, B=B, A=A, params=n, hbm_bytes_per_s=HBM_BYTES_PER_S, workspace_bytes=target.workspace_bytes(T, B, A),
               step=step, kernels=kernels, update=upd, target_state=state, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
