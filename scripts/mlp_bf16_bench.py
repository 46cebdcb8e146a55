#!/usr/bin/env python3
"""First measurement of the MLP policy's bf16 mode (include/fi_mlp.h) on one device, at T = 100, B = 4096, A = 18
(config #2: 128 -> 256 -> 256 -> heads).

  step     ms per resident step in fp32 and in bf16 mode: two learners of the same seed and batch in one process,
           stepped in turn, median / min / max over `--pairs` alternated pairs of unprofiled steps, and the pairwise
           difference with its spread. The fp32 handle never calls fi_learner_set_mlp_precision: its step is the
           step as it was before there was a mode, so the baseline is the same build in the same session.
  kernels  every launch by itself, from each handle's own launch tags (set_profiling), the handles profiled in turn.

Prints one JSON line and writes it to profiles/mlp_bf16.json.

    python scripts/mlp_bf16_bench.py [--out profiles/mlp_bf16.json] [--pairs 20] [--steps 5] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, hip  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from surrogate_bench import kernel_times, spread  # noqa: E402

T, B, A, D, H = 100, 4096, 18, 128, 256


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bf16.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("mlp_bf16_bench: no HIP device; nothing is measured without one")
    L = {k: DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, obs_dim=D, hidden=H, seed=1) for k in ("fp32", "bf16")}
    L["bf16"].set_mlp_precision("bf16")
    for X in L.values():
        X.synth(seed=1)
    for _ in range(3):  # warm both up
        for X in L.values():
            X.step_resident()
    ms = dict(fp32=[], bf16=[])
    for _ in range(args.pairs):
        for k, X in L.items():
            ms[k].append(X.step_resident()["step_ms"])
    us = dict(fp32={}, bf16={})
    for _ in range(args.rounds):
        for k, X in L.items():
            X.set_profiling(True)
            for _ in range(args.steps):
                X.step_resident()
            for tag, v in kernel_times(X).items():
                us[k].setdefault(tag, []).append(v)
            X.set_profiling(False)
    for X in L.values():
        X.close()
    diff = [b - a for a, b in zip(ms["fp32"], ms["bf16"])]
    res = dict(what="the MLP policy's bf16 mode (fi_mlp.h) at T = 100, B = 4096, A = 18, D = 128, H = 256: the resident step "
                    "in fp32 and in bf16 mode in alternated pairs of one process, and every launch by itself from the "
                    "launch tags; first measurement, no threshold",
               T=T, B=B, A=A, D=D, H=H, pairs=args.pairs, fp32_ms_per_step=spread(ms["fp32"]), bf16_ms_per_step=spread(ms["bf16"]),
               bf16_minus_fp32_ms=spread(diff),
               kernels_us={k: {tag: spread(v) for tag, v in d.items()} for k, d in us.items()},
               source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
