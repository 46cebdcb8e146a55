#!/usr/bin/env python3
"""First measurement of the V-MPO objective (include/fi_vmpo.h) on one device, on the Atari policy at T = 100,
B = 4096, A = 18. No threshold.

  step     ms per step with the V-MPO objective against the surrogate step: two learners of the same seed and batch
           stepped in turn, median / min / max over `--pairs` alternated pairs of unprofiled steps, and the pairwise
           difference.
  kernels  every launch by itself, from the step's own launch tags, the handles profiled in turn: the V-MPO step's
           surrogate_rows, surrogate_scan, vmpo_clear, vmpo_hist0..2, vmpo_sums, vmpo_loss and vmpo_eta, and the
           surrogate step's four launches of the same session, each with the bytes it moves at 6.3 TB/s and the ratio of
           its time to that. The selection's launches move 4 bytes per row (and the histograms): they are bound by the
           launch, not by the bytes, and the ratio says by how much.

Prints one JSON line and writes it to profiles/vmpo_kernels.json.

    python scripts/vmpo_bench.py [--out profiles/vmpo_kernels.json] [--pairs 20] [--steps 5] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, hip, vmpo  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from kl_bench import profiled  # noqa: E402
from surrogate_bench import HBM_BYTES_PER_S, TAGS as SURROGATE_TAGS, bytes_per_row, spread  # noqa: E402

T, B, A = 100, 4096, 18
SELECT_TAGS = ("vmpo_clear", "vmpo_hist0", "vmpo_hist1", "vmpo_hist2", "vmpo_sums")
VMPO_TAGS = ("surrogate_rows", "surrogate_scan") + SELECT_TAGS + ("vmpo_loss", "vmpo_eta")
HIST_BYTES = 3 * 2048 * 4


def bytes_moved() -> dict:
    """Per launch. A histogram pass reads the advantages and, in every workgroup, the earlier histograms; the flush is
    bounded by one histogram per workgroup and not counted. The loss reads pi, act, adv, V, vs and writes dlogits, dvalue."""
    n, g = T * B, vmpo.select_blocks(T * B)
    bpr = bytes_per_row(A)
    m = {k: bpr[k] * n for k in SURROGATE_TAGS if k in bpr}
    m.update(vmpo_clear=HIST_BYTES + 256, vmpo_hist0=4 * n, vmpo_hist1=4 * n + g * 8192, vmpo_hist2=4 * n + g * 2 * 8192,
             vmpo_sums=4 * n + g * (3 * 8192 + 16), vmpo_loss=(8 * A + 20) * n, vmpo_eta=vmpo.STATE_BYTES)
    return m


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vmpo_kernels.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("vmpo_bench: no HIP device; nothing is measured without one")
    P = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    Q = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    P.set_objective("surrogate")
    Q.set_objective("vmpo")
    for L in (P, Q):
        L.synth(seed=1)
    for _ in range(3):  # warm both up
        for L in (P, Q):
            L.step_resident()
    ms = dict(surrogate=[], vmpo=[])
    for _ in range(args.pairs):
        for L, name in ((P, "surrogate"), (Q, "vmpo")):
            ms[name].append(L.step_resident()["step_ms"])
    us = dict(vmpo={k: [] for k in VMPO_TAGS}, surrogate={k: [] for k in SURROGATE_TAGS})
    for _ in range(args.rounds):  # the handles in turn, so that both see the same session
        profiled(Q, args.steps, VMPO_TAGS, us["vmpo"])
        profiled(P, args.steps, SURROGATE_TAGS, us["surrogate"])
    state = Q.vmpo_state()
    for L in (P, Q):
        L.close()
    moved = bytes_moved()

    def entry(v, k):
        e = dict(us_per_launch=spread(v))
        if k in moved:
            floor = moved[k] / HBM_BYTES_PER_S * 1e6
            e.update(bytes_moved=moved[k], floor_us=round(floor, 3), over_floor=round(statistics.median(v) / floor, 3))
        return e

    kernels = {side: {k: entry(v, k) for k, v in tags.items() if v} for side, tags in us.items()}
    objective_us = {side: round(sum(statistics.median(v) for k, v in tags.items() if v and k != "vmpo_eta"), 3)
                    for side, tags in us.items()}
    extra = [b - a for a, b in zip(ms["surrogate"], ms["vmpo"])]
    step = dict(policy="atari", pairs=args.pairs, surrogate_ms_per_step=spread(ms["surrogate"]),
                vmpo_ms_per_step=spread(ms["vmpo"]), vmpo_minus_surrogate_ms=spread(extra))
    res = dict(what="the V-MPO objective (fi_vmpo.h) on the Atari policy at T = 100, B = 4096, A = 18: every launch by itself "
                    "from the step's launch tags beside the surrogate's four of the same session, and the step with either "
                    "objective in alternated pairs; first measurement, no threshold",
               T=T, B=B, A=A, hbm_bytes_per_s=HBM_BYTES_PER_S, select_blocks=vmpo.select_blocks(T * B),
               workspace_bytes=vmpo.workspace_bytes(T, B, A), step=step, kernels=kernels,
               objective_launches_us=objective_us, vmpo_state=state, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
