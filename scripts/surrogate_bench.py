#!/usr/bin/env python3
"""First measurement of the clipped surrogate objective's kernels (include/fi_surrogate.h) on one device,
at T = 100, B = 4096, A = 18.

  sequence  fi_surrogate_loss_fp32 (rows, scan, loss and stats kernels) and the fused V-trace kernel on the
            same tensors of one learner, alternated window by window in one session: us per launch sequence
            from HIP events around back-to-back launches, warm (the learner's own tensors) and cold (3
            rotating copies, past the 256 MB Infinity Cache), median / min / max over the windows.
  kernels   each launch by itself, from the step's own launch tags (an event pair around every launch): two
            MLP learners of the same parameters and batch, one with the objective on, profiled in windows
            of `--steps` steps taken in turn; us per launch, median / min / max over the windows, beside
            the bytes the kernel moves at 6.3 TB/s. Inside a step the tensors come from the forward that
            ran just before, so these are neither the warm nor the cold figure of `sequence`.
  step      ms per step of the two handles, pair by pair.

Prints one JSON line and writes it to profiles/surrogate_kernels.json (kept: "plain_step", which
scripts/ab_rounds.sh against the parent commit's library fills in).

    python scripts/surrogate_bench.py [--out profiles/surrogate_kernels.json] [--rounds 10] [--launches 50]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import _abi, build_info, hip, surrogate  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
T, B, A = 100, 4096, 18
INPUTS = ("logits", "mu", "actions", "rewards", "discounts", "values")
OUTPUTS = ("vs", "pg_adv", "dlogits", "dvalue")
TAGS = ("surrogate_rows", "surrogate_scan", "surrogate_loss", "surrogate_stats")


def spread(us: list[float]) -> dict:
    return dict(median=round(statistics.median(us), 3), min=round(min(us), 3), max=round(max(us), 3))


def bytes_per_row(a: int) -> dict:
    """What each kernel reads and writes per (t, b): rows pi, mu, act, rew, disc, V, V' -> d, k, log rho; scan d,
    k, rew, disc, V -> vs, A; loss pi, act, log rho, A, V, vs -> dlogits, dvalue."""
    return dict(surrogate_rows=8 * a + 20 + 12, surrogate_scan=20 + 8, surrogate_loss=4 * a + 20 + 4 * a + 4,
                vtrace=12 * a + 28)


class Replay:
    """fi_surrogate_loss_fp32 on a learner's tensors, or rotating over `sets` copies of them."""

    def __init__(self, L: DeviceLearner, sets: int, normalize: bool):
        self.L, self.owned = L, []
        base = {k: L.tensor_ptr(k) for k in INPUTS + OUTPUTS}
        self.sets = [{k: v[0] for k, v in base.items()}]
        L.sync()
        for _ in range(1, sets):
            d = {}
            for k, (ptr, nb) in base.items():
                buf = hip.DeviceBuffer(nb)
                hip.copy_d2d(buf.ptr, ptr, nb)
                self.owned.append(buf)
                d[k] = buf.ptr
            self.sets.append(d)
        self.ws_bytes = surrogate.workspace_bytes(L.T, L.B, L.A)
        self.ws = [hip.DeviceBuffer(self.ws_bytes) for _ in self.sets]
        self.stats = hip.DeviceBuffer(32)
        self.owned += self.ws + [self.stats]
        self.prm = surrogate.params(surrogate.CLIP, normalize)

    def launch(self, i: int) -> None:
        L, k = self.L, i % len(self.sets)
        p = self.sets[k]
        surrogate.surrogate_loss_dev(L.T, L.B, L.A, p["logits"], p["mu"], p["actions"], p["rewards"], p["discounts"],
                                     p["values"], L.cfg.hp, self.prm, p["vs"], p["pg_adv"], p["dlogits"], p["dvalue"], None,
                                     self.stats.ptr, self.ws[k].ptr, self.ws_bytes, None, L.stream)

    def burst_us(self, n: int) -> float:
        e0, e1 = hip.Event(), hip.Event()
        e0.record(self.L.stream)
        for i in range(n):
            self.launch(i)
        e1.record(self.L.stream)
        self.L.sync()
        return e0.elapsed_ms(e1) * 1e3 / n

    def free(self) -> None:
        for b in self.owned:
            b.free()


def sequence(L: DeviceLearner, rounds: int, launches: int) -> dict:
    res = {}
    for name, sets in (("warm", 1), ("cold", 3)):
        reps = {nm: Replay(L, sets, nz) for nm, nz in (("surrogate", False), ("surrogate_normalized", True))}
        out = {k: [] for k in ["vtrace", *reps]}
        for r in range(rounds + 1):  # round 0 warms everything up
            got = dict(vtrace=L.replay_vtrace(launches, sets) * 1e3)
            got.update({nm: rep.burst_us(launches) for nm, rep in reps.items()})
            if r:
                for k, v in got.items():
                    out[k].append(v)
        for rep in reps.values():
            rep.free()
        res[name] = {k: spread(v) for k, v in out.items()}
    return res


def kernel_times(L: DeviceLearner) -> dict:
    buf = C.create_string_buffer(8192)
    ms, cnt = (C.c_float * 128)(), (C.c_int * 128)()
    n = _abi.lib().fi_learner_kernel_times(L._h, buf, 8192, ms, cnt, 128)
    return {nm: ms[i] * 1e3 for i, nm in enumerate(buf.value.decode().split("\n")[:n])}


def in_step(rounds: int, steps: int) -> tuple[dict, dict]:
    P = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, seed=1)
    Q = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, seed=1)
    Q.set_objective("surrogate", normalize_advantages=True)
    for L in (P, Q):
        L.synth(seed=1)
        L.step_resident()
    us = {k: [] for k in ("vtrace",) + TAGS}
    ms = dict(vtrace=[], surrogate=[])
    for r in range(rounds + 1):
        for L, name in ((P, "vtrace"), (Q, "surrogate")):
            L.set_profiling(True)
            took = [L.step_resident()["step_ms"] for _ in range(steps)]
            kt = kernel_times(L)
            L.set_profiling(False)
            if r:
                ms[name].append(statistics.median(took))
                for k in us:
                    if k in kt:
                        us[k].append(kt[k])
    state = Q.objective_state()
    for L in (P, Q):
        L.close()
    bpr = bytes_per_row(A)
    kernels = {}
    for k, v in us.items():
        kernels[k] = dict(us_per_launch=spread(v))
        if k in bpr:
            nb = bpr[k] * T * B
            kernels[k].update(bytes_moved=nb, floor_us=round(nb / HBM_BYTES_PER_S * 1e6, 3))
    step = dict(policy="mlp", profiled=True, steps_per_window=steps, vtrace_ms_per_step=spread(ms["vtrace"]),
                surrogate_ms_per_step=spread(ms["surrogate"]),
                surrogate_minus_vtrace_ms=spread([s - v for s, v in zip(ms["surrogate"], ms["vtrace"])]),
                objective_state=state)
    return kernels, step


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surrogate_kernels.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("surrogate_bench: no HIP device; nothing is measured without one")
    L = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, seed=1)
    L.synth(seed=1)
    L.step_resident()
    seq = sequence(L, args.rounds, args.launches)
    L.close()
    kernels, step = in_step(args.rounds, args.steps)
    bpr = bytes_per_row(A)
    total = sum(v for k, v in bpr.items() if k != "vtrace") * T * B
    res = dict(what="the surrogate objective's kernels (fi_surrogate.h) and the fused V-trace kernel alternated in one "
                    "session at T = 100, B = 4096, A = 18: the launch sequence warm and cold, then every launch by itself "
                    "from the step's launch tags, against bytes / 6.3 TB/s; first measurement, no threshold",
               T=T, B=B, A=A, hbm_bytes_per_s=HBM_BYTES_PER_S, rounds=args.rounds, launches_per_round=args.launches,
               grid=dict(rows_and_loss_workgroups=surrogate.loss_blocks(T, B, A), scan_workgroups=surrogate.scan_blocks(B)),
               workspace_bytes=surrogate.workspace_bytes(T, B, A),
               sequence_bytes=total, sequence_floor_us=round(total / HBM_BYTES_PER_S * 1e6, 3),
               vtrace_bytes=bpr["vtrace"] * T * B, vtrace_floor_us=round(bpr["vtrace"] * T * B / HBM_BYTES_PER_S * 1e6, 3),
               sequence_us=seq, kernels=kernels, step=step, source_hash=build_info.source_hash())
    if os.path.exists(args.out):  # the A/B against the parent commit is another script's: keep its figure
        try:
            old = json.load(open(args.out))
            if "plain_step" in old:
                res["plain_step"] = old["plain_step"]
        except ValueError:
            pass
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
