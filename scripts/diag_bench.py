#!/usr/bin/env python3
"""First measurement of the off-policy diagnostics (include/fi_diag.h): offpolicy_diag_kernel plus its
finalize kernel beside the fused V-trace kernel on the same tensors, alternated in one session, at the
workload's shape (T = 100, B = 4096, A = 18) and at the training scripts' (T = 20, B = 256, A = 3).

Per shape an MLP learner steps its synthetic batch once, so its loss tensors hold a step's values. Then,
after a warm-up, `--rounds` rounds; a round times `--launches` back-to-back launches of V-trace
(DeviceLearner.replay_vtrace: no loss finalisation, one kernel) between two HIP events, then as many
of the diagnostics (two kernels per launch: the reduction and the one-workgroup finalize). Warm: every
launch reads the learner's own tensors, which stay in the Infinity Cache. Cold: the launches rotate
over 3 copies of the inputs (the workspace and outputs too), so each finds its tensors evicted. The
figure is microseconds per launch (median / min / max over the rounds) against bytes / 6.3 TB/s, the
achievable HBM rate README uses; the diagnostics read (8 A + 24) bytes per (t, b), V-trace moves
(12 A + 28). The launches go through ctypes, so at the small shape a per-launch figure is the host's
submission rate, not the kernels' time.

Then the added wall time of `--diagnostics 1` in scripts/train_breakout.py: its default loop (Adam,
host publication) run for `--train-unrolls` unrolls with diagnostics off and on, alternated.

A first measurement with no acceptance threshold. Prints one JSON line and writes it to
profiles/offpolicy_diag.json.

    python scripts/diag_bench.py [--out profiles/offpolicy_diag.json] [--rounds 10] [--launches 50] [--train-unrolls 200]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from freeimpala_amd import build_info, diag, hip  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPES = [(100, 4096, 18), (20, 256, 3)]
INPUTS = ("logits", "mu", "actions", "rewards", "discounts", "values", "vs")


def spread(us: list[float]) -> dict:
    return dict(median=round(statistics.median(us), 3), min=round(min(us), 3), max=round(max(us), 3))


class DiagReplay:
    """The diagnostics on a learner's tensors, or rotating over `sets` copies of them."""

    def __init__(self, L: DeviceLearner, sets: int):
        self.L, self.owned = L, []
        base = {k: L.tensor_ptr(k) for k in INPUTS}
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
        self.ws_bytes = diag.workspace_bytes(L.T, L.B, L.A)
        self.ws = [hip.DeviceBuffer(self.ws_bytes) for _ in self.sets]
        self.out = [hip.DeviceBuffer(160 + 8 * L.B) for _ in self.sets]
        self.owned += self.ws + self.out

    def launch(self, i: int) -> None:
        L, k = self.L, i % len(self.sets)
        p, out = self.sets[k], self.out[k].ptr
        diag.offpolicy_diag_dev(L.T, L.B, L.A, p["logits"], p["mu"], p["actions"], p["rewards"], p["discounts"],
                                p["values"], p["vs"], L.cfg.hp, out, out + 160, out + 160 + 4 * L.B, self.ws[k].ptr,
                                self.ws_bytes, L.stream)

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


def kernels(T: int, B: int, A: int, rounds: int, launches: int) -> dict:
    L = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=A, seed=1)
    L.synth(seed=1)
    L.step_resident()
    res = {}
    for name, sets in (("warm", 1), ("cold", 3)):
        rep = DiagReplay(L, sets)
        rep.burst_us(max(3, sets))
        out = dict(vtrace=[], diagnostics=[])
        for r in range(rounds + 1):  # round 0 warms both up
            v = L.replay_vtrace(launches, sets) * 1e3
            d = rep.burst_us(launches)
            if r:
                out["vtrace"].append(v)
                out["diagnostics"].append(d)
        rep.free()
        res[name] = dict(vtrace=spread(out["vtrace"]), diagnostics=spread(out["diagnostics"]))
    summary = L.diagnostics()
    L.close()
    ct, ts = diag.plan(T, B, A)
    bytes_diag, bytes_vt = (8 * A + 24) * T * B, (12 * A + 28) * T * B
    return dict(T=T, B=B, A=A, grid=dict(column_tiles=ct, time_slices=ts, workgroups=ct * ts),
                workspace_bytes=diag.workspace_bytes(T, B, A),
                diagnostics_bytes=bytes_diag, diagnostics_floor_us=round(bytes_diag / HBM_BYTES_PER_S * 1e6, 3),
                vtrace_bytes=bytes_vt, vtrace_floor_us=round(bytes_vt / HBM_BYTES_PER_S * 1e6, 3),
                us_per_launch=res, summary_of_the_step=diag.brief(summary))


def training(unrolls: int, window: int, blocks: int = 2) -> dict:
    import train_breakout as tb
    out = dict(off=[], on=[])
    for _ in range(blocks):
        for name, every in (("off", 0), ("on", 1)):
            out[name].append(tb.train("adam", unrolls, window, "host", None, every)["wall_s"])
    off, on = statistics.median(out["off"]), statistics.median(out["on"])
    return dict(script="train_breakout.py, Adam, host publication", unrolls=unrolls, wall_s_diagnostics_off=out["off"],
                wall_s_diagnostics_1=out["on"], added_ms_per_unroll=round((on - off) / unrolls * 1e3, 4))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offpolicy_diag.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--train-unrolls", type=int, default=200)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("diag_bench: no HIP device; nothing is measured without one")
    res = dict(what="offpolicy_diag_kernel + finalize (fi_diag.h) and the fused V-trace kernel alternated in one session on "
                    "the same tensors: us per launch from HIP events around back-to-back launches, warm (the learner's "
                    "own tensors) and cold (3 rotating copies), against bytes / 6.3 TB/s; then the wall time "
                    "train_breakout.py gains with --diagnostics 1; first measurement, no threshold",
               hbm_bytes_per_s=HBM_BYTES_PER_S, rounds=args.rounds, launches_per_round=args.launches,
               kernels=[kernels(*s, args.rounds, args.launches) for s in SHAPES],
               training=training(args.train_unrolls, max(1, args.train_unrolls // 2)) if args.train_unrolls else None,
               source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
