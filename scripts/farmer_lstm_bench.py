#!/usr/bin/env python3
"""First measurement of FarmerLstm's bf16 LSTM mode (include/fi_farmer_lstm.h) on one device, at (B, T) = (32, 10)
(the reference's defaults), (512, 100) and (4096, 100).

  step         ms per resident train step in fp32 and in bf16 mode: two handles of the same parameters and batch in
               one process, stepped in turn, median / min / max over `--pairs` alternated pairs, and the pairwise
               difference with its spread. The fp32 handle never calls fi_farmer_set_lstm_precision: its step is the
               step as it was before there was a mode, so the baseline is the same build in the same session.
  recurrence   fi_farmer_recurrence_ms of both handles: the forward recurrence and the BPTT kernel by themselves.

Prints one JSON line and writes it to profiles/farmer_lstm_bf16.json.

    python scripts/farmer_lstm_bench.py [--out profiles/farmer_lstm_bf16.json] [--pairs 20] [--shapes 32x10,512x100,4096x100]

--activation-error instead prints the figure tests/test_gpu_farmer_lstm_bf16.py builds its activation allowance on:
the largest relative error of the fp32 kernel's gates and c at (70, 5) against fp64 from its own xp and hprev.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from freeimpala_amd import build_info, farmer, hip  # noqa: E402
from surrogate_bench import spread  # noqa: E402


def activation_error() -> None:
    from freeimpala_amd import farmer_lstm as FL
    from test_gpu_farmer_lstm_bf16 import act, step
    B, T, H = 70, 5, 128
    M, p0, _ = step(B, T, prec=None)
    xp, c, gates, hp = (M.tensor_array(n, (B, T, w)).astype(np.float64)
                        for n, w in (("xp", 512), ("cst", H), ("gates", 512), ("hprev", H)))
    M.close()
    pre = xp + hp @ FL.split_lstm_params(p0)["W_hh"].T
    ref = np.concatenate([act(k, pre[..., k * H:(k + 1) * H]) for k in range(4)], -1)
    cprev = np.concatenate([np.zeros((B, 1, H)), c[:, :-1]], 1)
    cref = ref[..., H:2 * H] * cprev + ref[..., :H] * ref[..., 2 * H:3 * H]
    print(json.dumps(dict(what="fp32 recurrence at (70, 5): largest relative error of the stored gates and c against "
                               "fp64 from the kernel's own xp and hprev",
                          gates=float(np.max(np.abs(gates - ref) / np.abs(ref))),
                          c=float(np.max(np.abs(c - cref) / np.abs(cref))))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "farmer_lstm_bf16.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--shapes", default="32x10,512x100,4096x100")
    ap.add_argument("--activation-error", action="store_true")
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("farmer_lstm_bench: no HIP device; nothing is measured without one")
    if args.activation_error:
        return activation_error()
    from oracle import farmer_oracle as fo
    shapes = {}
    for spec in args.shapes.split(","):
        B, T = (int(v) for v in spec.split("x"))
        p0 = fo.gen_params(1)
        z, x, y = fo.gen_inputs(2, B, T)
        L = {k: farmer.FarmerLstmModel(B, T, "mse", "adam", 1e-3, params=p0) for k in ("fp32", "bf16")}
        L["bf16"].set_lstm_precision("bf16")
        for X in L.values():
            X.upload_inputs(z, x, y)
            for _ in range(3):  # warm both up
                X.train_step_resident()
        ms = dict(fp32=[], bf16=[])
        for _ in range(args.pairs):
            for k, X in L.items():
                X.train_step_resident()
                ms[k].append(X.last_step_ms)
        rec = {k: dict(zip(("fwd_ms", "bwd_ms"), (round(v, 4) for v in X.recurrence_ms(5)))) for k, X in L.items()}
        for X in L.values():
            X.close()
        diff = [b - a for a, b in zip(ms["fp32"], ms["bf16"])]
        med = spread(ms["bf16"])["median"]
        shapes[spec] = dict(B=B, T=T, fp32_ms_per_step=spread(ms["fp32"]), bf16_ms_per_step=spread(ms["bf16"]),
                            bf16_minus_fp32_ms=spread(diff), recurrence_ms=rec,
                            fp32_samples_per_s=round(B / spread(ms["fp32"])["median"] * 1e3, 1),
                            bf16_samples_per_s=round(B / med * 1e3, 1))
    res = dict(what="FarmerLstm's bf16 LSTM mode (fi_farmer_lstm.h): the resident train step (device ms, HIP events) in fp32 "
                    "and in bf16 mode in alternated pairs of one process, and the two recurrence kernels by themselves "
                    "(fi_farmer_recurrence_ms); first measurement, no threshold",
               pairs=args.pairs, shapes=shapes, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
