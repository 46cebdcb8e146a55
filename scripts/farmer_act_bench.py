#!/usr/bin/env python3
"""First measurement of FarmerLstm's device actor (include/fi_farmer_act.h) on one device, at S decision points of n
candidate rows each and T = 10: 1 x 32, 256 x 16 and 4096 x 16.

  new     one fi_farmer_actor_act call on resident inputs: host ms around the call (it ends in the one wait for the
          results), device ms of the call (HIP events on the handle's stream before and behind it) and of its LSTM,
          torso and pick launches (fi_farmer_actor_kernel_ms).
  old     the only route there was before: FarmerLstmModel(N, T) forward on resident inputs, z repeated for every
          candidate, the N values copied to the host and the argmax per decision point taken there; host ms around
          it (fi_farmer_forward ends in a wait too). Code this measurement's subject does not touch.

Both in one process, warmed up, in `--pairs` alternated pairs: median / min / max. Decisions and candidate rows per
second come from the host ms of a call, which is what an acting loop pays. weight_bytes_from_l2 is what the torso's
workgroups read of the bf16 images per call, from the shapes: one pass over all five images per 64-row tile.

Prints one JSON line and writes it to profiles/farmer_act.json.

    python scripts/farmer_act_bench.py [--out profiles/farmer_act.json] [--pairs 20] [--shapes 1x32,256x16,4096x16]
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

from freeimpala_amd import build_info, farmer, farmer_act, hip  # noqa: E402
from surrogate_bench import spread  # noqa: E402

T = 10
IMAGE_BYTES = 2 * (512 * 624 + 4 * 512 * 512)  # the five bf16 images of the torso


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "farmer_act.json"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--shapes", default="1x32,256x16,4096x16")
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("farmer_act_bench: no HIP device; nothing is measured without one")
    from oracle import farmer_oracle as fo
    p0 = fo.gen_params(1)
    shapes = {}
    for spec in args.shapes.split(","):
        S, n = (int(v) for v in spec.split("x"))
        N = S * n
        rs = np.random.RandomState(S + n)
        z = rs.standard_normal((S, T, 162)).astype(np.float32)
        x = rs.standard_normal((N, 484)).astype(np.float32)
        offsets = np.arange(S + 1, dtype=np.int32) * n
        A = farmer_act.FarmerActor(S, N, T, seed=1)
        A.set_params(p0)
        A.set_profiling(True)
        zd, xd = hip.DeviceBuffer.from_array(z), hip.DeviceBuffer.from_array(x)
        M = farmer.FarmerLstmModel(N, T, params=p0)
        M.upload_inputs(np.repeat(z, n, axis=0), x, np.zeros((N, 1), np.float32))
        mz, mx = M.tensor("z")[0], M.tensor("x")[0]
        vals = np.empty(N, np.float32)
        e0, e1, stream = hip.Event(), hip.Event(), farmer_act.lib().fi_farmer_actor_stream(A._h)

        def new():
            e0.record(stream)
            t0 = time.perf_counter()
            out = A.act(zd.ptr, xd.ptr, offsets, 0.0, on_device=True)
            host = (time.perf_counter() - t0) * 1e3
            e1.record(stream)
            return out, dict(host=host, device=e0.elapsed_ms(e1), **A.kernel_ms())

        def old():
            t0 = time.perf_counter()
            rc = farmer.lib().fi_farmer_forward(M._h, mz, mx, 1, vals.ctypes.data)
            act = vals.reshape(S, n).argmax(1)
            host = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rc
            return act, host

        for _ in range(3):  # warm both up
            got, _ = new()
            want, _ = old()
        ms = dict(host=[], device=[], lstm=[], torso=[], pick=[], old_host=[])
        for _ in range(args.pairs):
            _, t = new()
            for k, v in t.items():
                ms[k].append(v)
            ms["old_host"].append(old()[1])
        A.close()
        M.close()
        new_ms, old_ms = spread(ms["host"])["median"], spread(ms["old_host"])["median"]
        shapes[spec] = dict(
            S=S, rows_per_state=n, N=N, T=T,
            new_host_ms_per_call=spread(ms["host"]), new_device_ms_per_call=spread(ms["device"]),
            new_kernel_ms={k: spread(ms[k]) for k in ("lstm", "torso", "pick")},
            old_host_ms_per_call=spread(ms["old_host"]),
            old_minus_new_host_ms=spread([b - a for a, b in zip(ms["host"], ms["old_host"])]),
            new_decisions_per_s=round(S / new_ms * 1e3, 1), new_rows_per_s=round(N / new_ms * 1e3, 1),
            old_decisions_per_s=round(S / old_ms * 1e3, 1), old_rows_per_s=round(N / old_ms * 1e3, 1),
            weight_bytes_from_l2=-(-N // 64) * IMAGE_BYTES,
            # bf16 torso and LSTM against the fp32 forward: the share of decision points where both routes agree
            same_action_share=round(float((got["actions"] == want).mean()), 4))
    res = dict(what="FarmerLstm's device actor (fi_farmer_act.h): one act call on resident inputs beside the fp32 forward on z "
                    "repeated per candidate plus the host argmax, alternated pairs of one process; host ms around each "
                    "call, device ms by HIP events; first measurement, no threshold",
               pairs=args.pairs, shapes=shapes, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
