#!/usr/bin/env python3
"""First measurement of the optimiser kernels alone, at the Atari policy's parameter count, on one
device (include/fi_train.h).

  rmsprop   fi_train_rmsprop_update without momentum (p, g, v: 20 bytes per element) and with momentum
            0.9 (p, g, v, m: 28 bytes per element), by HIP events around bursts of launches after
            warm-up, beside the floors bytes / 6.3 TB/s. One set of buffers stays in the 256 MB Infinity
            Cache between launches (a warm figure); `--sets` disjoint copies, taken in turn, push every
            launch's tensors out of it before their turn comes again (the HBM figure).
  adam      adam_kernel through a learner's own "optimizer" tag: an Atari learner (A = 18, T = 2,
            B = 5) with profiling on, the mean of the event pair around the kernel over `--steps`
            resident steps. Inside a step the gradient was written just before and the parameters
            are read just after, so this is a warm figure; 28 bytes per element.

A first measurement: the floors stand beside the figures, there is no bar. Prints one JSON line and
writes it to profiles/optimizer_rmsprop.json.

    python scripts/optimizer_bench.py [--out profiles/optimizer_rmsprop.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import _abi, build_info, hip, train  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_TBS = 6.3


def spread(v) -> dict:
    a = np.asarray(v, np.float64)
    return dict(mean=round(float(a.mean()), 4), median=round(float(np.median(a)), 4), min=round(float(a.min()), 4),
                max=round(float(a.max()), 4), std=round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), n=int(a.size))


def rmsprop_alone(n: int, momentum: float, sets: int, bursts: int, per_burst: int) -> dict:
    """us per launch: `bursts` event pairs around `per_burst` launches each."""
    rs = np.random.RandomState(0)
    p, g = rs.standard_normal(n).astype(np.float32), (rs.standard_normal(n) * 0.1).astype(np.float32)
    zero = np.zeros(n, np.float32)
    bufs = [tuple(hip.DeviceBuffer.from_array(a) for a in (p, g, zero, zero)) for _ in range(sets)]
    k = 0

    def launch():
        nonlocal k
        bp, bg, bv, bm = bufs[k % sets]
        train.rmsprop_update(bp.ptr, bg.ptr, bv.ptr, bm.ptr, n, 1e-6, 0.99, momentum, 0.01)
        k += 1

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
    for t in bufs:
        for b in t:
            b.free()
    return dict(sets=sets, set_bytes=4 * n * (4 if momentum else 3), launches_per_burst=per_burst, us_per_launch=spread(us),
                us_per_launch_all=[round(x, 3) for x in us])


def adam_in_step(steps: int) -> dict:
    L = DeviceLearner("atari", seq_len=2, batch=5, num_actions=18, optimizer="adam", seed=1)
    L.synth(seed=3)
    for _ in range(3):
        L.step_resident()
    L.set_profiling(True)
    for _ in range(steps):
        L.step_resident()
    buf, ms, cnt = C.create_string_buffer(8192), (C.c_float * 128)(), (C.c_int * 128)()
    k = _abi.lib().fi_learner_kernel_times(L._h, buf, 8192, ms, cnt, 128)
    names = buf.value.decode().split("\n")[:k]
    i = names.index("optimizer")
    out = dict(param_count=L.param_count, steps=int(cnt[i]), us_per_launch_mean=round(float(ms[i]) * 1e3, 3))
    L.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_rmsprop.json"))
    ap.add_argument("--sets", type=int, default=12, help="disjoint buffer sets of the HBM figure (12 x 20 MB or more > 256 MB)")
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("optimizer_bench: no HIP device; nothing is measured without one")
    adam = adam_in_step(args.steps)
    n = adam["param_count"]

    def floor_us(bytes_per_element):
        return round(n * bytes_per_element / (HBM_TBS * 1e12) * 1e6, 3)

    rows = {}
    for name, momentum, bpe in (("rmsprop", 0.0, 20), ("rmsprop_momentum", 0.9, 28)):
        rows[name] = dict(momentum=momentum, bytes_per_element=bpe, bytes_moved=n * bpe, floor_us=floor_us(bpe),
                          warm=rmsprop_alone(n, momentum, 1, args.bursts, 20),
                          rotating=rmsprop_alone(n, momentum, args.sets, args.bursts, 2 * args.sets))
    rows["adam_in_step"] = dict(adam, bytes_per_element=28, bytes_moved=n * 28, floor_us=floor_us(28),
                                note="the learner's optimizer tag under profiling: warm, inside a step")
    res = dict(what="first measurement: the optimiser kernels alone at the Atari policy's parameter count, beside their HBM "
                    "floors; no bar",
               param_count=n, hbm_tbs=HBM_TBS, source_hash=build_info.source_hash(), kernels=rows)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
