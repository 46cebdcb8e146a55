#!/usr/bin/env python3
"""First measurement of the PopArt kernels (include/fi_popart.h) on one device.

  kernels  the launches of a step with PopArt on, alone, at T = 100, B = 4096: fi_popart_denormalize over
           (T+1) B values, fi_popart_scale_grad over T B gradients, fi_popart_update over T B targets (the
           moments kernel and the one-workgroup finalize on a 512 x 19 head: the ABI launches them as a
           pair) and the same pair over 4 targets, where the moments kernel is one workgroup with nothing
           to read: the pair's launch floor, the finalize's share. HIP events around bursts of back-to-back
           launches after warm-up, on one buffer set (warm) and on `--sets` disjoint sets taken in turn.
           The sets are 1.6 MB each: in turn they leave the L2 but not the 256 MB Infinity Cache. Each is
           set beside its bytes at 6.3 TB/s: 1.64 MB read and written for the two streams, 1.64 MB read
           for the moments. sigma = 1, mu = 0 and beta = 0 keep every value what it is over any number of
           launches.
  steps    the Atari learner step on a resident synthetic batch with and without PopArt: two handles with
           the same parameters and batch, alternated step by step in one session; ms per step of each
           (the step's own HIP events) and the difference pair by pair with its spread. The statement "no
           regression" can only be read off the plain handle of this same run.

Prints one JSON line and writes it to profiles/popart_kernels.json.

    python scripts/popart_bench.py [--out profiles/popart_kernels.json] [--steps 20] [--batch 4096]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from freeimpala_amd import build_info, hip, popart  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402
from prio_bench import spread  # noqa: E402

HBM_TBS = 6.3
HEAD_H, HEAD_O = 512, 19


def burst_us(launch, sets: int, bursts: int, per_burst: int) -> dict:
    n = 0

    def go():
        nonlocal n
        launch(n % sets)
        n += 1

    for _ in range(max(3, sets)):
        go()
    hip.synchronize()
    us = []
    for _ in range(bursts):
        e0, e1 = hip.Event(), hip.Event()
        e0.record()
        for _ in range(per_burst):
            go()
        e1.record()
        us.append(e0.elapsed_ms(e1) * 1e3 / per_burst)
    return dict(sets=sets, launches_per_burst=per_burst, us_per_launch=spread(us), us_per_launch_all=[round(x, 3) for x in us])


def kernels(T: int, B: int, sets: int, bursts: int) -> dict:
    rs = np.random.RandomState(0)
    rows, TB = (T + 1) * B, T * B
    state = hip.DeviceBuffer.from_array(popart.pack_state(0.0, 1.0, 1.0))
    vals = [hip.DeviceBuffer.from_array(rs.standard_normal(rows).astype(np.float32)) for _ in range(sets)]
    head = [hip.DeviceBuffer.from_array(rs.standard_normal(HEAD_H * HEAD_O + HEAD_O).astype(np.float32)) for _ in range(sets)]
    ws = [hip.DeviceBuffer(popart.workspace_bytes(TB)) for _ in range(sets)]

    def update(n):
        def launch(i):
            popart.update(vals[i].ptr, n, state.ptr, head[i].ptr + 4 * (HEAD_O - 1), HEAD_O, HEAD_H,
                          head[i].ptr + 4 * (HEAD_H * HEAD_O + HEAD_O - 1), 0.0, ws_ptr=ws[i].ptr, ws_bytes=ws[i].nbytes)
        return launch

    cases = dict(
        denormalize=(lambda i: popart.denormalize(vals[i].ptr, rows, state.ptr), 2 * 4 * rows),
        scale_grad=(lambda i: popart.scale_grad(vals[i].ptr, TB, state.ptr), 2 * 4 * TB),
        update=(update(TB), 4 * TB),
        update_4_targets=(update(4), 16))
    out = {}
    for name, (launch, nbytes) in cases.items():
        out[name] = dict(bytes_moved=nbytes, floor_us=round(nbytes / (HBM_TBS * 1e12) * 1e6, 3),
                         warm=burst_us(launch, 1, bursts, 20), rotating=burst_us(launch, sets, bursts, 2 * sets))
    st = popart.unpack_state(state.download(np.uint8, (32,)))
    assert (st["mu"], st["nu"], st["sigma"]) == (0.0, 1.0, 1.0) and st["updates"] > 0
    for b in vals + head + ws + [state]:
        b.free()
    return dict(seq_len=T, batch=B, moments_workgroups=popart.plan(TB), head=[HEAD_H, HEAD_O], hbm_tbs=HBM_TBS, launches=out)


def steps(T: int, B: int, A: int, n_steps: int) -> dict:
    plain = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    pop = DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, seed=1)
    pop.enable_popart()
    for L in (plain, pop):
        L.synth(seed=7)
    for _ in range(3):
        for L in (plain, pop):
            L.step_resident()
    ms = dict(plain=[], popart=[])
    for _ in range(n_steps):
        ms["plain"].append(plain.step_resident()["step_ms"])
        ms["popart"].append(pop.step_resident()["step_ms"])
    st = pop.popart_state()
    pairs = np.asarray(ms["popart"]) - np.asarray(ms["plain"])
    for L in (plain, pop):
        L.close()
    return dict(seq_len=T, batch=B, num_actions=A, steps=n_steps, warmup_steps=3,
                plain_ms_per_step=spread(ms["plain"]), popart_ms_per_step=spread(ms["popart"]),
                popart_minus_plain_ms=spread(pairs), plain_ms_all=[round(x, 4) for x in ms["plain"]],
                popart_ms_all=[round(x, 4) for x in ms["popart"]], popart_state=st)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "popart_kernels.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    T, A = 100, 18
    res = dict(what="first measurement: the PopArt launches alone beside their bytes at 6.3 TB/s, and the Atari step with "
                    "and without PopArt, two handles alternated step by step in one session; no threshold",
               source_hash=build_info.source_hash(), kernels=kernels(T, 4096, args.sets, args.bursts))
    if not args.skip_steps:
        res["steps"] = steps(T, args.batch, A, args.steps)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
