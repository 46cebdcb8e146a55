#!/usr/bin/env python3
"""First measurements of parameter publication on the device (include/fi_publish.h), on one device.

  kernel   publish_params_kernel alone (fi_publish_copy) at the Atari policy's parameter count, both
           dtypes, by HIP events around bursts of launches after warm-up, beside the floor
           8 n bytes / 6.3 TB/s (n floats read, n written). One pair of buffers stays in the 256 MB
           Infinity Cache between launches (a warm figure); `--sets` disjoint pairs, taken in turn, push
           every launch's buffers out of it before their turn comes again (the HBM figure).
  loops    three loops on device Breakout, N = B = 256 and 1024, T = 20, A = 3, each with its own
           learner, actor and environment of the same seeds, alternated unroll by unroll in one
           session, `--warmup` (3) warm-up and `--unrolls` (20) timed unrolls each:
             host      rollout(T), step_rollouts, get_blob -> set_params          (the blob round trip)
             device    rollout(T), step_rollouts, publish -> set_params_dev
             overlap   rollout(T - 1), step_rollouts_async, publish -> set_params_dev, rollout(1)
           A timed unroll ends when the learner and the actor are idle (learner.wait(), actor.sync()),
           so nothing of one loop runs inside another loop's time. Wall ms per unroll as median
           (min / max), env-steps/s from the median, and batch_versions min / max / mean over the
           timed unrolls, and version_lag: the version the step updates minus the batch's mean version
           (0: on policy; the overlapped loop acts one version behind).

`device` removes two PCIe copies and two host waits from `host` and adds two launches, so its median
must not exceed `host`'s by more than the spread (max - min) of `host`'s own timed unrolls:
`device_within_host_spread` says whether that held. There is no bar on a speed-up. Prints one JSON
line and writes it to profiles/param_publish.json.

    python scripts/publish_bench.py [--out profiles/param_publish.json]
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

from freeimpala_amd import breakout, build_info, hip, publish  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_TBS = 6.3
T, A, GAMMA, SEED, MAX_STEPS = 20, 3, 0.99, 1, 1000


def spread(v) -> dict:
    a = np.asarray(v, np.float64)
    return dict(mean=round(float(a.mean()), 4), median=round(float(np.median(a)), 4), min=round(float(a.min()), 4),
                max=round(float(a.max()), 4), std=round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), n=int(a.size))


# ------------------------------------------------------------------ (i) the kernel alone
def kernel_alone(n: int, dtype: str, sets: int, bursts: int, per_burst: int) -> dict:
    """us per launch: `bursts` event pairs around `per_burst` launches each."""
    p = np.random.RandomState(0).standard_normal(n).astype(np.float32)
    bufs = [(hip.DeviceBuffer.from_array(p), hip.DeviceBuffer(4 * n)) for _ in range(sets)]
    k = 0

    def launch():
        nonlocal k
        src, dst = bufs[k % sets]
        publish.publish_copy(dst.ptr, src.ptr, n, dtype)
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
    return dict(sets=sets, set_bytes=8 * n, launches_per_burst=per_burst, us_per_launch=spread(us),
                us_per_launch_all=[round(x, 3) for x in us])


# ------------------------------------------------------------------ (ii) the three loops
class Loop:
    def __init__(self, mode: str, n: int):
        self.mode, self.n = mode, n
        self.L = DeviceLearner("atari", seq_len=T, batch=n, num_actions=A, records="planes", seed=SEED)
        self.a = Actor("atari", n, num_actions=A, seed=SEED)
        self.e = breakout.BreakoutEnv(n, GAMMA, seed=SEED, max_steps=MAX_STEPS)
        self.hand_over()
        self.a.begin_rollout(T)
        # overlap starts with a complete unroll, the other two with its step 0
        assert self.e.rollout(self.a, T + 1 if mode == "overlap" else 1) > 0
        self.drain()
        self.ms, self.versions, self.lag, self.steps = [], [], [], 0

    def hand_over(self) -> None:
        if self.mode == "host":
            blob, version = self.L.get_blob()
            self.a.set_params(blob, version)
        else:
            self.L.publish()
            self.a.set_params_dev(self.L)

    def drain(self) -> None:
        self.L.wait()
        self.a.sync()

    def unroll(self, timed: bool) -> None:
        L, a, e = self.L, self.a, self.e
        t0 = time.perf_counter()
        if self.mode == "overlap":
            assert e.rollout(a, T - 1) == T - 1
            L.step_rollouts_async([a])
            self.hand_over()
            assert e.rollout(a, 1) == 1
        else:
            assert e.rollout(a, T) == T
            L.step_rollouts([a])
            self.hand_over()
        self.drain()
        t1 = time.perf_counter()
        self.steps += 1
        if timed:
            self.ms.append((t1 - t0) * 1e3)
            bv = L.batch_versions
            self.versions.append((bv["min"], bv["max"], bv["mean"]))
            self.lag.append(self.steps - 1 - bv["mean"])  # the version this step updated, minus the batch's

    def result(self) -> dict:
        s = spread(self.ms)
        v = np.asarray(self.versions, np.float64)
        return dict(wall_ms_per_unroll=s, wall_ms_all=[round(x, 3) for x in self.ms],
                    env_steps_per_s=round(self.n * T / (s["median"] * 1e-3), 1),
                    batch_versions=dict(min=int(v[:, 0].min()), max=int(v[:, 1].max()), mean=round(float(v[:, 2].mean()), 3)),
                    version_lag=dict(min=round(min(self.lag), 3), max=round(max(self.lag), 3),
                                     mean=round(float(np.mean(self.lag)), 3)),
                    learner_version=self.L.wait()["version"], actor_version=self.a.version)

    def close(self) -> None:
        self.a.end_rollout()
        for h in (self.a, self.e, self.L):
            h.close()


def three_loops(n: int, warmup: int, unrolls: int) -> dict:
    loops = [Loop(m, n) for m in ("host", "device", "overlap")]
    for u in range(warmup + unrolls):
        for lp in loops:
            lp.unroll(u >= warmup)
    out = {lp.mode: lp.result() for lp in loops}
    for lp in loops:
        lp.close()
    h, d, o = (out[m]["wall_ms_per_unroll"] for m in ("host", "device", "overlap"))
    out["host_spread_ms"] = round(h["max"] - h["min"], 4)
    out["device_minus_host_median_ms"] = round(d["median"] - h["median"], 4)
    out["device_within_host_spread"] = bool(d["median"] - h["median"] <= h["max"] - h["min"])
    out["overlap_minus_device_median_ms"] = round(o["median"] - d["median"], 4)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_publish.json"))
    ap.add_argument("--sets", type=int, default=24, help="disjoint buffer pairs of the HBM figure (24 x 13.5 MB > 256 MB)")
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--unrolls", type=int, default=20)
    ap.add_argument("--envs", default="256,1024")
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("publish_bench: no HIP device; nothing is measured without one")
    probe = DeviceLearner("atari", seq_len=1, batch=1, num_actions=18, seed=1)
    n = probe.param_count
    probe.close()
    floor_us = round(8 * n / (HBM_TBS * 1e12) * 1e6, 3)
    kernel = {dt: dict(warm=kernel_alone(n, dt, 1, args.bursts, 20), rotating=kernel_alone(n, dt, args.sets, args.bursts, 2 * args.sets))
              for dt in ("fp32", "bf16")}
    loops = {f"N{nn}": three_loops(nn, args.warmup, args.unrolls) for nn in (int(x) for x in args.envs.split(","))}
    res = dict(what="first measurements of parameter publication on the device: the publish kernel alone beside its HBM floor, "
                    "and three loops on device Breakout (host blob, device publish, device publish overlapped) alternated "
                    "unroll by unroll; no bar on a speed-up",
               param_count=n, bytes_moved=8 * n, floor_us=floor_us, hbm_tbs=HBM_TBS, kernel=kernel, seq_len=T, num_actions=A,
               warmup_unrolls=args.warmup, timed_unrolls=args.unrolls, loops=loops, source_hash=build_info.source_hash())
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
