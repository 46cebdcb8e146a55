#!/usr/bin/env python3
"""First measurements of the device Breakout environment (include/fi_breakout.h) next to Catch
(include/fi_env.h), both in one session.

Kernels: the update and the render of either environment alone, on buffers of their own, at N in
{1024, 65536}. Per kernel and N: `--reps` windows of `--launches` launches each between two HIP
events on the null stream, the four kernels (and Breakout's update once more without its totals,
which leaves out its atomic adds) alternated window by window; reported in device ms per launch as
median, min and max over the windows, so the session's spread is visible beside every difference. The actions vary, and every window of the update starts from the same uploaded states
(Breakout: `--reps` x `--launches` steps of a 1,000-step episode would otherwise end episodes at
different times in different windows). The render is a pure store stream: its floor is
N * 7056 B / 6.3 TB/s.

Loop: device_env_bench.py's rollout loop -- one recording Atari actor, one learner, N = B
environments, A = 18, T = 20, fi_env_rollout(T) then DeviceLearner.step_rollout -- with a CatchEnv and
with a BreakoutEnv, alternated unroll by unroll, at N in {256, 1024}: wall ms per unroll (median, min,
max) and env-steps/s from the median.

No number here has a threshold. Prints one JSON line and writes it to profiles/breakout_env.json.

    python scripts/breakout_bench.py [--out profiles/breakout_env.json]
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

from freeimpala_amd import breakout, build_info, env, hip  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
GAMMA, MAX_STEPS = 0.99, 1000


def spread(v) -> dict:
    return dict(median=round(float(np.median(v)), 5), min=round(min(v), 5), max=round(max(v), 5))


def kernel_ms(n: int, launches: int, reps: int) -> dict:
    """Device ms per launch of the kernels at n environments, alternated window by window."""
    catch0 = env.catch_reference(n, GAMMA, 2)
    s = catch0.state()
    catch_words = np.stack([s["r"], s["c"], s["p"], s["k"].astype(np.int32)], 1).astype(np.uint32)
    rs = np.random.RandomState(n)
    # Breakout states in mid-episode: the ball anywhere above the paddle's row, random bricks
    b = dict(r=rs.randint(0, 20, n), c=rs.randint(0, 21, n), p=rs.randint(1, 20, n), k=np.zeros(n, np.uint32),
             dr=rs.choice([-1, 1], n), dc=rs.choice([-1, 1], n), t=rs.randint(0, MAX_STEPS // 2, n), score=np.zeros(n),
             bricks=(rs.randint(0, 2 ** 31, n).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 2 ** 32, n, dtype=np.uint64)
             | np.uint64(1))
    brk_words = breakout.pack_state(b)
    d_act = hip.DeviceBuffer.from_array(rs.randint(0, 3, n).astype(np.int32))
    bufs = dict(cs=hip.DeviceBuffer(n * 16), bs=hip.DeviceBuffer(n * 32), cp=hip.DeviceBuffer(n * 7056),
                bp=hip.DeviceBuffer(n * 7056), start=hip.DeviceBuffer(n), rew=hip.DeviceBuffer(n * 4),
                disc=hip.DeviceBuffer(n * 4), tot=hip.DeviceBuffer(16))
    bufs["tot"].zero()
    p = {k: v.ptr for k, v in bufs.items()}
    calls = {
        "catch_update": lambda: env.env_update(p["cs"], d_act.ptr, n, GAMMA, 2, p["start"], p["rew"], p["disc"], p["tot"]),
        "breakout_update": lambda: breakout.breakout_update(p["bs"], d_act.ptr, n, GAMMA, 2, MAX_STEPS, p["start"], p["rew"],
                                                            p["disc"], p["tot"]),
        # the same launch without the totals: what the per-wave atomic adds on two addresses cost
        "breakout_update_no_totals": lambda: breakout.breakout_update(p["bs"], d_act.ptr, n, GAMMA, 2, MAX_STEPS, p["start"],
                                                                      p["rew"], p["disc"], None),
        "catch_render": lambda: env.env_render(p["cs"], p["cp"], n),
        "breakout_render": lambda: breakout.breakout_render(p["bs"], p["bp"], n),
    }

    def reset_states():
        bufs["cs"].upload(catch_words)
        bufs["bs"].upload(brk_words)

    reset_states()
    for call in calls.values():  # warm-up: code objects, clocks
        for _ in range(20):
            call()
    hip.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        reset_states()
        for name, call in calls.items():
            e0, e1 = hip.Event(), hip.Event()
            e0.record()
            for _ in range(launches):
                call()
            e1.record()
            ms[name].append(e0.elapsed_ms(e1) / launches)
    for x in list(bufs.values()) + [d_act]:
        x.free()
    floor_ms = n * 7056 / HBM_BYTES_PER_S * 1e3
    out = dict(num_envs=n, launches_per_window=launches, windows=reps, ms_per_launch={k: spread(v) for k, v in ms.items()},
               render_store_floor_ms=round(floor_ms, 6))
    for k in ("catch_render", "breakout_render"):
        out[k + "_share_of_floor"] = round(floor_ms / float(np.median(ms[k])), 4)
    out["breakout_over_catch_render_median"] = round(float(np.median(ms["breakout_render"]) / np.median(ms["catch_render"])), 4)
    return out


class Loop:
    """device_env_bench.py's rollout loop with either environment."""

    def __init__(self, kind: str, n: int, T: int, A: int, params: np.ndarray):
        self.T = T
        self.L = DeviceLearner("atari", seq_len=T, batch=n, num_actions=A, records="planes", lr=1e-4, seed=1)
        self.L.set_params(params)
        self.a = Actor("atari", n, num_actions=A, seed=1)
        self.a.set_params(params)
        self.a.begin_rollout(T)
        self.e = env.CatchEnv(n, GAMMA, seed=1) if kind == "catch" else breakout.BreakoutEnv(n, GAMMA, 1, MAX_STEPS)
        assert self.e.rollout(self.a, 1) == 1  # step 0 of the first unroll

    def unroll(self) -> float:
        t0 = time.perf_counter()
        assert self.e.rollout(self.a, self.T) == self.T
        self.L.step_rollout(self.a)
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.a.sync()
        self.a.end_rollout()
        for h in (self.a, self.e, self.L):
            h.close()


def loop_ms(n: int, T: int, A: int, params: np.ndarray, unrolls: int, warmup: int) -> dict:
    loops = {k: Loop(k, n, T, A, params) for k in ("catch", "breakout")}
    for _ in range(warmup):
        for lp in loops.values():
            lp.unroll()
    wall = {k: [] for k in loops}
    for _ in range(unrolls):  # alternating
        for k, lp in loops.items():
            wall[k].append(lp.unroll())
    stats = {k: lp.e.stats() for k, lp in loops.items()}
    for lp in loops.values():
        lp.close()
    return dict(num_envs=n, seq_len=T, wall_ms_per_unroll={k: spread(v) for k, v in wall.items()},
                env_steps_per_s={k: round(n * T / float(np.median(v)) * 1e3, 1) for k, v in wall.items()}, episodes=stats)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "breakout_env.json"))
    ap.add_argument("--kernel-envs", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-envs", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--unrolls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--num-actions", type=int, default=18)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit("breakout_bench: no HIP device; nothing is measured without one")
    kernels = [kernel_ms(n, args.launches, args.reps) for n in args.kernel_envs]
    L = DeviceLearner("atari", seq_len=1, batch=1, num_actions=args.num_actions, seed=1)
    params = L.get_params()
    L.close()
    loops = [loop_ms(n, args.seq_len, args.num_actions, params, args.unrolls, args.warmup) for n in args.loop_envs]
    res = dict(what="first measurements: the update and render kernels of the Catch and Breakout device environments "
                    "alternated in one session, and the recording rollout loop with either; no thresholds",
               hbm_bytes_per_s=HBM_BYTES_PER_S, max_steps=MAX_STEPS, num_actions=args.num_actions,
               source_hash=build_info.source_hash(), kernels=kernels, loops=loops)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
