"""PCIe-inclusive learner rate: the step fed from host SharedBuffer entries (what
Learner::trainModel hands over after SharedBuffer::readBatch, data_structures.h:267-300)
against the step on a batch already resident in HBM (bench.py's `value`).

usage: python scripts/host_batch_bench.py [--arch mlp|atari] [--records stacked|planes] [--T 100]
                                          [--B 4096] [--steps N]
--arch mlp: entries follow the 1 KiB record schema, T+1 records each.
--arch atari: entries of T+1 Atari records (28 elements = 28,672 B per step: the 84x84x4 frame,
then the header); at T=100, B=4096 a batch is 12.1 GB and the learner stages it through two
pinned and two device buffers of that size. When they cannot be allocated the run halves B until
they can and reports the B it used.
--arch atari --records planes: entries of T+1 single-plane records (7 elements = 7,168 B per step:
the newest 84x84 plane, then the header) and the 21-element history block; at T=100, B=4096 a
batch is 3.05 GB. The planes are channel 3 of the synthetic frames, the history channels 0..2 of
frame 0, and episode_start follows every discount of 0.
Prints one JSON line:
  resident    env-steps/s of fi_learner_step_resident
  host_serial        fi_learner_step: pinned staging copy + one H2D + ingest + step, returns
                     when done
  host_async         fi_learner_step_async x steps, then fi_learner_wait: the staging copy and
                     H2D of batch k+1 (copy stream, second device slot) overlap the device
                     step of batch k
  host_staged_h2d    fi_learner_acquire_staging + fi_learner_step_staged_async on buffers
                     the caller filled beforehand (its readBatchInto copy not timed): H2D +
                     step alone, the PCIe bound
  ingest             (from set_profiling) the "ingest" phase of a host-fed step -- it starts
                     with the wait for the batch's H2D -- and the ingest kernels alone; for
                     atari also the copy floor 2 * (T+1) * B * 28,224 B / 6.3 TB/s and the gap
                     (planes: the floor reads (T+1+3) * B * 7,056 B and writes (T+1) * B * 28,224 B)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_ACHIEVABLE = 6.3e12  # B/s, the achievable rate of DESIGN.md's roofline tables


def log(msg):
    print(f"[host_batch_bench] {msg}", file=sys.stderr, flush=True)


def kernel_times(L):
    from freeimpala_amd._abi import lib
    buf = C.create_string_buffer(8192)
    ms = (C.c_float * 128)()
    cnt = (C.c_int * 128)()
    n = lib().fi_learner_kernel_times(L._h, buf, 8192, ms, cnt, 128)
    names = buf.value.decode().split("\n")[:n]
    return {names[i]: ms[i] for i in range(n)}


def make_learner(arch, T, B, A, records="stacked"):
    """The learner with its host staging allocated, at the largest power-of-two B <= the asked
    one whose staging buffers can be had."""
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import DeviceLearner
    while True:
        L = DeviceLearner(arch, seq_len=T, batch=B, num_actions=A, optimizer="adam", records=records)
        try:
            L.acquire_staging()  # allocates the two pinned and the two device buffers
            return L, B
        except FiError as e:
            L.close()
            if "rc=-3" not in str(e) or B == 1:
                raise
            log(f"B={B}: {e}")
            B = 1 << ((B - 1).bit_length() - 1)  # the next power of two below B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=("mlp", "atari"), default="mlp")
    ap.add_argument("--records", choices=("stacked", "planes"), default="stacked", help="atari host record format")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=None, help="timed steps per row (default 8; atari 4)")
    args = ap.parse_args()
    from freeimpala_amd.learner import HostBatch, pack_atari_plane_records, pack_atari_records, pack_records
    atari = args.arch == "atari"
    planes = args.records == "planes"
    if planes and not atari:
        ap.error("--records planes needs --arch atari")
    T, A = args.T, 18
    steps = args.steps or (4 if atari else 8)
    L, B = make_learner(args.arch, T, args.B, A, args.records)
    log(f"{args.arch} {args.records if atari else ''} T={T} B={B}: staging 2 x {B * L.entry_bytes / 1e9:.2f} GB pinned + device")
    L.synth(seed=42)
    mu = L.tensor("mu", shape=(T, B, A))
    act = L.tensor("actions", np.int32, (T, B))
    rew = L.tensor("rewards", shape=(T, B))
    disc = L.tensor("discounts", shape=(T, B))
    t0 = time.perf_counter()
    if planes:
        obs = L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4))
        start = np.zeros((T + 1, B), bool)
        start[1:] = disc == 0
        entries = HostBatch(pack_atari_plane_records(
            np.ascontiguousarray(obs[..., 3]), np.ascontiguousarray(obs[0, :, :, :, :3].transpose(3, 0, 1, 2)),
            start, mu, act, rew, disc))
    elif atari:
        obs = L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4))
        entries = HostBatch(pack_atari_records(obs, mu, act, rew, disc))
    else:
        obs = L.tensor("obs", shape=(T + 1, B, 128))
        entries = HostBatch(pack_records(obs, mu, act, rew, disc, entry_size=T + 1))
    del obs
    pack_s = time.perf_counter() - t0
    eb = entries.entry_bytes
    log(f"packed {B} entries of {eb} bytes in {pack_s:.1f} s")

    def timed(fn, n):
        fn()
        L.sync()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        L.sync()
        return (time.perf_counter() - t) / n

    res = timed(lambda: L.step_resident(stats=False), steps)
    log(f"resident {1e3 * res:.2f} ms")
    # serial: fi_learner_step returns when the step is done (copy, H2D, step back to back)
    ser = timed(lambda: L.step(entries, stats=False), steps)
    log(f"serial {1e3 * ser:.2f} ms")
    # pipelined: fi_learner_step_async; copy + H2D of batch k+1 beside the step of batch k
    L.step_async(entries)
    L.wait()
    t = time.perf_counter()
    for _ in range(steps):
        c = time.perf_counter()
        L.step_async(entries)
        if os.environ.get("FI_STAGE_TIMING"):
            print(f"[async call] {1e3 * (time.perf_counter() - c):.3f} ms", file=sys.stderr, flush=True)
    L.wait()
    asy = (time.perf_counter() - t) / steps
    log(f"async {1e3 * asy:.2f} ms")
    # staged: the caller's readBatchInto fills the acquired pinned buffer (done once here:
    # the loop then times H2D + step alone, the PCIe bound of the staged path)
    stride = L.entry_bytes
    for _ in range(2):
        dst = L.acquire_staging()
        for b, e in enumerate(entries.bufs):
            dst[b] = e[:stride]
        L.step_staged_async()
    L.wait()
    t = time.perf_counter()
    for _ in range(steps):
        L.acquire_staging()
        L.step_staged_async()
    L.wait()
    stg = (time.perf_counter() - t) / steps
    log(f"staged {1e3 * stg:.2f} ms")
    # the ingest phase and kernels of a host-fed step
    L.set_profiling(True)
    for _ in range(min(steps, 3)):
        L.step(entries, stats=False)
    ingest = {"phase_ms": round(L.phase_times()["ingest"], 3), "kernels_ms": round(kernel_times(L).get("ingest", 0.0), 3)}
    L.set_profiling(False)
    if atari:
        moved = ((T + 4) * 7056 + (T + 1) * 28224) * B if planes else 2 * (T + 1) * B * 28224
        floor_ms = 1e3 * moved / HBM_ACHIEVABLE
        ingest["copy_floor_ms"] = round(floor_ms, 3)
        ingest["kernels_over_floor"] = round(ingest["kernels_ms"] / floor_ms, 2)
    mb = B * eb / 1e6
    out = {
        "arch": args.arch, **({"records": args.records} if atari else {}), "T": T, "B": B, "B_requested": args.B, "entry_bytes": eb, "batch_mb": round(mb, 1),
        "resident": {"ms_per_step": round(1e3 * res, 3), "env_steps_per_s": round(T * B / res, 1)},
        "host_serial": {"ms_per_step": round(1e3 * ser, 3), "env_steps_per_s": round(T * B / ser, 1)},
        "host_async": {"ms_per_step": round(1e3 * asy, 3), "env_steps_per_s": round(T * B / asy, 1),
                       "batch_gb_s": round(mb / 1e3 / asy, 1)},
        "host_staged_h2d": {"ms_per_step": round(1e3 * stg, 3), "env_steps_per_s": round(T * B / stg, 1),
                            "batch_gb_s": round(mb / 1e3 / stg, 1)},
        "ingest": ingest,
        "pack_records_s": round(pack_s, 2),
    }
    print(json.dumps(out), flush=True)
    L.close()


if __name__ == "__main__":
    main()
