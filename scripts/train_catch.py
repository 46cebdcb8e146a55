#!/usr/bin/env python3
"""A first learning measurement: the Atari policy on the built-in Catch environment, everything on
one device (include/fi_env.h, fi_rollout.h, fi_train.h). N = B = 256 environments, T = 20, A = 3.

Each unroll: env.rollout(actor, T) -> learner.step_rollout(actor) -> actor.set_params(the learner's
blob). `--unrolls` unrolls per configuration (default 2,000); every `--window` unrolls (default 100)
the mean return of the episodes that finished in the window, from the differences of env.stats().
Two configurations, each with its own learner, actor and environment of the same seeds:

  adam      Adam at the repository's default rate, nothing else set
  rmsprop   RMSProp with monobeast's numbers: lr 4.8e-4, decay 0.99, eps 0.01, momentum 0, the rate
            annealed linearly to 0 over the run, rewards clipped to [-1, 1]

and, as the baseline, the return of the untrained policy measured the same way over one window with a
third learner's initial parameters and no learner step. An episode of Catch lasts 20 steps and ends
with +1 (caught) or -1 (missed). Nothing is tuned and there is no threshold: the curves are the
result. Prints one JSON line and writes it to profiles/train_catch.json.

    python scripts/train_catch.py [--out profiles/train_catch.json] [--unrolls 2000] [--window 100]
                                   [--publish host|device] [--overlap]
                                [--temperature TAU] [--epsilon EPS] [--epsilon-alpha ALPHA]

`--publish device` replaces the blob round trip by learner.publish() -> actor.set_params_dev(learner)
(include/fi_publish.h): the parameters stay on the device and neither side waits for the hand-over.
`--overlap` (with `--publish device`) also enqueues the next unroll's acting before this unroll's
step: env.rollout(actor, T - 1) -> learner.step_rollouts_async([actor]) -> learner.publish() ->
actor.set_params_dev(learner) -> env.rollout(actor, 1). The last step of an unroll writes record 0 of
the next one into the buffer the learner reads, so it goes behind the release; the T - 1 steps before
it run while the learner steps, one version behind, which `batch_versions` reports and V-trace
corrects. The host waits once per window (learner.wait()). The default is `host` without overlap:
the loop above, unchanged. The other modes write profiles/train_catch_device_publish.json.

`--temperature`, `--epsilon` and `--epsilon-alpha` make the training actors explore (include/fi_explore.h):
a sampling temperature, an epsilon for every environment, and with `--epsilon-alpha` Ape-X's ladder
across the N environments, eps_i = EPS ** (1 + ALPHA i / (N - 1)). The records' mu are then the behaviour
logits, so V-trace stays right; the scores are those of the exploring actors. The untrained baseline
stays the plain draw. The defaults (1, 0, no ladder) leave the loop and the output unchanged; anything
else writes profiles/train_catch_explore.json.

`--diagnostics K` enqueues the off-policy diagnostics (include/fi_diag.h) behind the step of every K-th
unroll and reads the newest one in front of the next report line: the clip rates, kl_mu_pi, ess, max_rho
and explained_variance go to stderr and into the window's entry of the JSON
(profiles/train_catch_diag.json unless --out names another file). The step is unchanged by it.

`--popart [BETA]` (include/fi_popart.h; BETA defaults to the paper's 3e-4) runs, next to the `rmsprop`
configuration as it stands, `rmsprop_popart`: the same RMSProp numbers and schedule WITHOUT the reward
clip and with PopArt value normalisation on the learner; `adam` is left out. Every window's entry of
that run carries the statistics mu, sigma; the output goes to profiles/train_catch_popart.json unless --out
names another file. Off by default: without the flag the loops enqueue what they enqueued before.

`--objective surrogate` (include/fi_surrogate.h; `--clip EPS`, default 0.2) runs, next to the `rmsprop`
configuration as it stands (the V-trace policy gradient), `rmsprop_surrogate`: the same numbers, schedule and
reward clip with the clipped surrogate objective on the learner; `--normalize-adv` adds
`rmsprop_surrogate_normalized`, the same with the advantages normalised over the batch; `adam` is left out.
Every window's entry of those runs carries the last step's clipped fraction and advantage moments; the output
goes to profiles/train_catch_surrogate.json unless --out names another file. The default, `--objective
vtrace`, leaves the loops as they were.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import build_info, diag, env, hip  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

N, T, A, GAMMA, SEED = 256, 20, 3, 0.99, 1
RMSPROP = dict(lr=4.8e-4, decay=0.99, eps=0.01, momentum=0.0, reward_clip=1.0)
POPART_BETA = None  # --popart [BETA]: the beta of the rmsprop_popart configuration
SURROGATE_CLIP = 0.2  # --clip EPS: the eps of the rmsprop_surrogate* configurations


def make_learner(config: str, unrolls: int) -> DeviceLearner:
    if config.startswith("rmsprop"):
        L = DeviceLearner("atari", seq_len=T, batch=N, num_actions=A, records="planes", optimizer="rmsprop",
                          lr=RMSPROP["lr"], seed=SEED)
        L.set_rmsprop(RMSPROP["decay"], RMSPROP["momentum"], RMSPROP["eps"])
        L.set_lr_schedule(0.0, unrolls)
        if config == "rmsprop_popart":  # the value head normalised in place of the clipped rewards
            L.enable_popart(beta=POPART_BETA)
        else:
            L.set_reward_clip(RMSPROP["reward_clip"])
        if "surrogate" in config:  # the second objective in V-trace's place; everything else as `rmsprop`
            L.set_objective("surrogate", clip=SURROGATE_CLIP, normalize_advantages=config.endswith("_normalized"))
        return L
    return DeviceLearner("atari", seq_len=T, batch=N, num_actions=A, records="planes", seed=SEED)


def window_of(e: env.CatchEnv, before: dict) -> tuple[dict, dict]:
    now = e.stats()
    n, s = now["episodes"] - before["episodes"], now["return_sum"] - before["return_sum"]
    return now, dict(episodes=n, mean_return=round(s / n, 4) if n else None)


def popart_window(L: DeviceLearner, config: str) -> dict:
    """The statistics at a window's end (waits for the learner's stream); nothing for a plain configuration."""
    if "surrogate" in config:
        s = L.objective_state()
        return dict(clipped_fraction=round(s["rows_clipped"] / max(1, s["rows"]), 4), adv_mean=round(s["adv_mean"], 6),
                    adv_std=round(s["adv_std"], 6))
    if config != "rmsprop_popart":
        return {}
    s = L.popart_state()
    return dict(popart_mu=round(s["mu"], 6), popart_sigma=round(s["sigma"], 6), popart_updates=s["updates"])


def hand_over(L: DeviceLearner, a: Actor, publish: str) -> None:
    if publish == "device":
        L.publish()
        a.set_params_dev(L)
    else:
        blob, version = L.get_blob()
        a.set_params(blob, version)


def explore(a: Actor, ex: dict | None) -> None:
    if ex:
        from freeimpala_amd.explore import epsilon_ladder
        eps = ex["epsilon"] if ex["epsilon_alpha"] is None else epsilon_ladder(N, ex["epsilon"], ex["epsilon_alpha"])
        a.set_exploration(ex["temperature"], eps)


def train_overlapped(config: str, unrolls: int, window: int, ex: dict | None = None, diag_every: int = 0) -> dict:
    """--publish device --overlap: unroll u + 1 is acted while unroll u is stepped; one host wait per window."""
    L = make_learner(config, unrolls)
    a = Actor("atari", N, num_actions=A, seed=SEED)
    hand_over(L, a, "device")
    explore(a, ex)
    a.begin_rollout(T)
    e = env.CatchEnv(N, GAMMA, seed=SEED)
    assert e.rollout(a, T + 1) == T + 1  # the first unroll, complete
    curve, seen, last, pending = [], e.stats(), {}, 0
    t0 = time.perf_counter()
    for u in range(1, unrolls + 1):
        assert e.rollout(a, T - 1) == T - 1
        L.step_rollouts_async([a])
        pending = diag.enqueue_every(L, u, diag_every) or pending  # --diagnostics K: no host wait
        hand_over(L, a, "device")
        assert e.rollout(a, 1) == 1
        if u % window == 0:
            last = L.wait()
            bv = L.batch_versions
            seen, w = window_of(e, seen)
            w.update(popart_window(L, config))
            pending = diag.report(L, config, pending, w)
            curve.append(dict(unroll=u, total_loss=round(last["total_loss"], 4), grad_norm=round(last["grad_norm"], 4),
                              batch_versions=[bv["min"], bv["max"], round(bv["mean"], 3)], **w))
    last = L.wait()
    wall = time.perf_counter() - t0
    state = L.train_state()
    a.sync()
    a.end_rollout()
    for h in (a, e, L):
        h.close()
    return dict(curve=curve, wall_s=round(wall, 3), env_steps=unrolls * N * T, env_steps_per_s=round(unrolls * N * T / wall, 1),
                learner_version=last.get("version"), train_state=state)


def train(config: str, unrolls: int, window: int, publish: str = "host", ex: dict | None = None,
          diag_every: int = 0) -> dict:
    L = make_learner(config, unrolls)
    a = Actor("atari", N, num_actions=A, seed=SEED)
    hand_over(L, a, publish)
    explore(a, ex)
    a.begin_rollout(T)
    e = env.CatchEnv(N, GAMMA, seed=SEED)
    assert e.rollout(a, 1) == 1  # step 0 of the first unroll
    curve, seen, last, pending = [], e.stats(), {}, 0
    t0 = time.perf_counter()
    for u in range(1, unrolls + 1):
        assert e.rollout(a, T) == T
        last = L.step_rollout(a)
        pending = diag.enqueue_every(L, u, diag_every) or pending  # --diagnostics K: no host wait
        hand_over(L, a, publish)
        if u % window == 0:
            seen, w = window_of(e, seen)
            w.update(popart_window(L, config))
            pending = diag.report(L, config, pending, w)
            curve.append(dict(unroll=u, total_loss=round(last["total_loss"], 4), grad_norm=round(last["grad_norm"], 4), **w))
    wall = time.perf_counter() - t0
    state = L.train_state()
    a.sync()
    a.end_rollout()
    for h in (a, e, L):
        h.close()
    return dict(curve=curve, wall_s=round(wall, 3), env_steps=unrolls * N * T, env_steps_per_s=round(unrolls * N * T / wall, 1),
                learner_version=last.get("version"), train_state=state)


def untrained(window: int) -> dict:
    """One window of the loop with a never-stepped learner's parameters: no record, no learner step."""
    L = make_learner("adam", 1)
    a = Actor("atari", N, num_actions=A, seed=SEED)
    blob, version = L.get_blob()
    a.set_params(blob, version)
    e = env.CatchEnv(N, GAMMA, seed=SEED)
    assert e.rollout(a, 1) == 1
    seen = e.stats()
    for _ in range(window):
        assert e.rollout(a, T) == T
    a.sync()
    _, w = window_of(e, seen)
    for h in (a, e, L):
        h.close()
    return w


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--unrolls", type=int, default=2000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--publish", choices=("host", "device"), default="host")
    ap.add_argument("--overlap", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--epsilon-alpha", type=float, default=None)
    ap.add_argument("--diagnostics", type=int, default=0, metavar="K")
    ap.add_argument("--popart", type=float, nargs="?", const=3e-4, default=None, metavar="BETA")
    ap.add_argument("--objective", choices=("vtrace", "surrogate"), default="vtrace")
    ap.add_argument("--clip", type=float, default=0.2, metavar="EPS")
    ap.add_argument("--normalize-adv", action="store_true")
    # include/fi_mlp.h: the MLP policy's numeric mode. Catch is played from frames by the Atari policy, which has
    # one mode (bf16 images already), so there is no MLP learner here for the option to reach
    ap.add_argument("--mlp-precision", choices=("fp32", "bf16"), default="fp32")
    args = ap.parse_args()
    if args.mlp_precision != "fp32":
        print("train_catch: --mlp-precision applies to an MLP policy; this script trains the Atari policy only (ignored)")
    if args.diagnostics < 0:
        raise SystemExit("train_catch: --diagnostics K enqueues every K-th unroll, K >= 1 (0: off)")
    if args.overlap and args.publish != "device":
        raise SystemExit("train_catch: --overlap needs --publish device (the host blob waits for the learner)")
    default_mode = args.publish == "host" and not args.overlap
    ex = None
    if args.temperature != 1.0 or args.epsilon != 0.0:
        ex = dict(temperature=args.temperature, epsilon=args.epsilon, epsilon_alpha=args.epsilon_alpha)
    elif args.epsilon_alpha is not None:
        raise SystemExit("train_catch: --epsilon-alpha is the ladder's exponent and needs --epsilon, its base")
    global POPART_BETA
    if args.popart is not None and not 0.0 <= args.popart <= 1.0:
        raise SystemExit("train_catch: --popart BETA is the statistics' step size, in [0, 1]")
    POPART_BETA = args.popart
    configs = ("adam", "rmsprop") if args.popart is None else ("rmsprop", "rmsprop_popart")
    global SURROGATE_CLIP
    if args.objective == "surrogate":
        if args.popart is not None:
            raise SystemExit("train_catch: --objective surrogate and --popart are separate comparisons; run them apart")
        if not 0.0 < args.clip < float("inf"):
            raise SystemExit("train_catch: --clip EPS is the surrogate's clip range, finite and > 0")
        SURROGATE_CLIP = args.clip
        configs = ("rmsprop", "rmsprop_surrogate") + (("rmsprop_surrogate_normalized",) if args.normalize_adv else ())
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "train_catch_surrogate.json")
    elif args.normalize_adv or args.clip != 0.2:
        raise SystemExit("train_catch: --clip and --normalize-adv belong to --objective surrogate")
    if args.out is None and args.popart is not None:
        args.out = os.path.join(ROOT, "profiles", "train_catch_popart.json")
    if args.out is None and args.diagnostics:
        args.out = os.path.join(ROOT, "profiles", "train_catch_diag.json")
    if args.out is None and ex:
        args.out = os.path.join(ROOT, "profiles", "train_catch_explore.json")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "train_catch.json" if default_mode else "train_catch_device_publish.json")
    if hip.device_count() < 1:
        raise SystemExit("train_catch: no HIP device; nothing is measured without one")
    t0 = time.perf_counter()
    base = untrained(args.window)
    if args.overlap:
        runs = {c: train_overlapped(c, args.unrolls, args.window, ex, args.diagnostics) for c in configs}
    else:
        runs = {c: train(c, args.unrolls, args.window, args.publish, ex, args.diagnostics) for c in configs}
    res = dict(what="first learning measurement: the Atari policy on device-resident Catch, mean return of the episodes "
                    "finished in every window of unrolls; two documented settings, nothing tuned, no threshold",
               num_envs=N, batch=N, seq_len=T, num_actions=A, gamma=GAMMA, seed=SEED, unrolls=args.unrolls,
               window_unrolls=args.window, episode_steps=env.EPISODE_STEPS, return_range=[-1, 1],
               configs=dict(adam="Adam, fi_learner_config_init's rate and moments, global-norm clip 40",
                            rmsprop=dict(RMSPROP, lr_end=0.0, lr_steps=args.unrolls, max_grad_norm="default (40)")),
               untrained_policy=base, runs=runs, wall_s=round(time.perf_counter() - t0, 3),
               source_hash=build_info.source_hash())
    if not default_mode:
        res.update(publish=args.publish, overlap=args.overlap)
    if args.diagnostics:
        res.update(diagnostics_every=args.diagnostics)
    if args.popart is not None:
        res["configs"].pop("adam")
        res["configs"]["rmsprop_popart"] = dict({k: v for k, v in RMSPROP.items() if k != "reward_clip"}, lr_end=0.0,
                                                lr_steps=args.unrolls, max_grad_norm="default (40)", reward_clip="off",
                                                popart=dict(beta=args.popart, sigma_min=1e-4, sigma_max=1e6))
    if args.objective == "surrogate":
        res["configs"].pop("adam")
        for c in configs[1:]:
            res["configs"][c] = dict(RMSPROP, lr_end=0.0, lr_steps=args.unrolls, max_grad_norm="default (40)",
                                     objective=dict(name="surrogate", clip=args.clip, adv_eps=1e-8,
                                                    normalize_advantages=c.endswith("_normalized")))
    if ex:
        res.update(exploration=dict(ex, note="the training actors explore and record their behaviour logits as mu; "
                                             "the scores are the exploring actors' own; the untrained baseline is the plain draw"))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
