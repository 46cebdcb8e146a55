#!/usr/bin/env python3
"""A learning measurement on an environment that needs the frame stack: the Atari policy on the
built-in Breakout environment, everything on one device (include/fi_breakout.h, fi_env.h,
fi_rollout.h, fi_train.h). N = B = 256 environments, T = 20, A = 3, max_steps = 1000.

Each unroll: env.rollout(actor, T) -> learner.step_rollout(actor) -> actor.set_params(the learner's
blob). `--unrolls` unrolls per configuration (default 2,000); every `--window` unrolls (default 100)
the mean score of the episodes that finished in the window, from the differences of env.stats().
Two configurations, each with its own learner, actor and environment of the same seeds:

  adam      Adam at the repository's default rate, nothing else set
  rmsprop   RMSProp with monobeast's numbers: lr 4.8e-4, decay 0.99, eps 0.01, momentum 0, the rate
            annealed linearly to 0 over the run, rewards clipped to [-1, 1]

and, as the baseline, the score of the untrained policy measured the same way over one window with a
third learner's initial parameters and no learner step. An episode ends when the ball passes the
paddle or after max_steps steps; its return is the number of bricks it cleared (a reward of 1 each).
Nothing is tuned and there is no threshold: the curves are the result. Prints one JSON line and
writes it to profiles/train_breakout.json.

    python scripts/train_breakout.py [--out profiles/train_breakout.json] [--unrolls 2000] [--window 100]
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
the loop above, unchanged. The other modes write profiles/train_breakout_device_publish.json.

`--temperature`, `--epsilon` and `--epsilon-alpha` make the training actors explore (include/fi_explore.h):
a sampling temperature, an epsilon for every environment, and with `--epsilon-alpha` Ape-X's ladder
across the N environments, eps_i = EPS ** (1 + ALPHA i / (N - 1)). The records' mu are then the behaviour
logits, so V-trace stays right; the scores are those of the exploring actors. The untrained baseline
stays the plain draw. The defaults (1, 0, no ladder) leave the loop and the output unchanged; anything
else writes profiles/train_breakout_explore.json.

`--diagnostics K` enqueues the off-policy diagnostics (include/fi_diag.h) behind the step of every K-th
unroll and reads the newest one in front of the next report line: the clip rates, kl_mu_pi, ess, max_rho
and explained_variance go to stderr and into the window's entry of the JSON
(profiles/train_breakout_diag.json unless --out names another file). The step is unchanged by it.

`--popart [BETA]` (include/fi_popart.h; BETA defaults to the paper's 3e-4) runs, next to the `rmsprop`
configuration as it stands, `rmsprop_popart`: the same RMSProp numbers and schedule WITHOUT the reward
clip and with PopArt value normalisation on the learner; `adam` is left out. Every window's entry of
that run carries the statistics mu, sigma; the output goes to profiles/train_breakout_popart.json unless --out
names another file. Off by default: without the flag the loops enqueue what they enqueued before.

`--objective surrogate` (include/fi_surrogate.h; `--clip EPS`, default 0.2) runs, next to the `rmsprop`
configuration as it stands (the V-trace policy gradient), `rmsprop_surrogate`: the same numbers, schedule and
reward clip with the clipped surrogate objective on the learner; `--normalize-adv` adds
`rmsprop_surrogate_normalized`, the same with the advantages normalised over the batch; `adam` is left out.
Every window's entry of those runs carries the last step's clipped fraction and advantage moments; the output
goes to profiles/train_breakout_surrogate.json unless --out names another file. The default, `--objective
vtrace`, leaves the loops as they were.

`--n-fresh K` (K divides B = 256, K < B) is the replaying loop: every unroll goes through an `EntryRing` of 8 B
entries (`ring.push_rollout(actor)`), and the learner takes B / K steps per unroll, each
`learner.step_ring(ring, n_fresh=K)`: K columns are that unroll's, B - K are drawn from the entries read before that
are still resident, up to eight unrolls old. (The first unroll is one step with all B columns fresh: nothing can be
replayed before something was read.) The learning-rate schedule runs over the steps taken. Next to `rmsprop` it runs
`rmsprop_surrogate` with `--objective surrogate`, and with `--target-period P` (`--target-tau TAU`, default 1; both
need `--objective surrogate`) also `rmsprop_surrogate_target`: the same with the learner's target network on
(include/fi_target.h), whose windows carry mean_log_r and the target's updates. The output goes to
profiles/train_breakout_target.json unless --out names another file. Without these flags the script runs the loops
it ran before.

`--kl-coeff C` (include/fi_kl.h; `--kl-target D`, default 0.01; `--kl-reference behaviour|target`, default behaviour;
`--kl-fixed` keeps C where it is) runs, next to the configurations the other flags select, the last of them once more
with the KL penalty on the learner, as `<that configuration>_kl`: C KL(q || pi) in the loss, q the records' behaviour
policy or (with `--target-period`) the target network's, and C adapting to D on the device. Every window's entry of
that run carries the coefficient, the last step's mean KL and the counts of adaptations, and the same go to stderr
with the window's score. The output goes to profiles/train_breakout_kl.json unless --out names another file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from freeimpala_amd import breakout, build_info, diag, hip  # noqa: E402
from freeimpala_amd.actor import Actor  # noqa: E402
from freeimpala_amd.learner import DeviceLearner  # noqa: E402

N, T, A, GAMMA, SEED, MAX_STEPS = 256, 20, 3, 0.99, 1, 1000
RMSPROP = dict(lr=4.8e-4, decay=0.99, eps=0.01, momentum=0.0, reward_clip=1.0)
POPART_BETA = None  # --popart [BETA]: the beta of the rmsprop_popart configuration
SURROGATE_CLIP = 0.2  # --clip EPS: the eps of the rmsprop_surrogate* configurations
KL = None  # --kl-coeff C, --kl-target D, --kl-reference R, --kl-fixed: enable_kl_penalty's arguments of the *_kl configuration
TARGET = None  # --target-period P, --target-tau TAU: (P, TAU) of the rmsprop_surrogate_target configuration
RING_UNROLLS = 8  # --n-fresh: the ring holds this many unrolls


def make_learner(config: str, unrolls: int) -> DeviceLearner:
    kl_on, config = config.endswith("_kl"), config.removesuffix("_kl")
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
        if config.endswith("_target"):
            L.enable_target(*TARGET)
        if kl_on:  # behind enable_target: the reference "target" needs the target network
            L.enable_kl_penalty(**KL)
        return L
    return DeviceLearner("atari", seq_len=T, batch=N, num_actions=A, records="planes", seed=SEED)


def window_of(e: breakout.BreakoutEnv, before: dict) -> tuple[dict, dict]:
    now = e.stats()
    n, s = now["episodes"] - before["episodes"], now["return_sum"] - before["return_sum"]
    return now, dict(episodes=n, mean_return=round(s / n, 4) if n else None)


def popart_window(L: DeviceLearner, config: str, mean_return=None) -> dict:
    """The statistics at a window's end (waits for the learner's stream); nothing for a plain configuration."""
    if config.endswith("_kl"):
        w = popart_window(L, config.removesuffix("_kl"))
        k = L.kl_state()
        w.update(kl_coeff=k["coeff"], mean_kl=round(k["mean_kl"], 6), kl_raised=k["raised"], kl_lowered=k["lowered"])
        print(f"[{config}] mean_return {mean_return} kl_coeff {k['coeff']:g} mean_kl {k['mean_kl']:.6f} "
              f"raised {k['raised']} lowered {k['lowered']}", file=sys.stderr, flush=True)
        return w
    if "surrogate" in config:
        s = L.objective_state()
        w = dict(clipped_fraction=round(s["rows_clipped"] / max(1, s["rows"]), 4), adv_mean=round(s["adv_mean"], 6),
                 adv_std=round(s["adv_std"], 6))
        if config.endswith("_target"):
            t = L.target_state()
            w.update(mean_log_r=round(t["mean_log_r"], 6), mean_sq_log_r=round(t["mean_sq_log_r"], 6),
                     target_updates=t["updates"])
        return w
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
    e = breakout.BreakoutEnv(N, GAMMA, seed=SEED, max_steps=MAX_STEPS)
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
            w.update(popart_window(L, config, w["mean_return"]))
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
    e = breakout.BreakoutEnv(N, GAMMA, seed=SEED, max_steps=MAX_STEPS)
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
            w.update(popart_window(L, config, w["mean_return"]))
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


def train_replay(config: str, unrolls: int, window: int, n_fresh: int, publish: str = "host", ex: dict | None = None) -> dict:
    """--n-fresh K: every unroll through an entry ring, N / K steps per unroll with K fresh columns each."""
    from freeimpala_amd.ring import EntryRing
    per_unroll = N // n_fresh
    L = make_learner(config, 1 + (unrolls - 1) * per_unroll)
    a = Actor("atari", N, num_actions=A, seed=SEED)
    hand_over(L, a, publish)
    explore(a, ex)
    a.begin_rollout(T)
    ring = EntryRing(L.entry_bytes, RING_UNROLLS * N, seed=SEED)
    e = breakout.BreakoutEnv(N, GAMMA, seed=SEED, max_steps=MAX_STEPS)
    assert e.rollout(a, 1) == 1  # step 0 of the first unroll
    curve, seen, last = [], e.stats(), {}
    t0 = time.perf_counter()
    for u in range(1, unrolls + 1):
        assert e.rollout(a, T) == T
        ring.push_rollout(a)
        if u == 1:
            last = L.step_ring(ring)  # all N fresh: there is nothing to replay yet
        else:
            for _ in range(per_unroll):
                last = L.step_ring(ring, n_fresh=n_fresh)
        hand_over(L, a, publish)
        if u % window == 0:
            seen, w = window_of(e, seen)
            w.update(popart_window(L, config, w["mean_return"]))
            curve.append(dict(unroll=u, total_loss=round(last["total_loss"], 4), grad_norm=round(last["grad_norm"], 4), **w))
    wall = time.perf_counter() - t0
    state = L.train_state()
    a.sync()
    a.end_rollout()
    for h in (a, e, ring, L):
        h.close()
    return dict(curve=curve, wall_s=round(wall, 3), env_steps=unrolls * N * T, env_steps_per_s=round(unrolls * N * T / wall, 1),
                learner_steps=1 + (unrolls - 1) * per_unroll, learner_version=last.get("version"), train_state=state)


def untrained(window: int) -> dict:
    """One window of the loop with a never-stepped learner's parameters: no record, no learner step."""
    L = make_learner("adam", 1)
    a = Actor("atari", N, num_actions=A, seed=SEED)
    blob, version = L.get_blob()
    a.set_params(blob, version)
    e = breakout.BreakoutEnv(N, GAMMA, seed=SEED, max_steps=MAX_STEPS)
    assert e.rollout(a, 1) == 1
    seen = e.stats()
    for _ in range(window):
        assert e.rollout(a, T) == T
    a.sync()
    _, w = window_of(e, seen)
    for h in (a, e, L):
        h.close()
    return w


def default_out(args, explores: bool, default_mode: bool) -> str:
    """The file under profiles/ a run without --out writes: every comparison keeps its own record. The replaying loop
    and the target network come first, so that `--objective surrogate` with either leaves the surrogate's file alone;
    the KL penalty, the newest, in front of both. (getattr: a caller's Namespace may be older than the option.)"""
    if getattr(args, "kl_coeff", None) is not None:
        return "train_breakout_kl.json"
    if args.n_fresh is not None or args.target_period is not None:
        return "train_breakout_target.json"
    if args.objective == "surrogate":
        return "train_breakout_surrogate.json"
    if args.popart is not None:
        return "train_breakout_popart.json"
    if args.diagnostics:
        return "train_breakout_diag.json"
    if explores:
        return "train_breakout_explore.json"
    return "train_breakout.json" if default_mode else "train_breakout_device_publish.json"


def parser() -> argparse.ArgumentParser:
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
    ap.add_argument("--n-fresh", type=int, default=None, metavar="K")
    ap.add_argument("--target-period", type=int, default=None, metavar="P")
    ap.add_argument("--target-tau", type=float, default=1.0, metavar="TAU")
    ap.add_argument("--kl-coeff", type=float, default=None, metavar="C")
    ap.add_argument("--kl-target", type=float, default=0.01, metavar="D")
    ap.add_argument("--kl-reference", choices=("behaviour", "target"), default="behaviour")
    ap.add_argument("--kl-fixed", action="store_true")
    return ap


def main() -> None:
    args = parser().parse_args()
    if args.diagnostics < 0:
        raise SystemExit("train_breakout: --diagnostics K enqueues every K-th unroll, K >= 1 (0: off)")
    if args.overlap and args.publish != "device":
        raise SystemExit("train_breakout: --overlap needs --publish device (the host blob waits for the learner)")
    default_mode = args.publish == "host" and not args.overlap
    ex = None
    if args.temperature != 1.0 or args.epsilon != 0.0:
        ex = dict(temperature=args.temperature, epsilon=args.epsilon, epsilon_alpha=args.epsilon_alpha)
    elif args.epsilon_alpha is not None:
        raise SystemExit("train_breakout: --epsilon-alpha is the ladder's exponent and needs --epsilon, its base")
    global POPART_BETA
    if args.popart is not None and not 0.0 <= args.popart <= 1.0:
        raise SystemExit("train_breakout: --popart BETA is the statistics' step size, in [0, 1]")
    POPART_BETA = args.popart
    configs = ("adam", "rmsprop") if args.popart is None else ("rmsprop", "rmsprop_popart")
    global SURROGATE_CLIP
    if args.objective == "surrogate":
        if args.popart is not None:
            raise SystemExit("train_breakout: --objective surrogate and --popart are separate comparisons; run them apart")
        if not 0.0 < args.clip < float("inf"):
            raise SystemExit("train_breakout: --clip EPS is the surrogate's clip range, finite and > 0")
        SURROGATE_CLIP = args.clip
        configs = ("rmsprop", "rmsprop_surrogate") + (("rmsprop_surrogate_normalized",) if args.normalize_adv else ())
    elif args.normalize_adv or args.clip != 0.2:
        raise SystemExit("train_breakout: --clip and --normalize-adv belong to --objective surrogate")
    global TARGET
    if args.target_period is not None:
        if args.objective != "surrogate":
            raise SystemExit("train_breakout: --target-period needs --objective surrogate (the target network serves that objective)")
        if args.target_period < 1 or not 0.0 < args.target_tau <= 1.0:
            raise SystemExit("train_breakout: --target-period P >= 1, --target-tau TAU in (0, 1]")
        TARGET = (args.target_period, args.target_tau)
        configs += ("rmsprop_surrogate_target",)
    elif args.target_tau != 1.0:
        raise SystemExit("train_breakout: --target-tau belongs to --target-period")
    global KL
    if args.kl_coeff is not None:
        if not 0.0 <= args.kl_coeff < float("inf") or not 0.0 < args.kl_target < float("inf"):
            raise SystemExit("train_breakout: --kl-coeff C is finite and >= 0, --kl-target D finite and > 0")
        if args.kl_reference == "target" and args.target_period is None:
            raise SystemExit("train_breakout: --kl-reference target needs --target-period (the target network is the reference)")
        KL = dict(reference=args.kl_reference, coeff=args.kl_coeff, kl_target=args.kl_target, adapt=not args.kl_fixed)
        configs += (configs[-1] + "_kl",)
    elif args.kl_fixed or args.kl_target != 0.01 or args.kl_reference != "behaviour":
        raise SystemExit("train_breakout: --kl-target, --kl-reference and --kl-fixed belong to --kl-coeff")
    if args.n_fresh is not None:
        if not 1 <= args.n_fresh < N or N % args.n_fresh:
            raise SystemExit(f"train_breakout: --n-fresh K divides the batch {N} and is smaller than it")
        if args.overlap or args.diagnostics or args.popart is not None:
            raise SystemExit("train_breakout: --n-fresh is a loop of its own; run --overlap, --diagnostics and --popart apart")
        configs = tuple(c for c in configs if c != "adam")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", default_out(args, bool(ex), default_mode))
    if hip.device_count() < 1:
        raise SystemExit("train_breakout: no HIP device; nothing is measured without one")
    t0 = time.perf_counter()
    base = untrained(args.window)
    if args.n_fresh is not None:
        runs = {c: train_replay(c, args.unrolls, args.window, args.n_fresh, args.publish, ex) for c in configs}
    elif args.overlap:
        runs = {c: train_overlapped(c, args.unrolls, args.window, ex, args.diagnostics) for c in configs}
    else:
        runs = {c: train(c, args.unrolls, args.window, args.publish, ex, args.diagnostics) for c in configs}
    res = dict(what="learning measurement on an environment that needs the frame stack: the Atari policy on "
                    "device-resident Breakout, mean score of the episodes finished in every window of unrolls; " +
                    ("two" if args.n_fresh is None else f"the replaying loop, {len(configs)}") +
                    " documented settings, nothing tuned, no threshold",
               num_envs=N, batch=N, seq_len=T, num_actions=A, gamma=GAMMA, seed=SEED, max_steps=MAX_STEPS,
               unrolls=args.unrolls, window_unrolls=args.window, return_range=[0, MAX_STEPS],
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
                                                    normalize_advantages="_normalized" in c))
            if "_target" in c:
                res["configs"][c]["target"] = dict(period=TARGET[0], tau=TARGET[1])
    if KL is not None:
        c = configs[-1]
        res["configs"][c] = dict(res["configs"].get(c) or res["configs"][c.removesuffix("_kl")],
                                 kl=dict(KL, band=1.5, factor=2.0, coeff_min=2.0 ** -20, coeff_max=2.0 ** 20))
    if args.n_fresh is not None:
        res["configs"].pop("adam", None)
        steps = 1 + (args.unrolls - 1) * (N // args.n_fresh)
        for c in res["configs"].values():
            c["lr_steps"] = steps
        res.update(replay=dict(n_fresh=args.n_fresh, steps_per_unroll=N // args.n_fresh, ring_entries=RING_UNROLLS * N,
                               note="the first unroll is one step with every column fresh"))
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
