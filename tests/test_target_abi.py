"""CPU-side checks of the target network's ABI (include/fi_target.h): the in-tree libfi_learner.so exports
exactly the functions the header declares, freeimpala_amd.target binds exactly that set, none of it is in an
older header or table, the two structures have one layout in C and in ctypes, and target_reference /
update_reference -- the host form of the rule -- on hand-computed cases, against torch autograd of the loss it
reports, against surrogate_reference for the targets, and against the oracle's V-trace where pi_tgt = pi."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_surrogate_abi import HP as SUR_HP, OTHER_HEADERS, header_functions, rand_case as sur_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("fi_target_enable", "fi_target_disable", "fi_target_sync", "fi_target_get_params", "fi_target_set_params",
             "fi_target_get_state", "fi_target_params_dev", "fi_target_logits_dev", "fi_target_stats_dev",
             "fi_target_workspace_bytes", "fi_target_loss_fp32", "fi_target_update")
PARAM_FIELDS = ["period", "tau", "reserved"]
STATS_FIELDS = ["updates", "rows", "mean_log_r", "mean_sq_log_r"]
HP = dict(SUR_HP, pg_rho_bar=1.1)  # a finite pg_rho_bar inside the spread of rho: beta = min(pg_rho_bar, rho_t) bites
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def rand_case(seed, T, B, A):
    """test_surrogate_abi's case with tgt = pi + 0.3 noise' and mu = tgt + 0.5 noise."""
    pi, _, act, rew, disc, val = sur_case(seed, T, B, A)
    rs = np.random.RandomState(seed + 1)
    tgt = (pi + 0.3 * rs.randn(T, B, A)).astype(np.float32)
    mu = (tgt + 0.5 * rs.randn(T, B, A)).astype(np.float32)
    return pi, tgt, mu, act, rew, disc, val


def test_library_exports_exactly_the_target_header():
    from freeimpala_amd import (_abi, actor, breakout, diag, env, explore, farmer, gather, popart, prio, publish, ring,
                                rollout, surrogate, target, train, weights)
    lib = target.lib()
    names = header_functions("fi_target.h")
    assert names == sorted(FUNCTIONS)
    assert all(n.startswith("fi_target_") for n in names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(target.SIGNATURES), set(names) ^ set(target.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_target_")} == set(names)
    # a header of its own: no older header and no older table gains a function
    others = OTHER_HEADERS + ("fi_surrogate.h",)
    for other in others:
        assert not set(names) & set(header_functions(other)), other
    tables = (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish, explore, diag, popart,
              surrogate)
    for mod in tables:
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(surrogate.SIGNATURES) == 7 and len(popart.SIGNATURES) == 9
    assert lib.fi_abi_version() == 1


def test_struct_layouts_match_c(tmp_path):
    from freeimpala_amd import target
    assert [f for f, _ in target.TargetParams._fields_] == PARAM_FIELDS
    assert [f for f, _ in target.TargetStats._fields_] == STATS_FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_target.h"\nint main(){'
           'printf("%zu", sizeof(fi_target_params));' +
           "".join(f'printf(" %zu", offsetof(fi_target_params, {f}));' for f in PARAM_FIELDS) +
           'printf(" %zu", sizeof(fi_target_stats));' +
           "".join(f'printf(" %zu", offsetof(fi_target_stats, {f}));' for f in STATS_FIELDS) +
           'printf(" %u %.17g", FI_TARGET_PERIOD, (double)FI_TARGET_TAU);}')
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out[:-2]]
    P, S = target.TargetParams, target.TargetStats
    assert got == ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAM_FIELDS] +
                   [ctypes.sizeof(S)] + [getattr(S, f).offset for f in STATS_FIELDS])
    assert got == [16, 0, 4, 8, 32, 0, 8, 16, 24]
    assert (int(out[-2]), float(out[-1])) == (target.PERIOD, target.TAU)
    p = target.params()
    assert (p.period, p.tau, list(p.reserved)) == (4, 1.0, [0, 0])
    raw = np.frombuffer(np.array([3, 80], np.uint64).tobytes() + np.array([-0.5, 0.75]).tobytes(), np.uint8)
    assert raw.nbytes == target.STATS_BYTES == 32
    assert target.unpack_stats(raw) == dict(updates=3, rows=80, mean_log_r=-0.5, mean_sq_log_r=0.75)
    assert S(3, 80, -0.5, 0.75).as_dict() == target.unpack_stats(raw)


def test_workspace_needs_no_device():
    from freeimpala_amd import surrogate, target
    assert target.workspace_bytes(5, 24, 1) == 0 and target.workspace_bytes(5, 24, 65) == 0
    assert target.workspace_bytes(0, 4, 4) == 0 and target.workspace_bytes(2 ** 15, 2 ** 15, 2) == 0
    for T, B, A in ((1, 1, 3), (5, 24, 18), (7, 65, 64), (100, 4096, 18)):
        ws, sur = target.workspace_bytes(T, B, A), surrogate.workspace_bytes(T, B, A)
        assert ws % 256 == 0 and ws >= sur + 2 * 24 * surrogate.loss_blocks(T, B, A)


def hand_case(r, r0):
    """T = 2, B = 1, A = 2: V = (1, 2, 4), g = 0.5, the action is 0 on both rows. Row 1: pi = pi_tgt = mu, reward 1.
    Row 0: pi_tgt(0) = 1/2, mu(0) = 1/4 (rho_t = 2), pi(0) = r / 2, reward r0."""
    pi = np.zeros((2, 1, 2), np.float32)
    tgt = np.zeros((2, 1, 2), np.float32)
    mu = np.zeros((2, 1, 2), np.float32)
    mu[0, 0, 1] = np.log(3.0)          # 1 / (1 + 3) = 1/4
    pi[0, 0, 1] = np.log(2.0 / r - 1)  # 1 / (1 + 2/r - 1) = r/2
    return (pi, tgt, mu, np.zeros((2, 1), np.int32), np.array([[r0], [1.0]], np.float32), np.full((2, 1), 0.5, np.float32),
            np.array([[1.0], [2.0], [4.0]], np.float32))


def test_target_reference_by_hand():
    """rho_bar = c_bar = lambda = 1, pg_rho_bar = 1.5. Row 1: everything is 1: acc = 1 + 0.5 * 4 - 2 = 1, vs = 3, A = 1,
    beta = 1. Row 0, rho_t = 2: rho^ = c = 1, acc = (r0 + 0.5 * 2 - 1) + 0.5 * 1 = r0 + 0.5, vs = r0 + 1.5,
    A = r0 + 0.5 * 3 - 1 = r0 + 0.5, beta = 1.5."""
    from freeimpala_amd.target import near_rows, target_reference
    hp = dict(rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.5, lambda_=1.0, baseline_cost=0.5, entropy_cost=0.0)
    # clipped from above: r = 1.5 > 1.25, A = 1.5 > 0
    case = hand_case(1.5, 1.0)
    t = target_reference(*case, hp, clip=0.25)
    np.testing.assert_allclose(t["r"][:, 0], [1.5, 1.0], rtol=1e-6)
    np.testing.assert_allclose(t["rho"][:, 0], [2.0, 1.0], rtol=1e-6)
    np.testing.assert_allclose(t["beta"][:, 0], [1.5, 1.0], rtol=1e-6)
    np.testing.assert_allclose(t["vs"][:, 0], [2.5, 3.0], rtol=1e-6)
    np.testing.assert_allclose(t["pg_adv"][:, 0], [1.5, 1.0], rtol=1e-6)
    assert t["clipped"][:, 0].tolist() == [True, False] and t["rows_clipped"] == 1 and t["rows"] == 2 and t["bad"] == 0
    np.testing.assert_allclose(t["losses"], [-1.5 * (1.25 * 1.5) - 1.0, 0.5 * (1.5 ** 2 + 1.0),
                                             0.75 * np.log(0.75) + 0.25 * np.log(0.25) + np.log(0.5)], rtol=1e-6)
    np.testing.assert_allclose(t["dlogits"][0, 0], [0.0, 0.0], atol=1e-12)  # clipped: no policy gradient
    np.testing.assert_allclose(t["dlogits"][1, 0], [-0.5, 0.5], rtol=1e-6)  # g = -1: -(1 - 1/2), -(0 - 1/2)
    np.testing.assert_allclose(t["dvalue"][:, 0], [0.5 * (1 - 2.5), 0.5 * (2 - 3), 0.0], rtol=1e-6)
    np.testing.assert_allclose([t["mean_log_r"], t["mean_sq_log_r"]], [np.log(1.5) / 2, np.log(1.5) ** 2 / 2], rtol=1e-6)
    assert near_rows(*case, hp, clip=0.25) == 0 and near_rows(*case, hp, clip=0.5) == 1  # hi = 1.5 = r
    # clipped from below: r = 1/2 < 0.75, A = -2 + 0.5 = -1.5 < 0
    t = target_reference(*hand_case(0.5, -2.0), hp, clip=0.25)
    np.testing.assert_allclose(t["r"][:, 0], [0.5, 1.0], rtol=1e-6)
    np.testing.assert_allclose(t["pg_adv"][:, 0], [-1.5, 1.0], rtol=1e-6)
    assert t["clipped"][:, 0].tolist() == [True, False]
    np.testing.assert_allclose(t["losses"][0], 1.5 * (0.75 * 1.5) - 1.0, rtol=1e-6)  # -1.5 min(-0.75, -1.125)
    np.testing.assert_allclose(t["dlogits"][0, 0], [0.0, 0.0], atol=1e-12)
    # active: r = 1.5 with A = -1.5 is not clipped (the ratio moved against the advantage): g = 1.5 * 1.5 * 1.5
    t = target_reference(*hand_case(1.5, -2.0), hp, clip=0.25)
    assert t["clipped"].sum() == 0
    np.testing.assert_allclose(t["losses"][0], 3.375 - 1.0, rtol=1e-6)  # -1.5 min(-2.25, -1.875)
    np.testing.assert_allclose(t["dlogits"][0, 0], [3.375 * 0.25, -3.375 * 0.25], rtol=1e-6)  # g (1 - 3/4), g (0 - 1/4)
    # normalised: m = -0.25, s = 1.25: A~ = (-1, 1); a bad action is clamped and counted
    t = target_reference(*hand_case(1.5, -2.0), hp, clip=0.25, normalize=True, adv_eps=0.0)
    np.testing.assert_allclose(t["adv_used"][:, 0], [-1.0, 1.0], rtol=1e-6)
    np.testing.assert_allclose(t["losses"][0], 1.5 * 1.5 - 1.0, rtol=1e-6)
    case = list(hand_case(1.5, -2.0))
    case[3] = np.array([[2], [-1]], np.int32)
    t = target_reference(*case, hp)
    assert t["bad"] == 2 and np.isfinite(t["dlogits"]).all()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64)], ids=ids)
def test_reference_gradients_are_autograd_of_its_loss(shape, normalize):
    """dlogits and dvalue against torch autograd, in fp64 with beta, the advantages and the targets detached, of the
    total loss the reference reports: max abs difference <= 1e-12 max(1, |ref|), the surrogate's bar."""
    import torch
    from freeimpala_amd.surrogate import clip_bounds
    from freeimpala_amd.target import target_reference
    T, B, A = shape
    pi, tgt, mu, act, rew, disc, val = rand_case(100 * T + A, T, B, A)
    t = target_reference(pi, tgt, mu, act, rew, disc, val, HP, clip=0.2, normalize=normalize)
    assert 0 < t["rows_clipped"] < t["rows"] and (t["beta"] < t["rho"]).any() and (t["beta"] == t["rho"]).any()
    z = torch.tensor(pi, dtype=torch.float64, requires_grad=True)
    v = torch.tensor(val, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(act, dtype=torch.int64)[..., None]
    lpi = torch.log_softmax(z, -1)
    ltg = torch.log_softmax(torch.tensor(tgt, dtype=torch.float64), -1)
    r = torch.exp(lpi.gather(-1, a)[..., 0] - ltg.gather(-1, a)[..., 0])
    adv, vs, beta = torch.tensor(t["adv_used"]), torch.tensor(t["vs"]), torch.tensor(t["beta"])  # detached
    lo, hi = clip_bounds(0.2)
    l_pg = -(beta * torch.minimum(r * adv, torch.clamp(r, lo, hi) * adv)).sum()
    base = 0.5 * ((vs - v[:T]) ** 2).sum()
    ent = (torch.exp(lpi) * lpi).sum()
    total = l_pg + HP["baseline_cost"] * base + HP["entropy_cost"] * ent
    total.backward()
    for got, want, nm in ((l_pg.item(), t["losses"][0], "pg"), (base.item(), t["losses"][1], "baseline"),
                          (ent.item(), t["losses"][2], "entropy")):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (nm, got, want)
    for got, want, nm in ((z.grad.numpy(), t["dlogits"], "dlogits"), (v.grad.numpy(), t["dvalue"], "dvalue")):
        err = np.abs(got - want).max()
        print(f"{nm}: max abs difference {err:.3e}, bar {1e-12 * max(1.0, np.abs(want).max()):.3e}")
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), nm


@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64)], ids=ids)
def test_with_the_target_equal_to_pi_it_is_the_oracles_vtrace(orc, shape):
    """pi_tgt bit-equal to pi: r = 1 and nothing is clipped, both exactly, whatever the clip; and vs, dlogits, dvalue
    are the oracle's vtrace_loss at the same hyper-parameters, the finite pg_rho_bar included, inside the bar of
    test_reference_equals_the_oracles_vtrace_without_a_clip: the oracle's fp32 rounding of its outputs, 2^-24 |x|,
    plus 1e-12 max(1, |x|) for the two fp64 evaluation orders."""
    from freeimpala_amd.target import target_reference
    T, B, A = shape
    pi, _, mu, act, rew, disc, val = rand_case(7 * T + A, T, B, A)
    t = target_reference(pi, pi.copy(), mu, act, rew, disc, val, HP, clip=0.01, normalize=False)
    assert (t["r"] == 1.0).all() and (t["log_r"] == 0.0).all() and t["rows_clipped"] == 0 and not t["clipped"].any()
    assert t["mean_log_r"] == 0.0 and t["mean_sq_log_r"] == 0.0
    assert (t["beta"] < t["rho"]).any(), "the finite pg_rho_bar bites"
    o = orc.vtrace_loss(pi, mu, act, rew, disc, val, **HP)
    for k in ("vs", "dlogits", "dvalue"):
        want = o[k].astype(np.float64)
        bar = 2.0 ** -24 * np.abs(want) + 1e-12 * np.maximum(1.0, np.abs(want))
        ratio = (np.abs(t[k] - want) / bar).max()
        print(f"{k}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0, k
    np.testing.assert_allclose(t["pg_adv"] * t["beta"], o["pg_adv"], rtol=1e-6, atol=1e-6)  # V-trace's carries the factor
    for i in (1, 2):
        assert abs(t["losses"][i] - o["losses"][i]) <= 1e-12 * max(1.0, abs(o["losses"][i]))


@pytest.mark.parametrize("normalize", [False, True])
def test_the_targets_are_the_surrogates_on_the_target_logits(normalize):
    from freeimpala_amd.surrogate import surrogate_reference
    from freeimpala_amd.target import target_reference
    pi, tgt, mu, act, rew, disc, val = rand_case(3, 5, 24, 18)
    t = target_reference(pi, tgt, mu, act, rew, disc, val, HP, 0.2, normalize)
    s = surrogate_reference(tgt, mu, act, rew, disc, val, HP, 0.2, normalize)
    for k in ("vs", "pg_adv", "adv_used", "rho", "log_rho", "dvalue"):
        np.testing.assert_array_equal(t[k], s[k], err_msg=k)
    assert (t["adv_mean"], t["adv_std"], t["losses"][1]) == (s["adv_mean"], s["adv_std"], s["losses"][1])
    assert set(s) | {"r", "log_r", "beta", "mean_log_r", "mean_sq_log_r"} == set(t)


def test_update_reference():
    from freeimpala_amd.target import update_reference
    rs = np.random.RandomState(0)
    p, t = rs.randn(1027).astype(np.float32), rs.randn(1027).astype(np.float32)
    one = update_reference(p, t, 1.0)
    assert one.dtype == np.float64 and np.array_equal(one.astype(np.float32).view(np.uint32), p.view(np.uint32))
    q = update_reference(p, t, 0.25)
    exact = t.astype(np.float64) + 0.25 * (p.astype(np.float64) - t.astype(np.float64))
    # it differs from the exact step by the one fp32 rounding of the difference: 0.25 * 2^-24 |p - t|
    assert (np.abs(q - exact) <= 0.25 * 2.0 ** -24 * np.abs(p.astype(np.float64) - t)).all() and (q != exact).any()
    np.testing.assert_array_equal(update_reference(p, p, 0.25), p.astype(np.float64))  # a fixed point


def test_train_breakout_keeps_every_comparisons_record_apart():
    """scripts/train_breakout.py without --out: the replaying loop and the target network write their own file, also
    with --objective surrogate, whose own record (quoted in README and DESIGN) a target run must not overwrite."""
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_breakout", os.path.join(ROOT, "scripts", "train_breakout.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)

    def out(**kw):
        a = dict(n_fresh=None, target_period=None, objective="vtrace", popart=None, diagnostics=0)
        a.update(kw)
        return tb.default_out(argparse.Namespace(**a), False, True)

    assert out() == "train_breakout.json"
    assert out(objective="surrogate") == "train_breakout_surrogate.json"
    assert out(objective="surrogate", n_fresh=128, target_period=4) == "train_breakout_target.json"
    assert out(objective="surrogate", target_period=4) == "train_breakout_target.json"
    assert out(n_fresh=128) == "train_breakout_target.json"
    assert out(popart=3e-4) == "train_breakout_popart.json" and out(diagnostics=5) == "train_breakout_diag.json"
    assert tb.default_out(argparse.Namespace(n_fresh=None, target_period=None, objective="vtrace", popart=None,
                                             diagnostics=0), True, True) == "train_breakout_explore.json"
    assert tb.default_out(argparse.Namespace(n_fresh=None, target_period=None, objective="vtrace", popart=None,
                                             diagnostics=0), False, False) == "train_breakout_device_publish.json"
