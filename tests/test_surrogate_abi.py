"""CPU-side checks of the clipped surrogate objective's ABI (include/fi_surrogate.h): the in-tree
libfi_learner.so exports exactly the functions the header declares, freeimpala_amd.surrogate binds exactly
that set, none of it is in an older header or table, the two structures have one layout in C and in
ctypes, and surrogate_reference -- the host form of the rule -- on hand-computed cases, against torch
autograd of the loss it reports, and against the oracle's V-trace where the two rules coincide."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h", "fi_train.h", "fi_breakout.h", "fi_publish.h", "fi_explore.h", "fi_diag.h",
                 "fi_popart.h")
FUNCTIONS = ("fi_surrogate_enable", "fi_surrogate_disable", "fi_surrogate_get_state", "fi_surrogate_stats_dev",
             "fi_surrogate_workspace_bytes", "fi_surrogate_loss_blocks", "fi_surrogate_loss_fp32")
PARAM_FIELDS = ["clip", "normalize", "adv_eps", "reserved"]
STATE_FIELDS = ["enabled", "normalize", "clip", "adv_eps", "rows", "rows_clipped", "adv_mean", "adv_std"]
HP = dict(rho_bar=1.3, c_bar=0.9, lambda_=1.0, baseline_cost=0.5, entropy_cost=0.01)  # test_gpu_diag.BARS


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_surrogate_header():
    from freeimpala_amd import (_abi, actor, breakout, diag, env, explore, farmer, gather, popart, prio, publish, ring,
                                rollout, surrogate, train, weights)
    lib = surrogate.lib()
    names = header_functions("fi_surrogate.h")
    assert names == sorted(FUNCTIONS)
    assert all(n.startswith("fi_surrogate_") for n in names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(surrogate.SIGNATURES), set(names) ^ set(surrogate.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_surrogate_")} == set(names)
    # a header of its own: no older header and no older table gains a function
    assert len(OTHER_HEADERS) == 15 and all(os.path.exists(os.path.join(ROOT, "include", h)) for h in OTHER_HEADERS)
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    tables = (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish, explore, diag, popart)
    assert len(tables) == 15
    for mod in tables:
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(popart.SIGNATURES) == 9 and len(diag.SIGNATURES) == 6
    assert lib.fi_abi_version() == 1


def test_struct_layouts_match_c(tmp_path):
    from freeimpala_amd import surrogate
    assert [f for f, _ in surrogate.SurrogateParams._fields_] == PARAM_FIELDS
    assert [f for f, _ in surrogate.SurrogateState._fields_] == STATE_FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_surrogate.h"\nint main(){'
           'printf("%zu", sizeof(fi_surrogate_params));' +
           "".join(f'printf(" %zu", offsetof(fi_surrogate_params, {f}));' for f in PARAM_FIELDS) +
           'printf(" %zu", sizeof(fi_surrogate_state));' +
           "".join(f'printf(" %zu", offsetof(fi_surrogate_state, {f}));' for f in STATE_FIELDS) +
           'printf(" %.17g %.17g", (double)FI_SURROGATE_CLIP, (double)FI_SURROGATE_ADV_EPS);}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out[:-2]]
    P, S = surrogate.SurrogateParams, surrogate.SurrogateState
    assert got == ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAM_FIELDS] +
                   [ctypes.sizeof(S)] + [getattr(S, f).offset for f in STATE_FIELDS])
    assert got == [16, 0, 4, 8, 12, 48, 0, 4, 8, 12, 16, 24, 32, 40]
    assert [float(v) for v in out[-2:]] == [float(np.float32(surrogate.CLIP)), float(np.float32(surrogate.ADV_EPS))]
    d = S(1, 1, 0.25, 0.5, 80, 7, -1.5, 2.5).as_dict()
    assert d == dict(enabled=True, normalize=True, clip=0.25, adv_eps=0.5, rows=80, rows_clipped=7, adv_mean=-1.5,
                     adv_std=2.5)
    raw = np.frombuffer(np.array([80, 7], np.uint64).tobytes() + np.array([-1.5, 2.5]).tobytes(), np.uint8)
    assert raw.nbytes == surrogate.STATS_BYTES == 32
    assert surrogate.unpack_stats(raw) == dict(rows=80, rows_clipped=7, adv_mean=-1.5, adv_std=2.5)
    p = surrogate.params()
    assert (p.clip, p.normalize, p.adv_eps, p.reserved) == (np.float32(0.2), 0, np.float32(1e-8), 0)


def test_plan_and_workspace_need_no_device():
    from freeimpala_amd import surrogate
    assert surrogate.loss_blocks(1, 1, 3) == 1 and surrogate.scan_blocks(1) == 1
    assert surrogate.loss_blocks(5, 24, 1) == 0 and surrogate.loss_blocks(5, 24, 65) == 0 and surrogate.loss_blocks(0, 4, 4) == 0
    assert surrogate.workspace_bytes(5, 24, 1) == 0 and surrogate.workspace_bytes(2 ** 15, 2 ** 15, 2) == 0
    # column tiles of 64 times slices of whole rounds of four time steps
    assert surrogate.loss_blocks(33, 72, 18) == 2 * 9 and surrogate.loss_blocks(9, 200, 5) == 4 * 3
    assert surrogate.loss_blocks(100, 4096, 18) == 64 * 9 and surrogate.scan_blocks(4096) == 64
    for T, B, A in ((1, 1, 3), (5, 24, 18), (7, 65, 64), (100, 4096, 18)):
        ws = surrogate.workspace_bytes(T, B, A)
        assert ws % 256 == 0 and ws >= 3 * 4 * T * B + 16 * surrogate.scan_blocks(B) + 32 * surrogate.loss_blocks(T, B, A)


def hand_case(log_ratio, r0):
    """T = 2, B = 1, A = 2: V = (1, 2, 4), g = 0.5, the action is 0 on both rows; row 1 is on-policy with reward
    1, row 0 has log rho = log_ratio and reward r0."""
    pi = np.zeros((2, 1, 2), np.float32)
    mu = np.zeros((2, 1, 2), np.float32)
    # log pi[0] - log mu[0] with pi = (0, 0): log 1/2 - log_softmax(mu)[0]; mu = (0, x) gives -log(1 + e^x)
    with np.errstate(divide="ignore"):  # rho = 1/2: x = -inf, mu puts everything on action 0
        mu[0, 0, 1] = np.log(np.expm1(np.log(2.0) + log_ratio))
    return (pi, mu, np.zeros((2, 1), np.int32), np.array([[r0], [1.0]], np.float32), np.full((2, 1), 0.5, np.float32),
            np.array([[1.0], [2.0], [4.0]], np.float32))


def test_surrogate_reference_by_hand():
    """rho_bar = c_bar = lambda = 1. Row 1: rho = 1, acc = 1 + 0.5 * 4 - 2 = 1, vs = 3, A = 1. Row 0 with rho = 2:
    rho^ = c = 1, acc = (r + 0.5 * 2 - 1) + 0.5 * 1 = r + 0.5, vs = r + 1.5, A = r + 0.5 * 3 - 1 = r + 0.5."""
    from freeimpala_amd.surrogate import near_rows, surrogate_reference
    hp = dict(rho_bar=1.0, c_bar=1.0, lambda_=1.0, baseline_cost=0.5, entropy_cost=0.0)
    # clipped from above: rho = 2 > 1.25, A = 1.5 > 0
    case = hand_case(np.log(2.0), 1.0)
    r = surrogate_reference(*case, hp, clip=0.25)
    np.testing.assert_allclose(r["rho"][:, 0], [2.0, 1.0], rtol=1e-6)
    np.testing.assert_allclose(r["vs"][:, 0], [2.5, 3.0], rtol=1e-6)
    np.testing.assert_allclose(r["pg_adv"][:, 0], [1.5, 1.0], rtol=1e-6)
    assert r["clipped"][:, 0].tolist() == [True, False] and r["rows_clipped"] == 1 and r["rows"] == 2 and r["bad"] == 0
    np.testing.assert_allclose(r["losses"], [-(1.25 * 1.5) - 1.0, 0.5 * (1.5 ** 2 + 1.0), 2 * np.log(0.5)], rtol=1e-6)
    np.testing.assert_allclose(r["dlogits"][0, 0], [0.0, 0.0], atol=1e-12)      # clipped: no policy gradient
    np.testing.assert_allclose(r["dlogits"][1, 0], [-0.5, 0.5], rtol=1e-6)      # g = -1: -(1 - 1/2), -(0 - 1/2)
    np.testing.assert_allclose(r["dvalue"][:, 0], [0.5 * (1 - 2.5), 0.5 * (2 - 3), 0.0], rtol=1e-6)
    np.testing.assert_allclose([r["adv_mean"], r["adv_std"]], [1.25, 0.25], rtol=1e-6)
    assert near_rows(*case, hp, clip=0.25) == 0 and near_rows(*case, hp, clip=1.0) == 1  # hi = 2 = rho
    # clipped from below: rho = 1/2 < 0.75, A = -2 + 0.5 = -1.5 < 0
    r = surrogate_reference(*hand_case(np.log(0.5), -2.0), hp, clip=0.25)
    np.testing.assert_allclose(r["rho"][:, 0], [0.5, 1.0], rtol=1e-6)
    np.testing.assert_allclose(r["pg_adv"][:, 0], [-1.5, 1.0], rtol=1e-6)       # acc = 0.5 (-2) + 0.5 * 0.5 = -0.75
    np.testing.assert_allclose(r["vs"][:, 0], [0.25, 3.0], rtol=1e-6)
    assert r["clipped"][:, 0].tolist() == [True, False]
    np.testing.assert_allclose(r["losses"][0], 0.75 * 1.5 - 1.0, rtol=1e-6)     # -min(-0.75, -1.125) = 1.125
    np.testing.assert_allclose(r["dlogits"][0, 0], [0.0, 0.0], atol=1e-12)
    # active: rho = 2 with A = -1.5 is not clipped (the ratio moved against the advantage): g = 2 * 1.5 = 3
    r = surrogate_reference(*hand_case(np.log(2.0), -2.0), hp, clip=0.25)
    np.testing.assert_allclose(r["pg_adv"][:, 0], [-1.5, 1.0], rtol=1e-6)
    assert r["clipped"].sum() == 0
    np.testing.assert_allclose(r["losses"][0], 3.0 - 1.0, rtol=1e-6)            # -min(-3, -1.875) = 3
    np.testing.assert_allclose(r["dlogits"][0, 0], [1.5, -1.5], rtol=1e-6)      # 3 (1 - 1/2), 3 (0 - 1/2)
    # normalised: m = -0.25, s = 1.25: A~ = (-1, 1); a bad action is clamped and counted
    r = surrogate_reference(*hand_case(np.log(2.0), -2.0), hp, clip=0.25, normalize=True, adv_eps=0.0)
    np.testing.assert_allclose(r["adv_used"][:, 0], [-1.0, 1.0], rtol=1e-6)
    np.testing.assert_allclose(r["pg_adv"][:, 0], [-1.5, 1.0], rtol=1e-6)
    case = list(hand_case(np.log(2.0), -2.0))
    case[2] = np.array([[2], [-1]], np.int32)
    r = surrogate_reference(*case, hp)
    assert r["bad"] == 2 and np.isfinite(r["dlogits"]).all()


def rand_case(seed, T, B, A):
    rs = np.random.RandomState(seed)
    pi = rs.randn(T, B, A).astype(np.float32)
    mu = (pi + 0.5 * rs.randn(T, B, A)).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.choice([-1.0, 0.0, 1.0], (T, B)).astype(np.float32)
    disc = np.where(rs.rand(T, B) < 0.05, 0.0, 0.99).astype(np.float32)
    val = rs.randn(T + 1, B).astype(np.float32)
    return pi, mu, act, rew, disc, val


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64)], ids=lambda s: "x".join(map(str, s)))
def test_reference_gradients_are_autograd_of_its_loss(shape, normalize):
    """dlogits and dvalue against torch autograd, in fp64 with the advantages and the targets detached, of the total
    loss the reference reports: max abs difference <= 1e-12 max(1, |ref|)."""
    import torch
    from freeimpala_amd.surrogate import clip_bounds, surrogate_reference
    T, B, A = shape
    pi, mu, act, rew, disc, val = rand_case(100 * T + A, T, B, A)
    r = surrogate_reference(pi, mu, act, rew, disc, val, HP, clip=0.2, normalize=normalize)
    assert 0 < r["rows_clipped"] < r["rows"]
    z = torch.tensor(pi, dtype=torch.float64, requires_grad=True)
    v = torch.tensor(val, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(act, dtype=torch.int64)[..., None]
    lpi = torch.log_softmax(z, -1)
    lmu = torch.log_softmax(torch.tensor(mu, dtype=torch.float64), -1)
    rho = torch.exp(lpi.gather(-1, a)[..., 0] - lmu.gather(-1, a)[..., 0])
    adv, vs = torch.tensor(r["adv_used"]), torch.tensor(r["vs"])  # detached
    lo, hi = clip_bounds(0.2)
    l_pg = -torch.minimum(rho * adv, torch.clamp(rho, lo, hi) * adv).sum()
    base = 0.5 * ((vs - v[:T]) ** 2).sum()
    ent = (torch.exp(lpi) * lpi).sum()
    total = l_pg + HP["baseline_cost"] * base + HP["entropy_cost"] * ent
    total.backward()
    for got, want, nm in ((l_pg.item(), r["losses"][0], "pg"), (base.item(), r["losses"][1], "baseline"),
                          (ent.item(), r["losses"][2], "entropy")):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (nm, got, want)
    for got, want, nm in ((z.grad.numpy(), r["dlogits"], "dlogits"), (v.grad.numpy(), r["dvalue"], "dvalue")):
        err = np.abs(got - want).max()
        print(f"{nm}: max abs difference {err:.3e}, bar {1e-12 * max(1.0, np.abs(want).max()):.3e}")
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), nm


@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64)], ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_the_oracles_vtrace_without_a_clip(orc, shape):
    """clip = 1e30, normalize = 0 against the oracle's vtrace_loss at pg_rho_bar = 1e30. The oracle computes in
    fp64 and hands vs, dlogits and dvalue back rounded to fp32: half an ulp, 2^-24 |x|, is what its outputs can say.
    The bar is that plus 1e-12 max(1, |x|) for the two fp64 evaluation orders -- far inside the oracle's TOL of 1e-5."""
    from freeimpala_amd.surrogate import surrogate_reference
    T, B, A = shape
    case = rand_case(7 * T + A, T, B, A)
    r = surrogate_reference(*case, HP, clip=1e30, normalize=False)
    o = orc.vtrace_loss(*case, rho_bar=HP["rho_bar"], c_bar=HP["c_bar"], pg_rho_bar=1e30, lambda_=HP["lambda_"],
                        baseline_cost=HP["baseline_cost"], entropy_cost=HP["entropy_cost"])
    assert r["rows_clipped"] == 0
    for k in ("vs", "dlogits", "dvalue"):
        want = o[k].astype(np.float64)
        bar = 2.0 ** -24 * np.abs(want) + 1e-12 * np.maximum(1.0, np.abs(want))
        ratio = (np.abs(r[k] - want) / bar).max()
        print(f"{k}: worst error / bar {ratio:.3f}")
        assert ratio <= 1.0, k
    # pg_adv differs by the rho factor V-trace's carries
    np.testing.assert_allclose(r["pg_adv"] * r["rho"], o["pg_adv"], rtol=1e-6, atol=1e-6)
    for i in (1, 2):
        assert abs(r["losses"][i] - o["losses"][i]) <= 1e-12 * max(1.0, abs(o["losses"][i]))
