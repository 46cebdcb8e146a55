"""CPU-side checks of the KL penalty's ABI (include/fi_kl.h): the in-tree libfi_learner.so exports exactly the
functions the header declares, freeimpala_amd.kl binds exactly that set, none of it is in an older header or table,
the two structures have one layout in C and in ctypes, and kl_reference / adapt_reference -- the host form of the
rule -- by hand, against torch autograd of c * sum kl, against the diagnostics' KL(mu || pi), and branch by branch."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from test_surrogate_abi import OTHER_HEADERS, header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("fi_kl_enable", "fi_kl_disable", "fi_kl_set_coeff", "fi_kl_get_state", "fi_kl_state_dev", "fi_kl_workspace_bytes",
             "fi_kl_penalty_fp32", "fi_kl_finalize")
PARAM_FIELDS = ["reference", "adapt", "coeff", "kl_target", "band", "factor", "coeff_min", "coeff_max"]
STATS_FIELDS = ["coeff", "mean_kl", "kl_sum", "rows", "updates", "raised", "lowered"]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def rand_case(seed, T, B, A):
    rs = np.random.RandomState(seed)
    pi = (2 * rs.randn(T, B, A)).astype(np.float32)
    q = (pi + 0.5 * rs.randn(T, B, A)).astype(np.float32)
    return pi, q, rs.randn(T, B, A).astype(np.float32)


def test_library_exports_exactly_the_kl_header():
    from freeimpala_amd import (_abi, actor, breakout, diag, env, explore, farmer, gather, kl, popart, prio, publish, ring,
                                rollout, surrogate, target, train, weights)
    lib = kl.lib()
    names = header_functions("fi_kl.h")
    assert names == sorted(FUNCTIONS)
    assert all(n.startswith("fi_kl_") for n in names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(kl.SIGNATURES), set(names) ^ set(kl.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_kl_")} == set(names)
    # a header of its own: no older header and no older table gains a function
    for other in OTHER_HEADERS + ("fi_surrogate.h", "fi_target.h"):
        assert not set(names) & set(header_functions(other)), other
    tables = (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish, explore, diag, popart,
              surrogate, target)
    for mod in tables:
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(target.SIGNATURES) == 12 and len(surrogate.SIGNATURES) == 7
    assert lib.fi_abi_version() == 1


def test_struct_layouts_match_c(tmp_path):
    from freeimpala_amd import kl
    assert [f for f, _ in kl.KlParams._fields_] == PARAM_FIELDS
    assert [f for f, _ in kl.KlStats._fields_] == STATS_FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_kl.h"\nint main(){'
           'printf("%zu", sizeof(fi_kl_params));' +
           "".join(f'printf(" %zu", offsetof(fi_kl_params, {f}));' for f in PARAM_FIELDS) +
           'printf(" %zu", sizeof(fi_kl_stats));' +
           "".join(f'printf(" %zu", offsetof(fi_kl_stats, {f}));' for f in STATS_FIELDS) +
           'printf(" %u %u", FI_KL_REF_BEHAVIOUR, FI_KL_REF_TARGET);'
           'printf(" %.17g %.17g %.17g %.17g %.17g %.17g", (double)FI_KL_COEFF, (double)FI_KL_TARGET, (double)FI_KL_BAND,'
           '(double)FI_KL_FACTOR, (double)FI_KL_COEFF_MIN, (double)FI_KL_COEFF_MAX);}')
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out[:-6]]
    P, S = kl.KlParams, kl.KlStats
    assert got == ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAM_FIELDS] +
                   [ctypes.sizeof(S)] + [getattr(S, f).offset for f in STATS_FIELDS] + [kl.REF_BEHAVIOUR, kl.REF_TARGET])
    assert got == [32, 0, 4, 8, 12, 16, 20, 24, 28, 48, 0, 8, 16, 24, 32, 40, 44, 0, 1]
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert [float(v) for v in out[-6:]] == [f32(kl.COEFF), f32(kl.KL_TARGET), f32(kl.BAND), f32(kl.FACTOR), kl.COEFF_MIN,
                                            kl.COEFF_MAX]
    assert (kl.COEFF_MIN, kl.COEFF_MAX) == (2.0 ** -20, 2.0 ** 20)
    p = kl.params()
    assert (p.reference, p.adapt, p.coeff, p.kl_target, p.band, p.factor, p.coeff_min, p.coeff_max) == \
        (0, 1, 1.0, f32(0.01), 1.5, 2.0, 2.0 ** -20, 2.0 ** 20)
    assert kl.params("target", adapt=False).reference == 1 and kl.params("target", adapt=False).adapt == 0
    raw = kl.pack_state(0.5, 0.25, 20.0, 80, 3, 2, 1)
    assert raw.nbytes == kl.STATE_BYTES == 48
    want = dict(coeff=0.5, mean_kl=0.25, kl_sum=20.0, rows=80, updates=3, raised=2, lowered=1)
    assert kl.unpack_state(raw) == want and S(0.5, 0.25, 20.0, 80, 3, 2, 1).as_dict() == want
    assert S.from_buffer_copy(raw.tobytes()).as_dict() == want


def test_workspace_needs_no_device():
    from freeimpala_amd import kl, surrogate
    assert kl.workspace_bytes(5, 24, 1) == 0 and kl.workspace_bytes(5, 24, 65) == 0
    assert kl.workspace_bytes(0, 4, 4) == 0 and kl.workspace_bytes(2 ** 15, 2 ** 15, 2) == 0
    for T, B, A in ((1, 1, 3), (5, 24, 18), (7, 65, 64), (100, 4096, 18)):
        ws = kl.workspace_bytes(T, B, A)
        assert ws % 256 == 0 and ws >= 8 * surrogate.loss_blocks(T, B, A) > 0  # the surrogate's grid: one partial each


def test_kl_reference_by_hand():
    """T = B = 1, A = 2: pi = (1/2, 1/2), q = (1/4, 3/4): kl = 1/4 ln(1/2) + 3/4 ln(3/2), gradient c (1/4, -1/4)."""
    from freeimpala_amd.kl import kl_reference
    pi = np.zeros((1, 1, 2), np.float32)
    q = np.array([[[0.0, np.log(3.0)]]], np.float32)
    d0 = np.array([[[0.5, -2.0]]], np.float32)
    for c in (1.0, 0.5, 4.0):
        r = kl_reference(pi, q, d0, c)
        want = 0.25 * np.log(0.5) + 0.75 * np.log(1.5)
        np.testing.assert_allclose(r["kl"], [[want]], rtol=1e-6)  # log(3) is a float
        np.testing.assert_allclose(r["dlogits"][0, 0], [0.5 + c * 0.25, -2.0 - c * 0.25], rtol=1e-6)
        assert r["rows"] == 1 and r["kl_sum"] == r["kl"][0, 0] == r["mean_kl"] and r["dlogits"].dtype == np.float64
    same = kl_reference(q, q.copy(), d0, 3.0)
    assert same["kl_sum"] == 0.0 and np.array_equal(same["dlogits"], d0.astype(np.float64))


@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64)], ids=ids)
def test_reference_gradient_is_autograd_of_the_penalty(shape):
    """dlogits - dlogits0 against torch autograd of c * sum kl in fp64: max abs difference <= 1e-12 max(1, |ref|), the
    bar test_target_abi.py uses for the same comparison; and kl against the diagnostics' KL(mu || pi)."""
    import torch
    from freeimpala_amd import diag
    from freeimpala_amd.kl import kl_reference
    T, B, A = shape
    pi, q, d0 = rand_case(100 * T + A, T, B, A)
    c = 0.75
    r = kl_reference(pi, q, d0, c)
    z = torch.tensor(pi, dtype=torch.float64, requires_grad=True)
    lq = torch.log_softmax(torch.tensor(q, dtype=torch.float64), -1)
    kl = (torch.exp(lq) * (lq - torch.log_softmax(z, -1))).sum(-1)
    (c * kl.sum()).backward()
    kl = kl.detach()
    want = d0.astype(np.float64) + z.grad.numpy()
    err, bar = np.abs(r["dlogits"] - want).max(), 1e-12 * max(1.0, np.abs(want).max())
    print(f"dlogits: max abs difference {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    err, bar = np.abs(r["kl"] - kl.numpy()).max(), 1e-12 * max(1.0, float(kl.max()))
    print(f"kl: max abs difference {err:.3e}, bar {bar:.3e}")
    assert err <= bar and abs(r["kl_sum"] - kl.sum().item()) <= 1e-12 * max(1.0, kl.sum().item())
    assert r["mean_kl"] == r["kl_sum"] / (T * B) and r["mean_kl"] > 0.05
    # the direction fi_diag.h reports: KL(mu || pi) with q in mu's place
    rs = np.random.RandomState(1)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    f = rs.randn(T, B).astype(np.float32)
    hp = diag.hparams(1.0, 1.0, 1.0)
    d, _, _ = diag.offpolicy_reference(pi, q, act, f, f, f, f, hp)
    assert d["rows_used"] == T * B and abs(d["kl_mu_pi"] - r["mean_kl"]) <= 1e-12 * max(1.0, r["mean_kl"])


def test_adapt_reference_branches():
    from freeimpala_amd import kl
    p = kl.params(kl_target=0.02)
    t, hi, lo = float(p.kl_target), float(p.band) * float(p.kl_target), float(p.kl_target) / float(p.band)
    s0 = dict(coeff=1.0, mean_kl=7.0, kl_sum=70.0, rows=10, updates=5, raised=1, lowered=2)
    up = kl.adapt_reference(s0, hi * 1.01, p, rows=20, kl_sum=20 * hi * 1.01)
    assert up == dict(coeff=2.0, mean_kl=hi * 1.01, kl_sum=20 * hi * 1.01, rows=20, updates=6, raised=2, lowered=2)
    down = kl.adapt_reference(s0, lo * 0.99, p)
    assert down == dict(s0, coeff=0.5, mean_kl=lo * 0.99, updates=6, lowered=3)
    for m in (t, hi, lo):  # the thresholds themselves hold: the comparisons are strict
        assert kl.adapt_reference(s0, m, p) == dict(s0, mean_kl=m, updates=6)
    assert s0 == dict(coeff=1.0, mean_kl=7.0, kl_sum=70.0, rows=10, updates=5, raised=1, lowered=2), "the input is not changed"
    # the clamps, still counted
    top, bottom = dict(s0, coeff=2.0 ** 20), dict(s0, coeff=2.0 ** -20)
    assert kl.adapt_reference(top, 1.0, p) == dict(top, mean_kl=1.0, updates=6, raised=2)
    assert kl.adapt_reference(bottom, 0.0, p) == dict(bottom, mean_kl=0.0, updates=6, lowered=3)
    assert kl.adapt_reference(dict(s0, coeff=3.0), 1.0, kl.params(coeff_max=4.0))["coeff"] == 4.0
    assert kl.adapt_reference(dict(s0, coeff=0.75), 0.0, kl.params(coeff_min=0.5))["coeff"] == 0.5
    # ten doublings and ten halvings of 1.0 stay exact inside the default bounds
    s = dict(s0)
    for _ in range(10):
        s = kl.adapt_reference(s, 1.0, p)
    assert s["coeff"] == 1024.0 and s["raised"] == 11
    for _ in range(20):
        s = kl.adapt_reference(s, 0.0, p)
    assert s["coeff"] == 2.0 ** -10 and s["lowered"] == 22
    # skipped: nothing but rows / kl_sum / mean_kl changes
    assert kl.adapt_reference(s0, 1.0, p, skipped=True, rows=30, kl_sum=30.0) == dict(s0, mean_kl=1.0, rows=30, kl_sum=30.0)
    # a NaN (or infinite) mean: no adaptation, but the update counts
    for m in (float("nan"), float("inf")):
        got = kl.adapt_reference(s0, m, p)
        assert got["coeff"] == 1.0 and (got["updates"], got["raised"], got["lowered"]) == (6, 1, 2)
        assert got["mean_kl"] == m or math.isnan(got["mean_kl"])
    # adapt = 0
    assert kl.adapt_reference(s0, 1.0, kl.params(adapt=False)) == dict(s0, mean_kl=1.0, updates=6)
    # a dict in the structure's place
    d = dict(adapt=True, kl_target=0.5, band=2.0, factor=4.0, coeff_min=0.1, coeff_max=10.0)
    assert kl.adapt_reference(s0, 1.5, d)["coeff"] == 4.0 and kl.adapt_reference(s0, 0.2, d)["coeff"] == 0.25


def test_near_threshold():
    from freeimpala_amd import kl
    p = kl.params(kl_target=0.25, band=2.0)  # thresholds 0.5 and 0.125
    for m, want in ((0.5, True), (0.5 * (1 + 0.9e-3), True), (0.5 * (1 - 0.9e-3), True), (0.5 * (1 + 2e-3), False),
                    (0.125, True), (0.125 * (1 - 0.9e-3), True), (0.125 * (1 - 2e-3), False), (0.25, False), (0.0, False),
                    (3.0, False)):
        assert kl.near_threshold(m, p) is want, m


def test_train_breakout_keeps_the_kl_runs_record_apart():
    """scripts/train_breakout.py without --out: a run with --kl-coeff writes its own file, whatever else is on; the
    Namespaces of tests/test_target_abi.py, which lack the new attributes, keep their names."""
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_breakout", os.path.join(ROOT, "scripts", "train_breakout.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)

    def out(**kw):
        a = dict(n_fresh=None, target_period=None, objective="vtrace", popart=None, diagnostics=0)
        a.update(kw)
        return tb.default_out(argparse.Namespace(**a), False, True)

    assert out(kl_coeff=1.0) == "train_breakout_kl.json"
    assert out(kl_coeff=1.0, objective="surrogate", n_fresh=128, target_period=4) == "train_breakout_kl.json"
    assert out(kl_coeff=0.0) == "train_breakout_kl.json", "a coefficient that starts at 0 is still a KL run"
    assert out(kl_coeff=None) == "train_breakout.json" and out() == "train_breakout.json"
    assert out(objective="surrogate") == "train_breakout_surrogate.json"
    assert out(objective="surrogate", n_fresh=128, target_period=4) == "train_breakout_target.json"
    assert out(n_fresh=128) == "train_breakout_target.json"
    assert out(popart=3e-4) == "train_breakout_popart.json" and out(diagnostics=5) == "train_breakout_diag.json"
    ap = tb.parser() if hasattr(tb, "parser") else None
    if ap is not None:
        a = ap.parse_args(["--kl-coeff", "1", "--kl-target", "0.02", "--kl-reference", "target", "--kl-fixed"])
        assert (a.kl_coeff, a.kl_target, a.kl_reference, a.kl_fixed) == (1.0, 0.02, "target", True)
