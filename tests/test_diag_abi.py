"""CPU-side checks of the off-policy diagnostics' ABI (include/fi_diag.h): the in-tree libfi_learner.so
exports exactly the functions the header declares, freeimpala_amd.diag binds exactly that set, none of
it is in an older header or table, fi_offpolicy_diag has one layout in C and in ctypes, and
offpolicy_reference -- the host form of the rule -- on hand-computed cases."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h", "fi_train.h", "fi_breakout.h", "fi_publish.h", "fi_explore.h")
FUNCTIONS = ("fi_diag_workspace_bytes", "fi_diag_plan", "fi_diag_offpolicy", "fi_diag_enqueue", "fi_diag_read",
             "fi_diag_learner")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_diag_header():
    from freeimpala_amd import (_abi, actor, breakout, diag, env, explore, farmer, gather, prio, publish, ring, rollout,
                                train, weights)
    lib = diag.lib()
    names = header_functions("fi_diag.h")
    assert names == sorted(FUNCTIONS)
    assert all(n.startswith("fi_diag_") for n in names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(diag.SIGNATURES), set(names) ^ set(diag.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_diag_")} == set(names)
    # a header of its own: no older header and no older table gains a function
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for mod in (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish, explore):
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(publish.SIGNATURES) == 8 and len(explore.SIGNATURES) == 6
    assert lib.fi_abi_version() == 1


def test_offpolicy_diag_layout_matches_c(tmp_path):
    from freeimpala_amd import diag
    fields = [f for f, _ in diag.OffPolicyDiag._fields_]
    assert fields == ["struct_size", "reserved"] + list(diag.COUNTS) + list(diag.DOUBLES)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_diag.h"\nint main(){'
           'printf("%zu", sizeof(fi_offpolicy_diag));' +
           "".join(f'printf(" %zu", offsetof(fi_offpolicy_diag, {f}));' for f in fields) + "}")
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(diag.OffPolicyDiag)] + [getattr(diag.OffPolicyDiag, f).offset for f in fields]
    assert got[0] == 160
    assert diag.OffPolicyDiag.rows.offset == 8 and diag.OffPolicyDiag.mean_log_rho.offset == 72
    assert diag.OffPolicyDiag.explained_variance.offset == 152


def test_plan_and_workspace_need_no_device():
    from freeimpala_amd import diag
    from freeimpala_amd._abi import FiError
    ct, ts = diag.plan(100, 4096, 18)
    assert ct == 64 and ct * ts >= 256, "the slices of T fill the chip's 256 CUs at B = 4096"
    assert diag.plan(1, 1, 3) == (1, 1) and diag.plan(33, 72, 18)[0] == 2
    assert diag.workspace_bytes(100, 4096, 18) > 0 and diag.workspace_bytes(5, 24, 18) % 8 == 0
    for bad in ((0, 8, 4), (4, 0, 4), (4, 8, 1), (4, 8, 65), (1 << 15, 1 << 14, 4)):
        assert diag.workspace_bytes(*bad) == 0, bad
        try:
            diag.plan(*bad)
        except FiError as e:
            assert "rc=-1" in str(e)
        else:
            raise AssertionError(bad)


def _hp(r=1.0, c=1.0, p=1.0):
    from freeimpala_amd import diag
    return diag.hparams(r, c, p)


def test_reference_single_row_by_hand():
    """T = B = 1, A = 2: pi = softmax(0, ln 3) = (1/4, 3/4), mu = (1/2, 1/2), action 1."""
    from freeimpala_amd.diag import offpolicy_reference
    pi = np.array([[[0.0, np.float32(math.log(3.0))]]], np.float32)
    mu = np.zeros((1, 1, 2), np.float32)
    one = np.ones((1, 1), np.float32)
    d, ckl, clr = offpolicy_reference(pi, mu, np.array([[1]], np.int32), 2 * one, 0 * one, 3 * one, 5 * one, _hp(1.0, 1.6, 1.5))
    assert d["rows"] == d["rows_used"] == 1 and d["rows_bad_action"] == d["rows_nonfinite"] == 0
    np.testing.assert_allclose(d["mean_rho"], 1.5, rtol=1e-7)   # the fp32 ln 3 is 2e-8 away from ln 3
    np.testing.assert_allclose(d["max_rho"], 1.5, rtol=1e-7)
    np.testing.assert_allclose(d["min_rho"], 1.5, rtol=1e-7)
    np.testing.assert_allclose(d["mean_log_rho"], math.log(1.5), rtol=1e-7)
    np.testing.assert_allclose(d["kl_mu_pi"], 0.5 * math.log(4.0 / 3.0), rtol=1e-7)
    np.testing.assert_allclose(d["entropy_mu"], math.log(2.0), rtol=1e-12)
    np.testing.assert_allclose(d["entropy_pi"], -(0.25 * math.log(0.25) + 0.75 * math.log(0.75)), rtol=1e-7)
    assert d["ess"] == 1.0
    assert d["mean_abs_td"] == 2.0 and d["mean_reward"] == 2.0 and d["n_episode_ends"] == 1
    # 1.5 > rho_bar = 1.0 and not > c_bar = 1.6 (rho is a hair off 1.5, so the third bar proves nothing here)
    assert (d["n_rho_clipped"], d["n_c_clipped"]) == (1, 0)
    assert math.isnan(d["explained_variance"]), "one row: Var(vs) = 0"
    np.testing.assert_allclose(ckl, [d["kl_mu_pi"]], rtol=0, atol=0)
    np.testing.assert_allclose(clr, [d["mean_log_rho"]], rtol=0, atol=0)


def _random_case(T=6, B=5, A=7, seed=0):
    rs = np.random.RandomState(seed)
    pi = (3 * rs.standard_normal((T, B, A))).astype(np.float32)
    mu = (pi + rs.standard_normal((T, B, A))).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew, val, vs = (rs.standard_normal((T, B)).astype(np.float32) for _ in range(3))
    disc = np.where(rs.rand(T, B) < 0.1, 0.0, 0.99).astype(np.float32)
    return pi, mu, act, rew, disc, val, vs


def test_reference_on_policy_is_exact():
    from freeimpala_amd.diag import offpolicy_reference
    pi, _, act, rew, disc, val, vs = _random_case()
    d, ckl, clr = offpolicy_reference(pi, pi.copy(), act, rew, disc, val, vs, _hp())
    assert d["mean_log_rho"] == 0.0 and d["kl_mu_pi"] == 0.0
    assert d["n_rho_clipped"] == d["n_c_clipped"] == d["n_pg_clipped"] == 0, "strict tests at the default bars"
    assert d["mean_rho"] == d["max_rho"] == d["min_rho"] == d["ess"] == 1.0
    assert d["entropy_pi"] == d["entropy_mu"] > 0
    assert (ckl == 0).all() and (clr == 0).all()
    assert d["n_episode_ends"] == int((disc == 0).sum())
    assert 0 < abs(d["explained_variance"]) < 10


def test_reference_skip_order_and_all_skipped_column():
    from freeimpala_amd.diag import offpolicy_reference
    pi, mu, act, rew, disc, val, vs = _random_case()
    T, B, A = pi.shape
    act[0, 0], act[1, 1] = -1, A          # bad actions
    pi[2, 2, 3] = np.nan                  # non-finite rows
    mu[3, 3, 0] = np.inf
    pi[0, 0, 1] = np.nan                  # a bad action AND a NaN: counted as a bad action, first in the order
    act[:, 4] = A + 3                     # one whole column bad
    d, ckl, clr = offpolicy_reference(pi, mu, act, rew, disc, val, vs, _hp(1.3, 0.9, 2.1))
    assert d["rows"] == T * B and d["rows_bad_action"] == 2 + T and d["rows_nonfinite"] == 2
    assert d["rows_used"] == T * B - 4 - T
    assert np.isnan(ckl[4]) and np.isnan(clr[4]) and np.isfinite(ckl[:4]).all() and np.isfinite(clr[:4]).all()
    assert all(math.isfinite(d[k]) for k in ("mean_log_rho", "mean_rho", "kl_mu_pi", "entropy_pi", "entropy_mu", "max_rho",
                                              "min_rho", "ess", "explained_variance", "mean_abs_td", "mean_reward"))
    assert d["n_episode_ends"] == int((disc == 0).sum()), "over all rows, skipped ones included"
    # the sums are those of the batch without the skipped rows: drop them by hand and compare
    keep = np.ones((T, B), bool)
    keep[0, 0] = keep[1, 1] = keep[2, 2] = keep[3, 3] = False
    keep[:, 4] = False
    rows = lambda x: x[keep][None]  # noqa: E731  (1, n_used[, A]): one time step, the used rows as columns
    d2, _, _ = offpolicy_reference(rows(pi), rows(mu), rows(act), rows(rew), rows(disc), rows(val), rows(vs),
                                   _hp(1.3, 0.9, 2.1))
    for k in ("mean_log_rho", "mean_rho", "kl_mu_pi", "entropy_pi", "entropy_mu", "mean_abs_td", "mean_reward", "ess",
              "explained_variance"):
        np.testing.assert_allclose(d[k], d2[k], rtol=1e-12, err_msg=k)
    for k in ("rows_used", "n_rho_clipped", "n_c_clipped", "n_pg_clipped", "max_rho", "min_rho"):
        assert d[k] == d2[k], k
    # everything skipped: every double is NaN
    act[:] = -5
    d3, ckl3, _ = offpolicy_reference(pi, mu, act, rew, disc, val, vs, _hp())
    assert d3["rows_used"] == 0 and d3["rows_bad_action"] == T * B and d3["rows_nonfinite"] == 0
    from freeimpala_amd.diag import DOUBLES
    assert all(math.isnan(d3[k]) for k in DOUBLES) and np.isnan(ckl3).all()


def test_reference_constant_vs_has_no_explained_variance():
    from freeimpala_amd.diag import offpolicy_reference
    pi, mu, act, rew, disc, val, vs = _random_case()
    vs[:] = 0.7
    d, _, _ = offpolicy_reference(pi, mu, act, rew, disc, val, vs, _hp())
    assert math.isnan(d["explained_variance"]) and math.isfinite(d["mean_abs_td"]) and 0 < d["ess"] <= 1
    # values may come with the bootstrap row: only the first T rows count
    val1 = np.concatenate([val, 100 * np.ones((1, val.shape[1]), np.float32)])
    d1, _, _ = offpolicy_reference(pi, mu, act, rew, disc, val1, vs, _hp())
    assert d1["mean_abs_td"] == d["mean_abs_td"]
