"""CPU-side checks of PopArt's ABI (include/fi_popart.h): the in-tree libfi_learner.so exports exactly the
functions the header declares, freeimpala_amd.popart binds exactly that set, none of it is in an older
header or table, fi_popart_state has one layout in C and in ctypes, popart_reference -- the host form of
the rule -- on hand-computed cases, the preserved output in fp64, and the moments plan."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h", "fi_train.h", "fi_breakout.h", "fi_publish.h", "fi_explore.h", "fi_diag.h")
FUNCTIONS = ("fi_popart_enable", "fi_popart_get_state", "fi_popart_set_state", "fi_popart_state_dev", "fi_popart_plan",
             "fi_popart_workspace_bytes", "fi_popart_denormalize", "fi_popart_scale_grad", "fi_popart_update")
FIELDS = ["enabled", "reserved", "beta", "sigma_min", "sigma_max", "mu", "nu", "sigma", "updates"]


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_popart_header():
    from freeimpala_amd import (_abi, actor, breakout, diag, env, explore, farmer, gather, popart, prio, publish, ring,
                                rollout, train, weights)
    lib = popart.lib()
    names = header_functions("fi_popart.h")
    assert names == sorted(FUNCTIONS)
    assert all(n.startswith("fi_popart_") for n in names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(popart.SIGNATURES), set(names) ^ set(popart.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_popart_")} == set(names)
    # a header of its own: no older header and no older table gains a function
    assert len(OTHER_HEADERS) == 14 and all(os.path.exists(os.path.join(ROOT, "include", h)) for h in OTHER_HEADERS)
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for mod in (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout, publish, explore, diag):
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(train.SIGNATURES) == 8 and len(diag.SIGNATURES) == 6
    assert lib.fi_abi_version() == 1


def test_popart_state_layout_matches_c(tmp_path):
    from freeimpala_amd import popart
    assert [f for f, _ in popart.PopartState._fields_] == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_popart.h"\nint main(){'
           'printf("%zu", sizeof(fi_popart_state));' +
           "".join(f'printf(" %zu", offsetof(fi_popart_state, {f}));' for f in FIELDS) +
           'printf(" %.17g %.17g %.17g", FI_POPART_BETA, FI_POPART_SIGMA_MIN, FI_POPART_SIGMA_MAX);}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    got = [int(v) for v in out[:-3]]
    assert got == [ctypes.sizeof(popart.PopartState)] + [getattr(popart.PopartState, f).offset for f in FIELDS]
    assert got == [64, 0, 4] + list(range(8, 64, 8))
    assert [float(v) for v in out[-3:]] == [popart.BETA, popart.SIGMA_MIN, popart.SIGMA_MAX] == [3e-4, 1e-4, 1e6]
    d = popart.PopartState(1, 0, 0.25, 0.5, 2.0, 3.0, 15.25, 2.5, 7).as_dict()
    assert d == dict(enabled=True, beta=0.25, sigma_min=0.5, sigma_max=2.0, mu=3.0, nu=15.25, sigma=2.5, updates=7)
    raw = popart.pack_state(3.0, 15.25, 2.5, 7)
    assert raw.nbytes == popart.STATE_BYTES == 32
    assert popart.unpack_state(raw) == dict(mu=3.0, nu=15.25, sigma=2.5, updates=7)


def test_popart_reference_by_hand():
    from freeimpala_amd.popart import popart_reference, sigma_of
    w, b = np.array([0.5, -2.0, 0.125]), 0.75
    n = np.array([[1.0, -1.0], [0.0, 2.0]])
    # beta = 0: everything comes back unchanged, and the values are sigma n + mu
    r = popart_reference(n, [1.0, 3.0], w, b, 3.0, 15.25, beta=0.0)
    assert (r["mu"], r["nu"], r["sigma"], r["b"], r["updated"]) == (3.0, 15.25, 2.5, 0.75, True)
    np.testing.assert_array_equal(r["w"], w)
    np.testing.assert_array_equal(r["values"], np.array([[5.5, 0.5], [3.0, 8.0]]))
    # beta = 1 with vs = {1, 3}: mu' = 2, nu' = 5, sigma' = 1; from mu = 0, sigma = 1: w' = w, b' = b - 2
    r = popart_reference(n, [1.0, 3.0], w, b, 0.0, 1.0, beta=1.0)
    assert (r["mu"], r["nu"], r["sigma"]) == (2.0, 5.0, 1.0)
    np.testing.assert_array_equal(r["w"], w)
    assert r["b"] == -1.25
    # the same targets from sigma = 2.5, mu = 3: w' = 2.5 w, b' = 2.5 b + 3 - 2
    r = popart_reference(n, np.array([[1.0], [3.0]]), w, b, 3.0, 15.25, beta=1.0)
    assert (r["mu"], r["nu"], r["sigma"]) == (2.0, 5.0, 1.0)
    np.testing.assert_array_equal(r["w"], 2.5 * w)
    assert r["b"] == 2.5 * 0.75 + 1.0
    # a target set with zero variance hits sigma_min, and sigma_max bounds the other side
    r = popart_reference(n, [4.0, 4.0, 4.0], w, b, 0.0, 1.0, beta=1.0, sigma_min=1e-4)
    assert (r["mu"], r["nu"], r["sigma"]) == (4.0, 16.0, 1e-4)
    np.testing.assert_array_equal(r["w"], w * 1.0 / 1e-4)
    r = popart_reference(n, [-10.0, 10.0], w, b, 0.0, 1.0, beta=1.0, sigma_max=4.0)
    assert (r["mu"], r["nu"], r["sigma"]) == (0.0, 100.0, 4.0)
    # a partial step: mu' = 0.75 * 3 + 0.25 * 2, nu' = 0.75 * 15.25 + 0.25 * 5
    r = popart_reference(n, [1.0, 3.0], w, b, 3.0, 15.25, beta=0.25)
    assert (r["mu"], r["nu"]) == (2.75, 12.6875) and r["sigma"] == math.sqrt(12.6875 - 2.75 ** 2)
    # a non-finite target: nothing moves
    for bad in (np.nan, np.inf):
        r = popart_reference(n, [1.0, bad], w, b, 3.0, 15.25, beta=0.5)
        assert (r["mu"], r["nu"], r["sigma"], r["b"], r["updated"]) == (3.0, 15.25, 2.5, 0.75, False)
        np.testing.assert_array_equal(r["w"], w)
    assert sigma_of(0.0, 0.0) == 1e-4 and sigma_of(1.0, 0.5) == 1e-4 and sigma_of(0.0, 1e13) == 1e6


def test_update_preserves_the_unnormalised_output_in_fp64():
    """sigma' (w' . h + b') + mu' against sigma (w . h + b) + mu for random w, b, h and statistics that move
    by orders of magnitude: 1e-12 relative to sum_j |sigma w_j h_j| + |sigma b| + |mu| + |mu'|, the size of the terms
    the two sides add up (H = 64 terms, a few 2^-53 each)."""
    from freeimpala_amd.popart import popart_reference, preserved_output
    rs = np.random.RandomState(7)
    worst = 0.0
    for case in range(24):
        H = 64
        w, b, h = rs.standard_normal(H), rs.standard_normal(), np.abs(rs.standard_normal((33, H)))
        mu, sd = rs.uniform(-50, 50), 10.0 ** rs.uniform(-3, 3)
        nu = sd * sd + mu * mu
        vs = rs.standard_normal(101) * 10.0 ** rs.uniform(-2, 3) + rs.uniform(-100, 100)
        r = popart_reference(np.zeros(1), vs, w, b, mu, nu, beta=rs.choice([3e-4, 0.25, 1.0]), sigma=sd)
        assert r["updated"] and (r["mu"] != mu or r["sigma"] != sd)
        before = preserved_output(h, w, b, mu, sd)
        after = preserved_output(h, r["w"], r["b"], r["mu"], r["sigma"])
        scale = np.abs(sd * h * w).sum(axis=1) + abs(sd * b) + abs(mu) + abs(r["mu"])
        worst = max(worst, float((np.abs(after - before) / scale).max()))
    print(f"preserve, fp64: worst relative error {worst:.3e} (bar 1e-12)")
    assert worst <= 1e-12


def test_plan_and_workspace_need_no_device():
    from freeimpala_amd import popart
    assert popart.plan(0) == 0 and popart.workspace_bytes(0) == 0
    assert popart.plan(1) == 1 and popart.workspace_bytes(1) == 16
    assert popart.plan(409600) == 200, "T = 100, B = 4096: 2,048 targets per workgroup"
    last = 0
    for n in (1, 2, 3, 5, 255, 257, 1027, 2047, 2048, 2049, 4097, 10 ** 5 + 1, 409600, 409601, 2 ** 19 - 1, 2 ** 19 + 1,
              10 ** 7 + 3, 2 ** 31 + 5):
        g = popart.plan(n)
        assert 1 <= g <= 256 and g >= last, (n, g)
        assert g == min(256, -(-n // 2048))
        assert popart.workspace_bytes(n) == 16 * g
        last = g
