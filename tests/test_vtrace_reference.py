"""CPU: the two V-trace references against each other, and the builders' conditions.

tests/vtrace_cases.ref_numpy (float64 numpy) judges the kernels in tests/test_gpu_vtrace_matrix.py.
Before it does, it has to agree with oracle/impala_oracle.c, written independently, on every case
of that matrix: the loss sums (fp64 in both) to 1e-12 * max(1, |x|), and the tensors, which the
oracle returns rounded to fp32, to the same bound after the same rounding. Each builder's promise
(a clip that binds for about half the rows, a clip that never binds, ratios past both ends of
fp32) is asserted here from the reference alone, so the GPU tests skip nothing.
"""
import itertools

import numpy as np
import pytest

import vtrace_cases as vc

SECTIONS = vc.all_cases()
AGREE = 1e-12


def _agree(x, y, what):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    err = np.abs(x - y) / np.maximum(1.0, np.abs(y))
    assert err.max() <= AGREE, f"{what}: {err.max():.3e}"


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_ref_numpy_agrees_with_the_oracle(orc, section):
    for name, seed, T, B, A in SECTIONS[section]:
        *case, hp = vc.build(name, seed, T, B, A)
        ref = vc.ref_numpy(*case, **hp)
        o = orc.vtrace_loss(*case, **hp)
        what = f"{name} seed={seed} T={T} B={B} A={A}"
        for k in ("vs", "pg_adv", "dlogits", "dvalue"):
            assert np.isfinite(ref[k]).all(), (what, k)
            _agree(ref[k].astype(np.float32), o[k], f"{what} {k}")
        assert np.isfinite(ref["losses"]).all(), what
        _agree(ref["losses"], o["losses"], f"{what} losses")


def _share(name, T, B, A, key):
    seed = next(c[1] for c in vc.cases_e() + vc.cases_f() if c[0] == name and c[2:] == (T, B, A))
    *case, hp = vc.build(name, seed, T, B, A)
    ref = vc.ref_numpy(*case, **hp)
    return float((ref["log_rho"] > np.log(hp[key])).mean()), case, hp, ref


@pytest.mark.parametrize("T,B,A", vc.EF_SHAPES)
@pytest.mark.parametrize("clip", vc.CLIPS)
def test_clip_sets_bind_as_promised(clip, T, B, A):
    """A half-clipping bar binds on 10 % to 90 % of the (t, b); a bar of 1e9 never binds."""
    half, *_ = _share(f"hp:{clip}_half", T, B, A, clip)
    never, *_ = _share(f"hp:{clip}_never", T, B, A, clip)
    print(f"\n{clip} T={T} B={B} A={A}: binds on {half:.3f} of the rows at {vc.HALF}, {never:.3f} at {vc.NEVER:g}")
    assert 0.10 <= half <= 0.90
    assert never == 0.0


@pytest.mark.parametrize("T,B,A", vc.EF_SHAPES)
@pytest.mark.parametrize("name", [n for n in vc.HP_SETS if n.endswith(("_half", "_never"))])
def test_exchanging_two_clips_moves_the_reference_past_the_bar(name, T, B, A):
    """The three bars of a clip set are distinct enough that a kernel reading one where another
    belongs misses the 1e-5 bar: each exchange moves some output by more than it."""
    _, case, hp, ref = _share("hp:" + name, T, B, A, "rho_bar")
    for x, y in itertools.combinations(vc.CLIPS, 2):
        sw = dict(hp)
        sw[x], sw[y] = hp[y], hp[x]
        other = vc.ref_numpy(*case, **sw)
        moved = max(float((np.abs(other[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
                    for k in ("vs", "pg_adv", "dlogits", "dvalue", "losses"))
        print(f"\n{name} T={T} A={A}: {x} <-> {y} moves the reference by {moved:.3e}")
        assert moved > 100 * vc.TOL, (x, y, moved)


@pytest.mark.parametrize("T,B,A", vc.EF_SHAPES)
def test_saturated_regime_leaves_fp32_on_both_sides(T, B, A):
    """At least 5 % of the ratios pi(a)/mu(a) exceed FLT_MAX and 5 % fall below FLT_MIN (float64)."""
    _, _, _, ref = _share("saturated", T, B, A, "rho_bar")
    over = float((ref["log_rho"] > np.log(vc.FLT_MAX)).mean())
    under = float((ref["log_rho"] < np.log(vc.FLT_MIN)).mean())
    print(f"\nsaturated T={T} B={B} A={A}: {over:.3f} of the ratios above FLT_MAX, {under:.3f} below FLT_MIN")
    assert over >= 0.05 and under >= 0.05


@pytest.mark.parametrize("T,B,A", vc.EF_SHAPES)
def test_regime_builders_build_what_they_name(T, B, A):
    seeds = {c[0]: c[1] for c in vc.cases_f() if c[2:] == (T, B, A)}
    b = {n: vc.build(n, seeds[n], T, B, A) for n in seeds}
    assert (b["disc_zero"][4] == 0).all() and (b["disc_one_long_memory"][4] == 1).all()
    z = np.flatnonzero((b["disc_zero_at_edges"][4] == 0).all(axis=1))
    assert z.tolist() == sorted({t for t in (0, 31, 32, T - 1) if t < T})
    assert (b["disc_zero_at_edges"][4][np.setdiff1d(np.arange(T), z)] != 0).all()
    assert b["pi_equals_mu"][0].tobytes() == b["pi_equals_mu"][1].tobytes()
    assert np.ptp(b["equal_logits"][0]) == 0 and np.ptp(b["equal_logits"][1]) == 0
    assert (b["actions_first"][2] == 0).all() and (b["actions_last"][2] == A - 1).all()
    assert (b["rewards_zero"][3] == 0).all()
    pi, mu, act = b["action_80_below_max"][:3]
    for zz in (pi, mu):
        za = np.take_along_axis(zz, act[..., None].astype(np.int64), -1)[..., 0]
        assert np.allclose(zz.max(-1) - za, 80.0, atol=1e-4)
    base = vc.unit_case(seeds["offset_plus_100"], T, B, A)
    assert np.allclose(b["offset_plus_100"][0] - base[0], 100.0) and np.allclose(b["offset_minus_100"][1] - vc.unit_case(seeds["offset_minus_100"], T, B, A)[1], -100.0)
    assert np.abs(b["returns_1e3"][3]).max() == 2e3 and np.abs(b["returns_1e3"][5]).max() > 300
    r = vc.ref_numpy(*b["disc_one_long_memory"][:6], **b["disc_one_long_memory"][6])
    assert (r["log_rho"] < np.log(vc.NEVER)).all()


UNIT_SECTIONS = sorted(k for k in SECTIONS if not k.startswith("m-"))


@pytest.mark.parametrize("section", UNIT_SECTIONS)
def test_unit_scale_cases_are_well_conditioned(section):
    """vtrace_cases.condition_numbers: in every case held to the unchanged 1e-5 bar, no output's
    terms exceed COND_MAX times the bar's measure max(1, |output|), so the bar judges the kernel
    and not a cancellation in the inputs."""
    worst = {}
    for case in SECTIONS[section]:
        if case[0] in vc.WIDE_REGIMES or case[0] == "mixed_sign":
            continue
        *inp, hp = vc.build(*case)
        for k, v in vc.condition_numbers(*inp, **hp).items():
            if v > worst.get(k, (0.0,))[0]:
                worst[k] = (v, case)
    print(f"\n{section}: worst condition numbers " + ", ".join(f"{k} {v[0]:.2f}" for k, v in worst.items()))
    for k, (v, case) in worst.items():
        assert v <= vc.COND_MAX, (k, v, case)


@pytest.mark.parametrize("A", vc.EVEN_A)
def test_mixed_sign_cases_have_both_signs_and_well_conditioned_tensors(A):
    """The mixed-sign cases are compared on the tensors only: those must be well conditioned, and
    deltas, pg_adv and rewards must take both signs on a fair share of the rows."""
    for case in vc.cases_mixed(A):
        *inp, hp = vc.build(*case)
        ref = vc.ref_numpy(*inp, **hp)
        cn = vc.condition_numbers(*inp, **hp)
        neg = float((ref["pg_adv"] < 0).mean())
        print(f"\n{case[2:]}: pg_adv < 0 on {neg:.3f} of the rows, condition numbers "
              + ", ".join(f"{k} {v:.2f}" for k, v in cn.items()))
        assert 0.25 <= neg <= 0.75 and (inp[3] < 0).any() and ((ref["vs"] - inp[5][:-1]) < 0).mean() >= 0.25
        for k in ("vs", "pg_adv", "dlogits"):
            assert cn[k] <= vc.COND_MAX, (k, cn[k], case)
