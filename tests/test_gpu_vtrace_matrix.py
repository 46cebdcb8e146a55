"""GPU: every instantiation, chunk edge, clip branch and input regime of csrc/vtrace.hip against
the fp64 reference tests/vtrace_cases.ref_numpy (itself proven against the oracle on these very
cases by tests/test_vtrace_reference.py, on the CPU).

Variants: 0 = what the learner step launches, 1 = vtrace_lds_kernel<A> (the production kernel),
2 = vtrace_column_kernel, 3 = vtrace_seq_kernel<A>, 4 = vtrace_stream_kernel<A>.

The bar. Unit-scale inputs (sections a to e, the first regimes of f) keep the project's bar
unchanged: |d| <= 1e-5 * max(1, |ref|) per element, 1e-5 relative on the loss sums (SURVEY.md 8(c),
BASELINE.json). That bar is relative to max(1, |output|), so it judges a kernel only where the
output's terms do not cancel far below their own size: the unit-scale inputs (vtrace_cases.unit_case)
are built so that they do not, and the CPU test asserts it from the reference (condition_numbers;
with rewards in {-1, 0, 1} and values ~ N(0, 1) the policy-loss sum of a few hundred rows lands
below 1 often enough that correct fp32 kernels miss 1e-5 of it by a factor of two to five).
The wide regimes of f with large logits cannot meet it in fp32 whatever the kernel does, so the
same 1e-5 is multiplied by a scale derived from the inputs alone (vtrace_cases.wide_scales):

* A log-probability is z_a - lse with |lse| up to max_i |z_i|. The correctly rounded fp32 lse is off
  by half an ulp of it, 2^-24 |lse| relative to 1, and so is everything computed from it: the ratio
  e^(lpa - lma) (relative error = absolute error of the exponent), rho, c, and through them acc,
  vs, pg_adv and dvalue; -pg_adv * lpa and the entropy (a difference of two numbers of size |z|).
  The unit-scale bar allows 1e-5 where |z| is of order 1, that is about 170 half-ulps; the same
  allowance at |z| = s is 1e-5 * s. So per row s = max(1, max_i |z_i|) over the pi and mu logits.
* dlogits_i = pg_adv (pi_i - [i = a]) + ec (...): an error dp in a probability (dp / p is again the
  error of a log-probability) comes out multiplied by pg_adv, and for the taken action pg_adv
  (pi_a - 1) cancels to the size of pg_adv * (1 - pi_a) with the error of pg_adv * pi_a left in it.
  So dlogits' scale is s * max(1, |pg_adv_ref|) of its row.
* A loss sum adds one term per row; its scale is the mean of its rows' scales.
* Rewards and values of 1e3 pass through no large logit: s is what randn logits give, about 3,
  and only dlogits, through max(1, |pg_adv_ref|), is judged much more widely than at unit scale.

The scale is fixed by this reasoning, not by what the kernels reach; scripts/vtrace_matrix_errors.py
records what they reach (profiles/vtrace_matrix_errors.json).
"""
import numpy as np
import pytest

import vtrace_cases as vc
from vtrace_cases import assert_bitwise, compare, run_vtrace, str_shape_ok

pytestmark = pytest.mark.gpu
_REFS = {}


def case_and_ref(case):
    """The inputs and the fp64 reference of a case, computed once and shared read-only."""
    if case not in _REFS:
        *inp, hp = vc.build(*case)
        ref = vc.ref_numpy(*inp, **hp)
        for a in list(inp) + [v for v in ref.values()]:
            a.setflags(write=False)
        _REFS[case] = (tuple(inp), hp, ref)
    return _REFS[case]


def check(case, variant, guard=True):
    inp, hp, ref = case_and_ref(case)
    out = run_vtrace(*inp, variant=variant, guard=guard, **hp)
    try:
        compare(out, ref)
    except AssertionError as e:
        raise AssertionError(f"variant {variant}, case {case}: {e}") from None
    return out


# ---- a. every instantiation of the production kernel, every chunk residue
@pytest.mark.parametrize("A", vc.EVEN_A)
def test_lds_kernel_every_T_to_70_and_the_dispatch_runs_it(A):
    """T = 1 .. 70 is 0, 1 and 2 whole chunks of 32 steps plus every residue twice (and the residues
    of 16-step chunks); B = 8 is one workgroup, B = 24 three. What the learner launches (variant 0)
    must be this kernel: bit-equal outputs."""
    for case in vc.cases_a(A):
        out = check(case, 1)
        inp, hp, _ = case_and_ref(case)
        assert_bitwise(run_vtrace(*inp, variant=0, guard=True, **hp), out, what=f"variant 0 vs 1, {case}")


@pytest.mark.parametrize("A", vc.EVEN_A)
def test_every_instantiation_on_returns_of_both_signs(A):
    """Rewards, deltas, acc and pg_adv of both signs through every instantiation of the three fast
    kernels (and the column kernel): the tensors at the unchanged bar. The loss sums of such inputs
    cancel and are judged in the other sections."""
    for case in vc.cases_mixed(A):
        inp, hp, ref = case_and_ref(case)
        for variant in (1, 2, 3, 4):
            out = run_vtrace(*inp, variant=variant, guard=True, **hp)
            try:
                vc.compare_tensors(out, ref)
            except AssertionError as e:
                raise AssertionError(f"variant {variant}, case {case}: {e}") from None
            assert np.isfinite(out["losses"]).all()


# ---- b. the on-request kernels, every instantiation
@pytest.mark.parametrize("A", vc.EVEN_A)
def test_seq_kernel_every_instantiation(A):
    for case in vc.cases_b(A, 3):
        check(case, 3)


@pytest.mark.parametrize("A", vc.EVEN_A)
def test_stream_kernel_every_instantiation(A):
    """The shapes str_shape_ok excludes are refused by the launcher, not run: their count per A is
    what the function gives for the list's (T, A), nothing more."""
    from freeimpala_amd._abi import FiError
    cases = vc.cases_b(A, 4)
    dropped = 0
    for case in cases:
        if str_shape_ok(case[2], A):
            check(case, 4)
        else:
            dropped += 1
            inp, hp, _ = case_and_ref(case)
            with pytest.raises(FiError, match=r"streaming kernel needs B%4==0, even A<=20, T\*A<=2048"):
                run_vtrace(*inp, variant=4, **hp)
    assert dropped == sum(not str_shape_ok(T, A) for T in vc.B_TS) * 2
    assert dropped < len(cases)


# ---- c. the column kernel and the dispatch
@pytest.mark.parametrize("A", vc.C_AS)
def test_column_kernel_any_A_any_B(A):
    for case in vc.cases_c(A):
        out = check(case, 2)
        B = case[3]
        inp, hp, _ = case_and_ref(case)
        if A == 1:  # one action: pi = 1, log pi = 0; no gradient, no entropy, no policy loss
            assert not out["dlogits"].any() and out["losses"][2] == 0 and out["losses"][0] == 0
        if A % 2 == 1 or B % 8 != 0 or A > 20:
            assert_bitwise(run_vtrace(*inp, variant=0, guard=True, **hp), out, what=f"variant 0 vs 2, {case}")
        nul = run_vtrace(*inp, variant=2, guard=True, null_targets=True, **hp)
        assert_bitwise(nul, out, keys=("dlogits", "dvalue", "losses"), what=f"NULL vs, adv, {case}")


def test_A1_reference_has_no_policy_gradient():
    for case in vc.cases_c(1):
        _, _, ref = case_and_ref(case)
        assert not ref["dlogits"].any() and ref["losses"][2] == 0 and ref["losses"][0] == 0


@pytest.mark.parametrize("variant,kernel", [(1, "LDS kernel"), (3, "sequence kernel"), (4, "streaming kernel")])
def test_fast_variants_refuse_what_they_cannot_run(variant, kernel):
    from freeimpala_amd._abi import FiError
    good = vc.rand_case(1, 4, 8, 6)

    def refused(match, case=good, **kw):
        with pytest.raises(FiError, match=match):
            run_vtrace(*case, variant=variant, **kw)

    refused(f"{kernel} writes vs and pg_adv", null_targets=True)
    refused(f"{kernel} needs 16-byte aligned" if variant != 3 else "needs 16-byte aligned logits",
            logits_byte_shift=4)
    refused("workspace too small", ws_short=1)
    shape = {1: "LDS kernel needs B%8==0, even A<=20", 3: "sequence kernel needs T<=128, B%8==0, even A<=20",
             4: "streaming kernel needs B%4==0, even A<=20"}[variant]
    refused(shape, case=vc.rand_case(2, 4, 6 if variant == 4 else 12, 6))
    refused(shape, case=vc.rand_case(3, 4, 8, 22))
    compare(run_vtrace(*good, variant=variant), vc.ref_numpy(*good))  # and the shape itself runs


# ---- d. persistent grids and the finalize kernel
def test_persistent_grids_and_finalize_around_their_edges():
    """More column groups than workgroups with a ragged last round (variants 3 and 4), and the
    finalize kernel's 256 threads over nblk = 1, 2, 255, 256, 257, 513 partials; variant 4 also at
    sequences of fewer DMA pieces than waves (T * A <= 64) on workgroups that walk three groups."""
    cus = vc.device_cu_count()
    for variant, case in vc.cases_d(cus):
        check(case, variant)


# ---- e. hyper-parameter branches
@pytest.mark.parametrize("hpset", list(vc.HP_SETS))
def test_hyper_parameter_branches(hpset):
    for case in vc.cases_e():
        if case[0] == "hp:" + hpset:
            for variant in (1, 2, 3, 4):
                check(case, variant)


# ---- f. input regimes
@pytest.mark.parametrize("regime", vc.UNIT_REGIMES)
def test_unit_scale_regimes(regime):
    for case in vc.cases_f((regime,)):
        for variant in (1, 2, 3, 4):
            check(case, variant)


@pytest.mark.parametrize("regime", vc.WIDE_REGIMES)
def test_wide_regimes_at_the_derived_bar(regime):
    """Every output finite and within 1e-5 times the scale derived in the module docstring."""
    for case in vc.cases_f((regime,)):
        inp, hp, ref = case_and_ref(case)
        scales = vc.wide_scales(inp[0], inp[1], ref)
        for variant in (1, 2, 3, 4):
            out = run_vtrace(*inp, variant=variant, guard=True, **hp)
            errs = vc.scaled_errors(out, ref, scales)
            print(f"{regime} {case[2:]} variant {variant}: worst error in bars {errs}")
            assert max(errs.values()) <= 1.0, (regime, case, variant, errs)
