"""GPU parity: the fused V-trace + loss + gradient kernels vs the CPU oracle.

Bar (BASELINE.json north_star): vs, pg_adv, dlogits, dvalue elementwise
|d| <= 1e-5 * max(1, |ref|); loss scalars relative 1e-5 (fp32 kernels vs fp64 oracle).
"""
import glob
import os

import numpy as np
import pytest

from vtrace_cases import HP_KEYS, TOL, _close, compare, rand_case, run_vtrace, str_shape_ok  # noqa: F401 (re-exported)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "vtrace_*.npz"))))
def test_vtrace_golden(path):
    z = np.load(path)
    hp = dict(zip(HP_KEYS, z["hp"].tolist()))
    out = run_vtrace(z["pi"], z["mu"], z["actions"], z["rewards"], z["discounts"], z["values"], **hp)
    compare(out, {k: z[k] for k in ("vs", "pg_adv", "dlogits", "dvalue", "losses")})


@pytest.mark.parametrize("T,B,A", [(1, 16, 18), (16, 16, 18), (17, 32, 18), (33, 48, 4),
                                   (100, 64, 2), (100, 32, 20), (50, 16, 6), (3, 16, 18),
                                   (100, 256, 18), (128, 64, 18), (127, 16, 18), (65, 24, 18)])
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_vtrace_kernels_vs_oracle(orc, T, B, A, variant):
    if variant == 4 and not str_shape_ok(T, A):
        pytest.skip("the streaming kernel holds a group's whole sequence in LDS and stores at most "
                    "2,048 dlogits pieces (vtrace.hip str_supported; vtrace_cases.str_shape_ok)")
    case = rand_case(T * 1000 + B + A, T, B, A)
    ref = orc.vtrace_loss(*case)
    out = run_vtrace(*case, variant=variant)
    compare(out, ref)


@pytest.mark.parametrize("T,A", [(113, 18), (120, 18), (102, 20), (110, 20)])
def test_vtrace_streaming_kernel_edge_of_its_store_rounds(orc, T, A):
    """variant 4 stores the dlogits tile in 4 rounds of 512 pieces, i.e. at most 2,048
    = T * A pieces. At the edge (T * A <= 2048) it must match the oracle; past it (the LDS would
    still fit) it must refuse loudly instead of leaving the rows past the last round unwritten."""
    from freeimpala_amd._abi import FiError
    case = rand_case(T * 31 + A, T, 8, A)
    if T * A <= 2048:
        compare(run_vtrace(*case, variant=4), orc.vtrace_loss(*case))
    else:
        with pytest.raises(FiError, match="T\\*A<=2048"):
            run_vtrace(*case, variant=4)


@pytest.mark.parametrize("T,B,A", [(7, 13, 18), (5, 40, 5), (100, 100, 33)])
def test_vtrace_ragged_shapes_use_column_kernel(orc, T, B, A):
    case = rand_case(7 + T + B + A, T, B, A)
    compare(run_vtrace(*case), orc.vtrace_loss(*case))


def test_vtrace_adversarial_clipping(orc):
    case = rand_case(99, 64, 32, 18, scale=8.0, done_p=0.2)
    hp = dict(rho_bar=0.7, c_bar=0.5, pg_rho_bar=1.3, lambda_=0.9, baseline_cost=0.3,
              entropy_cost=0.05)
    ref = orc.vtrace_loss(*case, **hp)
    for v in (1, 2, 3, 4):
        compare(run_vtrace(*case, variant=v, **hp), ref)


@pytest.mark.parametrize("variant", [1, 3, 4])
def test_vtrace_full_size_T100_B4096(orc, variant):
    """BASELINE config size (T=100, B=4096, A=18): full elementwise parity with the oracle
    plus the size-independent property sum(pg_adv-weighted) via the loss scalars; the chunked
    kernel (1), the whole-sequence kernel (3) and the streaming kernel (4)."""
    case = rand_case(4096, 100, 4096, 18)
    ref = orc.vtrace_loss(*case)
    out = run_vtrace(*case, variant=variant)
    compare(out, ref)


def test_vtrace_variants_agree_bitwise_on_losses_order_free_fields(orc):
    """Both kernels compute the same per-element quantities; the scan association differs, so
    compare them to each other at the same 1e-5 bar (and the bootstrap dvalue row is 0)."""
    case = rand_case(5, 40, 64, 18)
    a = run_vtrace(*case, variant=1)
    b = run_vtrace(*case, variant=2)
    c = run_vtrace(*case, variant=3)
    d = run_vtrace(*case, variant=4)
    compare(a, b)
    compare(c, a)
    compare(d, a)
    for o in (a, b, c, d):
        assert np.all(o["dvalue"][-1] == 0)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_vtrace_out_of_range_action_poisons_losses(variant):
    """Standalone kernels: an action outside [0, A) makes the finalised loss scalars NaN
    (the device-side signal of a rejected batch) instead of a silently clamped result."""
    pi, mu, act, rew, disc, val = rand_case(5, 8, 16, 6)
    act[3, 7] = 6
    out = run_vtrace(pi, mu, act, rew, disc, val, variant=variant)
    assert np.isnan(out["losses"]).all()
    act[3, 7] = 2
    out = run_vtrace(pi, mu, act, rew, disc, val, variant=variant)
    assert np.isfinite(out["losses"]).all()
