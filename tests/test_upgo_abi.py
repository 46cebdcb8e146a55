"""The UPGO term's header (include/fi_upgo.h) without a device: the exports, the two structures against the C
compiler's layout, the workspace of a refused shape, and upgo_reference (freeimpala_amd/upgo.py), the GPU tests' only
yardstick, on its own: both extremes of the rule in closed form and its gradient against a central difference."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["coeff", "rho_bar"]
STATS_FIELDS = ["loss_u", "sum_au", "rows", "links_up", "rows_positive"]


def small_case(T=3, B=4, A=5, seed=11):
    rs = np.random.RandomState(seed)
    return dict(logits=rs.randn(T, B, A).astype(np.float32), mu=rs.randn(T, B, A).astype(np.float32),
                actions=rs.randint(0, A, (T, B)).astype(np.int32), rewards=rs.randn(T, B).astype(np.float32),
                discounts=np.where(rs.rand(T, B) < 0.2, 0.0, 0.9).astype(np.float32),
                values=rs.randn(T + 1, B).astype(np.float32))


def test_exports_and_layouts_match_c(tmp_path):
    from freeimpala_amd import _abi, upgo
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_upgo_")} == set(upgo.SIGNATURES)
    upgo.lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_upgo.h"\nint main(){'
           'printf("%zu", sizeof(fi_upgo_params));' +
           "".join(f'printf(" %zu", offsetof(fi_upgo_params, {f}));' for f in PARAM_FIELDS) +
           'printf(" %zu", sizeof(fi_upgo_stats));' +
           "".join(f'printf(" %zu", offsetof(fi_upgo_stats, {f}));' for f in STATS_FIELDS) +
           'printf(" %.9g %.9g", (double)FI_UPGO_COEFF, (double)FI_UPGO_RHO_BAR);return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    P, S = upgo.UpgoParams, upgo.UpgoStats
    assert [f for f, _ in P._fields_] == PARAM_FIELDS and [f for f, _ in S._fields_] == STATS_FIELDS
    want = ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAM_FIELDS] + [ctypes.sizeof(S)] +
            [getattr(S, f).offset for f in STATS_FIELDS])
    assert [int(v) for v in got[:-2]] == want == [8, 0, 4, 40, 0, 8, 16, 24, 32]
    assert [float(v) for v in got[-2:]] == [upgo.COEFF, upgo.RHO_BAR] and upgo.STATE_BYTES == 40
    st = dict(loss_u=-1.5, sum_au=2.25, rows=7, links_up=3, rows_positive=4)
    raw = np.frombuffer(bytes(S(**st)), np.uint8)
    assert upgo.unpack_state(raw) == st


@pytest.mark.parametrize("shape", [(5, 24, 1), (5, 24, 65), (0, 24, 18), (5, 0, 18), (1 << 13, 1 << 12, 64)])
def test_workspace_of_a_refused_shape_is_zero(shape):
    from freeimpala_amd import upgo
    assert upgo.workspace_bytes(*shape) == 0 and upgo.workspace_bytes(5, 24, 18) >= 5 * 24 * 4


@pytest.mark.parametrize("up", [False, True], ids=["none_up", "all_up"])
def test_reference_extremes(up):
    """Rewards far below (above) what V asks for: no link is up and AU is the one-step TD advantage; every link is up
    and G is the discounted return to the bootstrap V_T."""
    from freeimpala_amd.upgo import upgo_reference
    c = small_case(T=6)
    c["rewards"] = c["rewards"] + np.float32(100.0 if up else -100.0)
    ref = upgo_reference(**c)
    r, g, v = (c[k].astype(np.float64) for k in ("rewards", "discounts", "values"))
    T = r.shape[0]
    assert ref["links_up"] == (T - 1) * r.shape[1] * up and not ref["up"][T - 1].any()
    if up:
        want = v[T].copy()
        for t in range(T - 1, -1, -1):
            want = r[t] + g[t] * want
            np.testing.assert_allclose(ref["G"][t], want, rtol=1e-13)
    else:
        np.testing.assert_allclose(ref["AU"], r + g * v[1:] - v[:T], rtol=1e-13)
    assert ref["rows"] == r.size and ref["rows_positive"] == int((ref["AU"] > 0).sum())
    np.testing.assert_allclose(ref["sum_au"], ref["AU"].sum(), rtol=1e-13)


def test_reference_gradient_is_the_central_difference_of_the_loss():
    """coeff times d loss_u / d logits with rho AU held constant, at (3, 4, 5); rho_bar = 1e30 never binds, so the
    weights are the ratios themselves. fp64, h = 1e-6: 1e-7 absolute."""
    from freeimpala_amd.upgo import upgo_reference
    c = small_case()
    ref = upgo_reference(**c, coeff=0.75, rho_bar=1e30)
    w, a = ref["rho"] * ref["AU"], c["actions"].astype(np.int64)

    def loss(z):  # - sum w log pi(a), w constant
        z = z - z.max(-1, keepdims=True)
        lp = z - np.log(np.exp(z).sum(-1, keepdims=True))
        return float(-(w * np.take_along_axis(lp, a[..., None], -1)[..., 0]).sum())

    z0, h = c["logits"].astype(np.float64), 1e-6
    num = np.zeros_like(z0)
    for i in np.ndindex(*z0.shape):
        zp, zm = z0.copy(), z0.copy()
        zp[i] += h
        zm[i] -= h
        num[i] = (loss(zp) - loss(zm)) / (2 * h)
    assert np.abs(ref["dlogits"] - float(np.float32(0.75)) * num).max() <= 1e-7
    assert abs(ref["loss_u"] - loss(z0)) <= 1e-12 * max(1.0, abs(ref["loss_u"]))
