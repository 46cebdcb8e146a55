"""PopArt value normalisation on the learner (include/fi_popart.h) on the GPU: the four kernels alone
between guard bytes against the fp64 rule, a handle with beta = 0 against a plain twin, one step
against the twin, the oracle's V-trace and popart_reference, the preserved outputs across an update,
rejected and non-finite batches, asynchronous steps, resume, the refusals and the coexistence with
column weights, the reward clip, the diagnostics and a prioritised ring.

u = 2^-24 (fp32 unit roundoff), DEN = 4 * 2^-149 (the denormal floor where a product can underflow).
Every bar is counted from the roundings of the operation it checks, in the test's docstring, and every
test prints its worst error / bar ratio."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_gpu_diag import TOL as DIAG_TOL
from test_gpu_prio import ETA, bar as prio_bar
from test_gpu_ring import B, T, Guarded, make_entries, make_learner, spaced
from test_gpu_vtrace import TOL as VT_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
U64 = 2.0 ** -53
DEN = 4 * 2.0 ** -149
STATES = ((1.0, -2.5), (0.37, 7.25), (41.5, -300.1))  # sigma, mu
# just past two grid strides of the streaming kernels on their 16-byte path (and eight on the other)
NBIG = 2 * 1024 * 256 * 4 + 5
SIZES = (1, 3, 4, 1027, NBIG)
POLICIES = (("mlp", 3), ("atari", 18))


def f32(x):
    return float(np.float32(x))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def state_bytes(sigma, mu, updates=5):
    from freeimpala_amd import popart
    return popart.pack_state(mu, sigma * sigma + mu * mu, sigma, updates)


def value_column(L, p=None):
    """(w, b): the value head's H weights and its bias in a parameter vector of learner L."""
    p = L.get_params() if p is None else p
    O = L.A + 1
    Hh = 512 if L.arch == "atari" else L.cfg.hidden
    head = p.size - O - Hh * O
    return p[head + L.A:head + Hh * O:O].copy(), p[-1]


def others(L, p):
    """p with the value column and its bias blanked: what a PopArt update must not touch."""
    q = p.copy()
    O = L.A + 1
    Hh = 512 if L.arch == "atari" else L.cfg.hidden
    head = q.size - O - Hh * O
    q[head + L.A:head + Hh * O:O] = 0
    q[-1] = 0
    return q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def kernel_tags(L):
    from freeimpala_amd._abi import lib
    buf = C.create_string_buffer(8192)
    ms, cnt = (C.c_float * 128)(), (C.c_int * 128)()
    n = lib().fi_learner_kernel_times(L._h, buf, 8192, ms, cnt, 128)
    return buf.value.decode().split("\n")[:n]


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_streaming_kernels_against_the_rule(n, off):
    """denormalise: one fma of the fp32 sigma_f, mu_f, a single rounding of sigma_f x + mu_f: half an ulp of
    the result, under u |result|; the bar is u (|sigma_f x| + |result|) (+ DEN). scale: one
    correctly rounded division, half an ulp, under u |result|; the bar is 2 u |result| (+ DEN), and
    sigma = 1 is exact. off = 1: the pointer one float behind a 16-byte boundary (the element-wise path).
    The float in front of it, the guards and the state block stay as they were."""
    from freeimpala_amd import hip, popart
    rs = np.random.RandomState(1000 * off + n % 9973)
    x = (rs.standard_normal(n + off) * 10.0 ** rs.uniform(-3, 3, n + off)).astype(np.float32)
    worst = [0.0, 0.0]
    for sigma, mu in STATES:
        st = state_bytes(sigma, mu)
        g = Guarded([(n + off, np.float32), (n + off, np.float32), (32, np.uint8)])
        hip.upload_ptr(g.ptr[0], x)
        hip.upload_ptr(g.ptr[1], x)
        hip.upload_ptr(g.ptr[2], st)
        popart.denormalize(g.ptr[0] + 4 * off, n, g.ptr[2])
        popart.scale_grad(g.ptr[1] + 4 * off, n, g.ptr[2])
        hip.synchronize()
        out = g.read(["values", "dvalue", "state"])
        g.free()
        np.testing.assert_array_equal(out["state"], st)
        for nm in ("values", "dvalue"):
            np.testing.assert_array_equal(bits(out[nm][:off]), bits(x[:off]), err_msg=nm + ": the float in front")
        sf, mf, xd = f32(sigma), f32(mu), x[off:].astype(np.float64)
        want = sf * xd + mf
        err = np.abs(out["values"][off:].astype(np.float64) - want)
        worst[0] = max(worst[0], float((err / (U * (np.abs(sf * xd) + np.abs(want)) + DEN)).max()))
        want = xd / sf
        if sigma == 1.0:
            np.testing.assert_array_equal(bits(out["dvalue"][off:]), bits(x[off:]), err_msg="sigma = 1 is the identity")
        err = np.abs(out["dvalue"][off:].astype(np.float64) - want)
        worst[1] = max(worst[1], float((err / (2 * U * np.abs(want) + DEN)).max()))
    print(f"n {n} off {off}: worst error / bar: denormalise {worst[0]:.3f}, scale {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def stat_bars(x, beta, mu, nu, ref):
    """What the device's mu', nu', sigma' may differ from popart_reference's by (ref: its result): the sums
    differ in their order alone, n 2^-53 sum |x| resp. sum x^2, which reaches the statistics as beta / n of
    that; at most four further roundings of numbers below |mu| + |mu'| resp. nu + nu'; and
    sigma' = sqrt(nu' - mu'^2) carries (d nu' + 2 |mu'| d mu' + 2^-52 (nu' + mu'^2)) / (2 sigma') and its
    own rounding."""
    d_mu = beta * U64 * float(np.abs(x).sum()) + 4 * U64 * (abs(mu) + abs(ref["mu"]))
    d_nu = beta * U64 * float((x * x).sum()) + 4 * U64 * (nu + ref["nu"])
    d_sg = (d_nu + 2 * abs(ref["mu"]) * d_mu + 2 * U64 * (ref["nu"] + ref["mu"] ** 2)) / (2 * ref["sigma"]) + \
        2 * U64 * ref["sigma"]
    return d_mu, d_nu, d_sg


def run_update(vs, w, b, st, off, H, stride, beta, skip=(0, 0, 0, 0)):
    from freeimpala_amd import hip, popart
    n = vs.size - off
    wsb = popart.workspace_bytes(n)
    g = Guarded([(n + off, np.float32), (w.size, np.float32), (1, np.float32), (32, np.uint8), (wsb, np.uint8),
                 (4, np.int32)])
    for k, a in enumerate((vs, w, b, st)):
        hip.upload_ptr(g.ptr[k], a)
    hip.upload_ptr(g.ptr[5], np.array(skip, np.int32))
    popart.update(g.ptr[0] + 4 * off, n, g.ptr[3], g.ptr[1] + 4 * (stride - 1), stride, H, g.ptr[2], beta, 1e-4, 1e6,
                  g.ptr[5], g.ptr[4], wsb)
    hip.synchronize()
    out = g.read(["vs", "w", "b", "state", "ws", "skip"])
    g.free()
    np.testing.assert_array_equal(bits(out["vs"]), bits(vs), err_msg="vs is read only")
    np.testing.assert_array_equal(out["skip"], np.array(skip, np.int32), err_msg="the flag words are read only")
    return out


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_update_against_the_rule(n, off):
    """fi_popart_update with beta = 1, so mu' = S1 / n and nu' = S2 / n. The device adds n fp64 numbers in
    some fixed order: n - 1 additions, each within 2^-53 of a partial sum that sum |x| bounds, and one
    division: |n mu' - S1| <= n 2^-53 sum |x|, and the same for nu' with sum x^2 (the squares of fp32
    numbers are exact in fp64). The reference sums are math.fsum's. sigma', the H = 300 weights (more than
    one lane round, at stride 4: the other three columns stay bit for bit) and the bias: sigma' within
    stat_bars of the reference's, then one fp64 expression each and one rounding to fp32: within 1 ulp
    (fp32) of popart_reference. With a skip flag set, or a NaN among the targets, the state,
    w and b keep their bits."""
    from freeimpala_amd import popart
    H, stride = 300, 4
    rs = np.random.RandomState(77 + 1000 * off + n % 9973)
    vs = np.empty(n + off, np.float32)
    vs[off:] = (rs.standard_normal(n) * 3.0 + 1.5).astype(np.float32)
    vs[:off] = 1e30
    w = rs.standard_normal(H * stride).astype(np.float32)
    b = np.array([0.3], np.float32)
    xs = vs[off:].astype(np.float64)
    s1, s2, a1 = math.fsum(xs.tolist()), math.fsum((xs * xs).tolist()), math.fsum(np.abs(xs).tolist())
    worst = [0.0, 0.0, 0.0]
    for sigma, mu in STATES:
        st = state_bytes(sigma, mu)
        out = run_update(vs, w, b, st, off, H, stride, 1.0)
        got = popart.unpack_state(out["state"])
        ref = popart.popart_reference(np.zeros(1), xs, w[stride - 1::stride], b[0], mu, sigma * sigma + mu * mu, 1.0, 1e-4, 1e6,
                                      sigma=sigma)
        assert got["updates"] == 6 and ref["updated"]
        worst[0] = max(worst[0], abs(got["mu"] - s1 / n) / (U64 * a1), abs(got["nu"] - s2 / n) / (U64 * s2))
        if n == 1:
            assert got["sigma"] == ref["sigma"] == 1e-4, "one target has no variance: sigma_min"
        else:
            worst[0] = max(worst[0], abs(got["sigma"] - ref["sigma"]) / stat_bars(xs, 1.0, mu, sigma * sigma + mu * mu, ref)[2])
        wcol = out["w"][stride - 1::stride].astype(np.float64)
        worst[1] = max(worst[1], float((np.abs(wcol - ref["w"]) / ulp32(ref["w"])).max()))
        worst[2] = max(worst[2], abs(float(out["b"][0]) - ref["b"]) / float(ulp32(ref["b"])))
        keep = np.ones(H * stride, bool)
        keep[stride - 1::stride] = False
        np.testing.assert_array_equal(bits(out["w"][keep]), bits(w[keep]), err_msg="the policy's columns")
    print(f"n {n} off {off}: worst error / bar: moments {worst[0]:.3f}, w' {worst[1]:.3f} ulp, b' {worst[2]:.3f} ulp")
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and worst[2] <= 1.0
    # nothing moves: a skipped update (either flag), a NaN or an Inf among the targets
    st = state_bytes(0.37, 7.25)
    bad_nan, bad_inf = vs.copy(), vs.copy()
    bad_nan[off + n // 2] = np.nan
    bad_inf[off + n - 1] = np.inf
    for what, v, skip in (("actions flag", vs, (2, 0, 0, 0)), ("non-finite flag", vs, (0, 1, 0, 0)),
                          ("NaN target", bad_nan, (0, 0, 0, 0)), ("Inf target", bad_inf, (0, 0, 0, 0))):
        out = run_update(v, w, b, st, off, H, stride, 1.0, skip)
        np.testing.assert_array_equal(out["state"], st, err_msg=what)
        np.testing.assert_array_equal(bits(out["w"]), bits(w), err_msg=what)
        np.testing.assert_array_equal(bits(out["b"]), bits(b), err_msg=what)


# ------------------------------------------------------------------ 2. beta = 0 is the plain step
@pytest.mark.parametrize("arch,A", POLICIES)
def test_beta_zero_is_the_plain_step(arch, A):
    """mu = 0, sigma = 1 and beta = 0: fmaf(1, v, 0) = v, d / 1 = d, and the update rewrites w sigma / sigma
    and (sigma b + 0) / sigma: value equality throughout (a -0.0 may come back +0.0 from the fma)."""
    P, Q = make_learner(arch, A), make_learner(arch, A)
    P.enable_popart(beta=0.0)
    for k in range(3):
        for L in (P, Q):
            L.synth(seed=30 + k)
            L.step_resident()
        for nm in ("params", "adam_m", "adam_v", "grads", "vs", "values", "dvalue"):
            assert np.array_equal(P.tensor(nm), Q.tensor(nm)), (k, nm)
    s = P.popart_state()
    assert (s["enabled"], s["updates"], s["mu"], s["nu"], s["sigma"], s["beta"]) == (True, 3, 0.0, 1.0, 1.0, 0.0)
    assert Q.popart_state() == dict(enabled=False, beta=3e-4, sigma_min=1e-4, sigma_max=1e6, mu=0.0, nu=1.0, sigma=1.0,
                                    updates=0)
    P.close()
    Q.close()


@pytest.mark.parametrize("arch,A", POLICIES)
def test_a_plain_handle_lists_no_new_tag(arch, A):
    """The launch tags of one profiled step: the plain handle's are the PopArt handle's without the three
    popart_* tags, in the same order; those sit behind the forward, behind V-trace and behind the optimiser."""
    P, Q = make_learner(arch, A), make_learner(arch, A)
    P.enable_popart()
    for L in (P, Q):
        L.synth(seed=3)
        L.set_profiling(True)
        L.step_resident()
    tp, tq = kernel_tags(P), kernel_tags(Q)
    assert not [t for t in tq if "popart" in t] and len(tq) > 5
    assert [t for t in tp if not t.startswith("popart_")] == tq
    assert [t for t in tp if t.startswith("popart_")] == ["popart_denorm", "popart_scale", "popart_update"]
    assert tp[tp.index("vtrace") - 1] == "popart_denorm" and tp[tp.index("vtrace") + 1] == "popart_scale"
    assert tp[tp.index("optimizer") + 1] == "popart_update"
    P.close()
    Q.close()


# ------------------------------------------------------------------ 3. inside a step
MU0, NU0, SIGMA0 = 3.0, 9.0 + 6.25, 2.5


def popart_twin(arch, A, beta, **kw):
    P = make_learner(arch, A, **kw)
    P.enable_popart(beta=beta)
    P.set_popart_state(MU0, NU0)
    return P


@pytest.mark.parametrize("arch,A", POLICIES)
def test_one_step_against_the_twin_and_the_oracle(arch, A, orc):
    """sigma = 2.5, mu = 3, beta = 0.25; P with PopArt, Q plain, R with PopArt and beta = 0 (the same step,
    statistics and value column left alone: the post-optimiser parameters).
    values: Q's are the n of P (the same forward), P's meet the denormalise bar u (|sigma_f n| + |result|).
    vs and dvalue: the oracle's V-trace on P's read-back tensors at test_gpu_vtrace's tolerance
    1e-5 max(1, |ref|); dvalue sigma_f with 2 u |ref| more (the division's rounding and the product's).
    The statistics: popart_reference on the read-back vs, within stat_bars (the moments bar carried through
    the rule).
    The value column and the bias: within 1 ulp (fp32) of the reference on R's parameters; every other
    parameter equals R's bit for bit."""
    from freeimpala_amd import popart
    P, Q, R = popart_twin(arch, A, 0.25), make_learner(arch, A), popart_twin(arch, A, 0.0)
    for L in (P, Q, R):
        L.synth(seed=41)
        L.step_resident()
    n_q, v_p = Q.tensor("values").astype(np.float64), P.tensor("values").astype(np.float64)
    want = SIGMA0 * n_q + MU0
    r_val = float((np.abs(v_p - want) / (U * (np.abs(SIGMA0 * n_q) + np.abs(want)) + DEN)).max())
    sh = dict(logits=(T + 1, B, A), mu=(T, B, A), actions=(T, B), rewards=(T, B), discounts=(T, B), values=(T + 1, B))
    t = {k: P.tensor(k, np.int32 if k == "actions" else np.float32, s) for k, s in sh.items()}
    ref = orc.vtrace_loss(t["logits"][:T], t["mu"], t["actions"], t["rewards"], t["discounts"], t["values"])
    vs, dv = P.tensor("vs", shape=(T, B)), P.tensor("dvalue", shape=(T + 1, B))
    rv = np.asarray(ref["vs"], np.float64)
    r_vs = float((np.abs(vs - rv) / (VT_TOL * np.maximum(1.0, np.abs(rv)))).max())
    rd = np.asarray(ref["dvalue"], np.float64)
    r_dv = float((np.abs(dv.astype(np.float64) * SIGMA0 - rd) / (VT_TOL * np.maximum(1.0, np.abs(rd)) + 2 * U * np.abs(rd))).max())
    assert (dv[T] == 0).all() and (rd[T] == 0).all(), "row T carries no gradient and is not scaled"
    # the statistics
    got, x = P.popart_state(), vs.astype(np.float64).reshape(-1)
    w_r, b_r = value_column(R)
    pr = popart.popart_reference(n_q, x, w_r, b_r, MU0, NU0, 0.25)
    assert got["updates"] == 1 and pr["updated"] and R.popart_state()["updates"] == 1
    assert (R.popart_state()["mu"], R.popart_state()["sigma"]) == (MU0, SIGMA0)
    d_mu, d_nu, d_sg = stat_bars(x, 0.25, MU0, NU0, pr)
    r_st = max(abs(got["mu"] - pr["mu"]) / d_mu, abs(got["nu"] - pr["nu"]) / d_nu, abs(got["sigma"] - pr["sigma"]) / d_sg)
    assert abs(pr["mu"] - MU0) > 0.01 and abs(pr["sigma"] - SIGMA0) > 0.01, "the statistics moved"
    # the head
    p_p, p_r = P.get_params(), R.get_params()
    np.testing.assert_array_equal(bits(others(P, p_p)), bits(others(R, p_r)), err_msg="parameters outside the value column")
    w_p, b_p = value_column(P, p_p)
    r_w = float((np.abs(w_p.astype(np.float64) - pr["w"]) / ulp32(pr["w"])).max())
    r_b = abs(float(b_p) - pr["b"]) / float(ulp32(pr["b"]))
    print(f"{arch}: worst error / bar: values {r_val:.3f}, vs {r_vs:.3f}, dvalue sigma {r_dv:.3f}, statistics {r_st:.3f}, "
          f"w' {r_w:.3f} ulp, b' {r_b:.3f} ulp")
    assert max(r_val, r_vs, r_dv, r_st, r_w, r_b) <= 1.0
    for L in (P, Q, R):
        L.close()


# ------------------------------------------------------------------ 4. outputs are preserved
# the Atari head runs on bf16 copies of its weights: see test_outputs_are_preserved
ATARI_PRESERVE_BAR = 4 * 6.8e-5


@pytest.mark.parametrize("arch,A", POLICIES)
def test_outputs_are_preserved(arch, A):
    """set_lr(0), beta = 0.5, two steps on one resident batch from mu = -2, sigma = 0.5: the optimiser moves
    nothing, the statistics move by more than 1 %, and step 2's values -- the rewritten head under the new
    statistics -- are step 1's.

    MLP (h2 is readable, fp32 throughout). With V = sigma (h . w + b) + mu the exact, preserved number and
    S = sum_j |h_j w_j| + |b|, a side's value differs from V by: the head's accumulation of H products and
    H additions in fp32, (H + 2) u S, times sigma; the roundings of sigma_f and mu_f, u |sigma n| + u |mu|;
    the fma, u |value|. Step 2 also carries one rounding of each w'_j and of b', u S' times sigma'. The bar
    is the sum over both sides (+ DEN).

    Atari: the heads' GEMM reads bf16 copies of the weights (atari_sync_weights), so w and w' are each
    rounded to 8 bits before the product and the two sides differ by up to 2^-9 (sigma S + sigma' S'),
    which no fp32 tolerance of `values` covers, and the fc activations S is made of are not readable. So
    this bar is a measured one, the only one in this file: the error against popart_reference's prediction
    (the same number on both sides) is measured, max |values2 - values1| / max(1, max |values1|), and the bar
    is 4 times the worst observed, 6.8e-5 at ("atari", 18), the one Atari case, on an MI355X (the fp32 forward
    tolerance of tests/test_gpu_learner.py, 1e-5 max(1, sigma'), is below that, as the count above says it must be)."""
    from freeimpala_amd import popart
    L = make_learner(arch, A)
    L.enable_popart(beta=0.5)
    L.set_popart_state(-2.0, 4.0 + 0.25)
    L.set_lr(0.0)
    L.synth(seed=52)
    p0, s0 = L.get_params(), L.popart_state()
    L.step_resident()
    v1, p1, s1 = L.tensor("values").astype(np.float64), L.get_params(), L.popart_state()
    L.step_resident()
    v2, s2 = L.tensor("values").astype(np.float64), L.popart_state()
    np.testing.assert_array_equal(bits(others(L, p1)), bits(others(L, p0)), err_msg="lr = 0: nothing else moves")
    assert (s0["mu"], s0["sigma"], s1["updates"], s2["updates"]) == (-2.0, 0.5, 1, 2)
    assert abs(s1["mu"] - s0["mu"]) > 0.01 * abs(s0["mu"]) and abs(s1["sigma"] - s0["sigma"]) > 0.01 * s0["sigma"], (s0, s1)
    (w0, b0), (w1, b1) = value_column(L, p0), value_column(L, p1)
    assert not np.array_equal(w0, w1) and b0 != b1
    if arch == "mlp":
        H = L.cfg.hidden
        h = np.abs(L.tensor("h2", shape=((T + 1) * B, H)).astype(np.float64))
        hs = L.tensor("h2", shape=((T + 1) * B, H)).astype(np.float64)
        S0, S1 = h @ np.abs(w0.astype(np.float64)) + abs(float(b0)), h @ np.abs(w1.astype(np.float64)) + abs(float(b1))
        n1 = popart.preserved_output(hs, w0, b0, 0.0, 1.0)
        n2 = popart.preserved_output(hs, w1, b1, 0.0, 1.0)
        bar = U * ((H + 2) * s0["sigma"] * S0 + np.abs(s0["sigma"] * n1) + abs(s0["mu"]) + np.abs(v1)) + \
            U * ((H + 3) * s1["sigma"] * S1 + np.abs(s1["sigma"] * n2) + abs(s1["mu"]) + np.abs(v2)) + DEN
        ratio = float((np.abs(v2 - v1) / bar).max())
        print(f"mlp: worst |values2 - values1| / bar {ratio:.3f} (worst difference {np.abs(v2 - v1).max():.3e})")
        assert ratio <= 1.0
    else:
        err = float(np.abs(v2 - v1).max() / max(1.0, np.abs(v1).max()))
        print(f"atari: max |values2 - values1| / max(1, max |values1|) = {err:.3e} (bar {ATARI_PRESERVE_BAR:.3e})")
        assert err <= ATARI_PRESERVE_BAR
    L.close()


# ------------------------------------------------------------------ 5. rejected and non-finite batches
@pytest.mark.parametrize("what", ["action", "reward"])
def test_a_skipped_update_leaves_statistics_and_head(what):
    from freeimpala_amd._abi import FiError
    arch, A = "mlp", 3
    P, Q = popart_twin(arch, A, 0.25), make_learner(arch, A)
    rcs = []
    for L in (P, Q):
        L.synth(seed=61)
        L.step_resident()
    s0, p0 = P.popart_state(), P.get_params()
    assert s0["updates"] == 1
    good = {nm: P.tensor(nm, dt) for nm, dt in (("actions", np.int32), ("rewards", np.float32))}
    bad = {k: v.copy() for k, v in good.items()}
    if what == "action":
        bad["actions"][3] = A + 2
    else:
        bad["rewards"][4] = np.nan
    for L in (P, Q):
        for nm in bad:
            L.upload(nm, bad[nm])
        with pytest.raises(FiError) as e:
            L.step_resident()
        rcs.append(str(e.value).split(":")[0])
    assert rcs[0] == rcs[1] and ("rc=-1" if what == "action" else "rc=-7") in rcs[0], rcs
    assert P.popart_state() == s0, "the statistics keep their bits"
    np.testing.assert_array_equal(bits(P.get_params()), bits(p0), err_msg="parameters, the value column among them")
    for nm in good:
        P.upload(nm, good[nm])
    P.step_resident()
    s1, (w0, b0), (w1, b1) = P.popart_state(), value_column(P, p0), value_column(P)
    assert s1["updates"] == 2 and s1["mu"] != s0["mu"] and s1["sigma"] != s0["sigma"]
    assert not np.array_equal(w0, w1) and b0 != b1
    P.close()
    Q.close()


# ------------------------------------------------------------------ 6. asynchronous steps
def test_async_steps_equal_waited_steps():
    """Four ring steps enqueued without a wait: every kernel reads the statistics from the device block, so
    step k + 1 sees what step k left. Bit for bit the four waited steps of a twin."""
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, 4 * B, A, seed=71)
    res = []
    for wait in (True, False):
        R = popart_twin(arch, A, 0.25)
        E = R.entry_bytes
        ring = EntryRing(E, 32, seed=5)
        src = spaced(raw, E)
        ring.push(src.ptr, E, 4 * B)
        for _ in range(4):
            assert (R.step_ring(ring, wait=wait) is None) == (not wait)
        if not wait:
            R.wait()
        res.append((R.popart_state(), R.get_params(), R.tensor("adam_m"), R.tensor("adam_v")))
        src.free()
        ring.close()
        R.close()
    assert res[0][0] == res[1][0] and res[0][0]["updates"] == 4 and res[0][0]["mu"] != MU0
    for k in (1, 2, 3):
        np.testing.assert_array_equal(bits(res[0][k]), bits(res[1][k]))


# ------------------------------------------------------------------ 7. resume
def test_resume_equals_the_straight_run():
    """enable_popart, set_popart_state, load_state on a fresh handle: set_popart_state derives sigma from mu, nu
    by the rule's own expression, so the resumed statistics are the saved ones bit for bit. `updates` is the
    handle's own count and starts again."""
    arch, A = "mlp", 3

    def steps(L, first, count):
        for k in range(first, first + count):
            L.synth(seed=80 + k)
            L.step_resident()

    S = make_learner(arch, A)
    S.enable_popart(beta=0.25)
    steps(S, 0, 4)
    F = make_learner(arch, A)
    F.enable_popart(beta=0.25)
    steps(F, 0, 2)
    blob, half = F.save_state(), F.popart_state()
    F.close()
    G_ = make_learner(arch, A)
    G_.enable_popart(beta=0.25)
    G_.set_popart_state(half["mu"], half["nu"])
    G_.load_state(blob)
    again = G_.popart_state()
    assert (again["mu"], again["nu"], again["sigma"], again["updates"]) == (half["mu"], half["nu"], half["sigma"], 0)
    steps(G_, 2, 2)
    for nm in ("params", "adam_m", "adam_v"):
        np.testing.assert_array_equal(bits(G_.tensor(nm)), bits(S.tensor(nm)), err_msg=nm)
    s, g = S.popart_state(), G_.popart_state()
    assert (g["updates"], s["updates"]) == (2, 4)
    assert {k: v for k, v in g.items() if k != "updates"} == {k: v for k, v in s.items() if k != "updates"}
    assert G_.save_state() == S.save_state()
    S.close()
    G_.close()


EXE = os.path.join(ROOT, "build", "host_popart_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_popart_check"], check=True)
    out = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("popart mlp:")])
    assert len(out[0]) == 1 and "updates 4" in out[0][0] and out[0][0].endswith("bytes equal")
    assert out[0] == out[1], "two runs print the same bits"


# ------------------------------------------------------------------ 8. refusals and coexistence
def test_refusals():
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp", 3)

    def refused(match, call, *args, **kw):
        with pytest.raises(FiError, match=match):
            call(*args, **kw)

    refused(r"rc=-4: .*PopArt is off", L.set_popart_state, 0.0, 1.0)
    refused(r"rc=-4: .*PopArt is off", L.popart_state_ptr)
    refused(r"rc=-1: .*beta -0.1\d* outside \[0, 1\]", L.enable_popart, -0.1)
    refused(r"rc=-1: .*beta 1.5\d* outside \[0, 1\]", L.enable_popart, 1.5)
    refused(r"rc=-1: .*beta nan", L.enable_popart, float("nan"))
    refused(r"rc=-1: .*sigma_min 0.0\d* outside \(0, 1\]", L.enable_popart, 0.1, 0.0)
    refused(r"rc=-1: .*sigma_min 2.0\d* outside \(0, 1\]", L.enable_popart, 0.1, 2.0)
    refused(r"rc=-1: .*sigma_max 0.5\d* is below 1", L.enable_popart, 0.1, 1e-4, 0.5)
    refused(r"rc=-1: .*sigma_max inf", L.enable_popart, 0.1, 1e-4, float("inf"))
    assert L.popart_state()["enabled"] is False
    L.enable_popart(0.1, 1e-3, 1e3)
    assert L.popart_state_ptr() % 8 == 0
    refused(r"rc=-1: .*nu 3.0\d* < mu\^2 4.0", L.set_popart_state, 2.0, 3.0)
    refused(r"rc=-1: .*not finite", L.set_popart_state, float("nan"), 1.0)
    refused(r"rc=-1: .*not finite", L.set_popart_state, 0.0, float("inf"))
    s = L.popart_state()
    assert (s["enabled"], s["beta"], s["sigma_min"], s["sigma_max"], s["mu"], s["nu"], s["sigma"]) == (True, 0.1, 1e-3, 1e3, 0.0, 1.0, 1.0)
    L.set_popart_state(2.0, 4.0)  # no variance: the lower bound
    assert L.popart_state()["sigma"] == 1e-3
    L.set_popart_state(3.0, 15.25)
    L.enable_popart(0.2)  # a second call: the three numbers change, the statistics stay
    s = L.popart_state()
    assert (s["beta"], s["sigma_min"], s["sigma_max"], s["mu"], s["nu"], s["sigma"]) == (0.2, 1e-4, 1e6, 3.0, 15.25, 2.5)
    L.close()


def test_coexists_with_weights_clip_and_diagnostics():
    """Column weights, the reward clip and the diagnostics on steps with PopArt: `values` and `vs` are
    unnormalised where the diagnostics read them, so explained_variance equals diag.offpolicy_reference on the
    read-back tensors at test_gpu_diag's tolerance."""
    from freeimpala_amd import diag
    arch, A = "mlp", 3
    L = popart_twin(arch, A, 0.25)
    rs = np.random.RandomState(9)
    L.set_column_weights(rs.uniform(0.2, 2.0, B).astype(np.float32))
    L.set_reward_clip(0.5)
    worst = 0.0
    for k in range(2):
        L.synth(seed=90 + k)
        L.step_resident()
        L.enqueue_diagnostics()
        d = L.read_diagnostics()
        c = dict(pi=L.tensor("logits", shape=(T + 1, B, A))[:T].copy(), mu=L.tensor("mu", shape=(T, B, A)),
                 act=L.tensor("actions", np.int32, (T, B)), rew=L.tensor("rewards", shape=(T, B)),
                 disc=L.tensor("discounts", shape=(T, B)), val=L.tensor("values", shape=(T + 1, B)),
                 vs=L.tensor("vs", shape=(T, B)))
        assert np.abs(c["rew"]).max() <= 0.5
        ref = diag.offpolicy_reference(c["pi"], c["mu"], c["act"], c["rew"], c["disc"], c["val"], c["vs"], L.cfg.hp)[0]
        for key in ("explained_variance", "mean_abs_td"):
            worst = max(worst, abs(d[key] - ref[key]) / (DIAG_TOL * max(1.0, abs(ref[key]))))
    assert L.popart_state()["updates"] == 2
    print(f"explained_variance: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    L.close()


def test_a_prioritised_step_refreshes_from_unnormalised_values():
    from freeimpala_amd.prio import td_priorities
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, B, A, seed=95)
    R = popart_twin(arch, A, 0.25)
    E = R.entry_bytes
    ring = EntryRing(E, 8, seed=4)
    ring.enable_priorities(ETA, 1.0)
    src = spaced(raw, E)
    ring.push(src.ptr, E, B)
    R.step_ring(ring, prioritized=True)
    vs, values = R.tensor("vs").reshape(T, B), R.tensor("values").reshape(T + 1, B)
    want, got = td_priorities(vs, values, ETA), ring.priorities().astype(np.int64)
    ratio = max(abs(int(g) - int(w)) / prio_bar(int(w), T) for g, w in zip(got, want))
    print(f"priorities: worst error / bar {ratio:.3f}")
    assert ratio <= 1.0 and R.popart_state()["updates"] == 1
    for h in (ring, R):
        h.close()
    src.free()
