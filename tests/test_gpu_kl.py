"""The adaptive KL penalty (include/fi_kl.h) on the GPU: the two kernels alone between guard bytes against
kl_reference / adapt_reference at test_gpu_diag's shapes; q = pi bit for bit, exact; two launches, the same bits;
every branch of the finalize; the refusals; then a handle on both policies: the behaviour reference under V-trace
against a twin and against the diagnostics' KL(mu || pi), the target reference under the surrogate against
target_reference, period 1 (three exact halvings), the steps that enqueue nothing, disable against a twin,
asynchronous steps, a rejected batch, column weights, set_kl_coeff, the refusals and the C++ check program.

The bars are the project's own, imported: TOL = 1e-5 max(1, |ref|) for tensors and for mean_kl and kl_sum / rows (fp64
sums of fp32 terms that each carry the tensors' error, as test_gpu_target.moments_close treats mean_log_r). Counters are
exact. The coefficient is exact: its arithmetic is fp64 on both sides once the branch agrees, and every test asserts on
the reference first that its mean KL is not near a threshold (kl.near_threshold; the seeds are chosen on the CPU for
it). Every comparison prints its worst error / bar before it asserts."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_diag import SHAPES, make_case as diag_case, make_learner
from test_gpu_popart import kernel_tags
from test_gpu_ring import Guarded
from test_gpu_surrogate import CLIP, OUT, bits, ids, learner_outputs, state_of, worst
from test_gpu_target import learner_case as target_case, perturbed, target_block, target_learner, target_logits
from test_gpu_vtrace import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHS = ["mlp", "atari"]
STATE0 = dict(mean_kl=-1.0, kl_sum=-2.0, rows=7, updates=5, raised=1, lowered=2)  # what a launch finds in the block
NAMES = ["dlogits", "state", "ws", "skip"]


def make_case(T, B, A, nan=False):
    """test_gpu_diag's pi and mu (mu = pi + N(0, 1): a mean KL of some tenths) and random dlogits to add onto."""
    c = diag_case(T, B, A)
    d0 = np.random.RandomState(1000 * T + 10 * B + A + 1).standard_normal((T, B, A)).astype(np.float32)
    pi = c["pi"].copy()
    if nan:
        pi[0, 0, 0] = np.nan
    return pi, c["mu"], d0


class Launch:
    """pi and q in device memory; dlogits, the block, the workspace and the skip words between guards."""

    def __init__(self, case):
        from freeimpala_amd import hip, kl
        self.case = [np.ascontiguousarray(x) for x in case]
        self.T, self.B, self.A = case[0].shape
        self.inp = [hip.DeviceBuffer.from_array(x) for x in self.case[:2]]
        self.ws_bytes = kl.workspace_bytes(self.T, self.B, self.A)
        assert self.ws_bytes > 0
        self.g = Guarded([(case[0].size, np.float32), (48, np.uint8), (self.ws_bytes, np.uint8), (2, np.int32)])

    def fill(self, coeff, **state):
        """dlogits <- the case's, the block <- coeff and STATE0 (or what is named)."""
        from freeimpala_amd import hip, kl
        hip.upload_ptr(self.g.ptr[0], self.case[2])
        self.state0 = dict(STATE0, coeff=float(coeff), **state)
        hip.upload_ptr(self.g.ptr[1], kl.pack_state(**self.state0))
        return self

    def penalty(self, **over):
        from freeimpala_amd import kl
        p = self.g.ptr
        kw = dict(T=self.T, B=self.B, A=self.A, pi=self.inp[0].ptr, q=self.inp[1].ptr, dlogits=p[0], state=p[1], ws=p[2],
                  ws_bytes=self.ws_bytes)
        kw.update(over)
        kl.kl_penalty_dev(kw["T"], kw["B"], kw["A"], kw["pi"], kw["q"], kw["dlogits"], kw["state"], kw["ws"], kw["ws_bytes"])
        return self

    def finalize(self, prm, skip=(0, 0), **over):
        from freeimpala_amd import hip, kl
        p = self.g.ptr
        if skip is not None:
            hip.upload_ptr(p[3], np.array(skip, np.int32))
        kw = dict(T=self.T, B=self.B, A=self.A, state=p[1], ws=p[2], ws_bytes=self.ws_bytes)
        kw.update(over)
        kl.kl_finalize_dev(kw["T"], kw["B"], kw["A"], prm, kw["state"], kw["ws"], kw["ws_bytes"], None if skip is None else p[3])
        return self

    def raw(self):
        """Every output's array, the guards checked, and the inputs bit-unchanged."""
        from freeimpala_amd import hip
        hip.synchronize()
        out = self.g.read(NAMES)
        for b, x in zip(self.inp, self.case):
            np.testing.assert_array_equal(b.download(np.uint8, (x.nbytes,)), x.view(np.uint8).reshape(-1), err_msg="an input")
        return out

    def read(self):
        from freeimpala_amd import kl
        o = self.raw()
        return o["dlogits"].reshape(self.T, self.B, self.A), kl.unpack_state(o["state"])

    def free(self):
        for b in self.inp:
            b.free()
        self.g.free()


def mean_close(st, ref, what):
    """rows exact; mean_kl and kl_sum / rows within TOL max(1, |ref|) of the reference's mean."""
    assert st["rows"] == ref["rows"]
    bar = TOL * max(1.0, abs(ref["mean_kl"]))
    r = max(abs(st["mean_kl"] - ref["mean_kl"]), abs(st["kl_sum"] / st["rows"] - ref["mean_kl"])) / bar
    print(f"{what}: mean_kl {st['mean_kl']!r} ref {ref['mean_kl']!r}; worst error / bar {r:.3f}")
    assert r <= 1.0


def adapted(st, state0, ref_mean, prm, skipped=False):
    """coeff, updates, raised, lowered are exactly adapt_reference's on the reference's mean, which is not near a
    threshold (asserted first)."""
    from freeimpala_amd import kl
    assert not kl.near_threshold(ref_mean, prm), f"pick another seed: mean KL {ref_mean} is near a threshold"
    want = kl.adapt_reference(state0, ref_mean, prm, skipped)
    got = {k: st[k] for k in ("coeff", "updates", "raised", "lowered")}
    print(f"coeff {state0['coeff']!r} -> {got['coeff']!r} (ref {want['coeff']!r}), updates {got['updates']}, "
          f"raised {got['raised']}, lowered {got['lowered']}")
    assert got == {k: want[k] for k in got}
    return want


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("c", [0.5, 4.0])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_match_reference(shape, c):
    """dlogits, pre-filled with random values, within TOL of kl_reference; after the finalize rows is exact, mean_kl and
    kl_sum / rows are within TOL and coeff, updates, raised, lowered are adapt_reference's, with kl_target a third of the
    reference's mean at the larger c (a raise) and the default at the smaller (a raise where the mean is tenths, a
    halving at the one row of the first shape)."""
    from freeimpala_amd import kl
    case = make_case(*shape)
    ref = kl.kl_reference(*case, c)
    prm = kl.params(kl_target=ref["mean_kl"] / 3 if c == 4.0 else kl.KL_TARGET)
    L = Launch(case).fill(c).penalty().finalize(prm)
    got, st = L.read()
    L.free()
    r = worst(got, ref["dlogits"])
    print(f"{ids(shape)} c {c}: dlogits worst error / bar {r:.3f}")
    assert r <= 1.0 and not np.array_equal(got, case[2])
    mean_close(st, ref, ids(shape))
    want = adapted(st, L.state0, ref["mean_kl"], prm)
    assert want["coeff"] == (2 * c if want["raised"] == 2 else c / 2), "every case moves the coefficient"


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_equal_rows_give_exactly_zero(shape):
    """q = pi bit for bit: mean_kl and kl_sum are 0.0, dlogits are what they held as numbers (a -0 may come back +0),
    and the adapting coefficient is exactly halved."""
    from freeimpala_amd import kl
    pi, _, d0 = make_case(*shape)
    L = Launch((pi, pi.copy(), d0)).fill(3.0).penalty().finalize(kl.params())
    got, st = L.read()
    L.free()
    assert st["mean_kl"] == 0.0 and st["kl_sum"] == 0.0 and st["rows"] == shape[0] * shape[1]
    assert (got == d0).all()
    assert (st["coeff"], st["lowered"], st["raised"], st["updates"]) == (1.5, 3, 1, 6)


def test_two_launches_return_the_same_bits():
    from freeimpala_amd import kl
    case, prm = make_case(33, 72, 18), kl.params()
    a, b = Launch(case).fill(0.5).penalty().finalize(prm), Launch(case).fill(0.5).penalty().finalize(prm)
    ra, rb = a.raw(), b.raw()
    rc = b.fill(0.5).penalty().finalize(prm).raw()  # and again over its own used workspace
    a.free()
    b.free()
    for k in ("dlogits", "state", "ws"):
        np.testing.assert_array_equal(bits(ra[k]) if k == "dlogits" else ra[k], bits(rb[k]) if k == "dlogits" else rb[k], err_msg=k)
        np.testing.assert_array_equal(rb[k], rc[k], err_msg=k)
    n = 8 * ((33 + 3) // 4) * 2  # nine slices of two column tiles at the most: the partials, then padding nobody wrote
    assert (ra["ws"][n:] == 0xA5).all()


def test_finalize_branches():
    """One penalty launch at (5, 24, 18); its partials then go through every branch, kl_target chosen around the
    reference's mean m. The block's other bytes are compared through adapt_reference on the device's own mean."""
    from freeimpala_amd import kl
    case = make_case(5, 24, 18)
    ref = kl.kl_reference(*case, 1.0)
    m = ref["mean_kl"]
    L = Launch(case).fill(1.0).penalty()

    def run(prm, coeff=1.0, skip=(0, 0)):
        from freeimpala_amd import hip
        L.state0 = dict(STATE0, coeff=float(coeff))
        hip.upload_ptr(L.g.ptr[1], kl.pack_state(**L.state0))
        st = L.finalize(prm, skip).read()[1]
        mean_close(st, ref, "finalize")
        skipped = skip is not None and any(skip)
        want = adapted(st, L.state0, m, prm, skipped)
        assert st == dict(kl.adapt_reference(L.state0, st["mean_kl"], prm, skipped, rows=ref["rows"], kl_sum=st["kl_sum"]))
        return st, want

    up, down, hold = kl.params(kl_target=m / 3), kl.params(kl_target=3 * m), kl.params(kl_target=m)
    assert run(up)[1]["coeff"] == 2.0 and run(up)[0]["raised"] == 2
    assert run(down)[1]["coeff"] == 0.5 and run(down)[0]["lowered"] == 3
    st, _ = run(hold)
    assert (st["coeff"], st["updates"], st["raised"], st["lowered"]) == (1.0, 6, 1, 2)
    assert run(kl.params(kl_target=m / 3, coeff_max=4.0), coeff=3.0)[0]["coeff"] == 4.0, "clamped at coeff_max, and counted"
    assert run(kl.params(kl_target=3 * m, coeff_min=0.75), coeff=1.0)[0]["coeff"] == 0.75
    assert run(kl.params(kl_target=m / 3, adapt=False))[0]["coeff"] == 1.0
    for skip in ((1, 0), (0, 1)):
        st, _ = run(up, skip=skip)
        assert (st["coeff"], st["updates"], st["raised"], st["lowered"]) == (1.0, 5, 1, 2), "skipped: only the mean is written"
    assert run(up, skip=None)[0]["updates"] == 6
    L.free()
    # a NaN logit: the mean is NaN, the coefficient stays, the update counts
    L = Launch(make_case(5, 24, 18, nan=True)).fill(1.0).penalty().finalize(up)
    got, st = L.read()
    L.free()
    assert np.isnan(st["mean_kl"]) and np.isnan(st["kl_sum"]) and st["rows"] == 120
    assert (st["coeff"], st["updates"], st["raised"], st["lowered"]) == (1.0, 6, 1, 2)
    assert np.isnan(got[0, 0]).all() and np.isfinite(got[1:]).all() and np.isfinite(got[0, 1:]).all(), "one row is poisoned"


def test_launcher_refusals():
    """Nothing was launched: the guards and every output are still 0xA5."""
    from freeimpala_amd import kl
    from freeimpala_amd._abi import FiError
    L = Launch(make_case(5, 24, 18))
    for why, kw in (("A = 1", dict(A=1)), ("A = 65", dict(A=65)), ("T = 0", dict(T=0)), ("16-byte", dict(pi=L.inp[0].ptr + 4)),
                    ("16-byte", dict(q=L.inp[1].ptr + 8)), ("16-byte", dict(dlogits=L.g.ptr[0] + 4)),
                    ("8-byte", dict(state=L.g.ptr[1] + 4)), ("null", dict(pi=None)), ("null", dict(q=None)),
                    ("null", dict(dlogits=None)), ("null", dict(state=None)), ("null", dict(ws=None)),
                    ("ws_bytes", dict(ws_bytes=L.ws_bytes - 8))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            L.penalty(**kw)
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))
    nan, inf = float("nan"), float("inf")
    bad = [("reference", dict(reference=2)), ("adapt", dict(adapt=2))]
    bad += [("coeff ", dict(coeff=v)) for v in (-1.0, nan, inf)]
    bad += [("kl_target", dict(kl_target=v)) for v in (0.0, -0.01, nan, inf)]
    bad += [("band", dict(band=v)) for v in (1.0, 0.5, nan)] + [("factor", dict(factor=v)) for v in (1.0, 0.5, nan)]
    bad += [("bounds", kw) for kw in (dict(coeff_min=0.0), dict(coeff_min=2.0, coeff_max=1.0), dict(coeff_max=inf),
                                      dict(coeff_min=nan))]
    for why, kw in bad:
        with pytest.raises(FiError, match=r"rc=-1: .*" + why):
            L.finalize(kl.params(**kw), skip=None)
    for why, kw in (("null", dict(state=None)), ("null", dict(ws=None)), ("ws_bytes", dict(ws_bytes=L.ws_bytes - 8)),
                    ("A = 65", dict(A=65)), ("T = 0", dict(T=0))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            L.finalize(kl.params(), skip=None, **kw)
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))
    with pytest.raises(FiError, match=r"rc=-1: .*null"):
        L.finalize(None, skip=None)
    raw = L.raw()
    L.free()
    assert all((v.view(np.uint8) == 0xA5).all() for v in raw.values()), "nothing was launched"
    assert kl.workspace_bytes(5, 24, 65) == 0


# ------------------------------------------------------------------ 2. on a handle
def kl_block(L):
    from freeimpala_amd import hip
    L.sync()
    return hip.download_ptr(L.kl_state_dev(), np.uint8, (48,))


def step_pair(X, Y, seed):
    """The same synthetic batch on both, one waited step each; the stats without the time."""
    stats = []
    for L in (X, Y):
        L.synth(seed=seed)
        st = L.step_resident()
        st.pop("step_ms")
        stats.append(st)
    return stats


def assert_twins(X, Y):
    for a, b in zip(state_of(X), state_of(Y)):
        np.testing.assert_array_equal(a, b)
    for nm in OUT:
        np.testing.assert_array_equal(bits(X.tensor(nm)), bits(Y.tensor(nm)), err_msg=nm)


@pytest.mark.parametrize("arch", ARCHS)
def test_behaviour_reference_under_vtrace(arch):
    """X with the penalty on mu, Y its twin without: the same parameters and batch, so the same logits, and X's dlogits
    are Y's + c (pi - mu) from kl_reference on the handle's own tensors. The block's mean is the diagnostics' KL(mu || pi),
    which is independent of the new reference. kl_penalty stands directly behind vtrace, kl_adapt behind the optimiser
    and, on the Atari policy, in front of weights_bf16."""
    from freeimpala_amd import kl
    c = 4.0
    X, Y = make_learner(arch), make_learner(arch)
    X.enable_kl_penalty("behaviour", coeff=c)
    X.set_profiling(True)
    sx, sy = step_pair(X, Y, 11)
    T, B, A = X.T, X.B, X.A
    pi = X.tensor("logits", shape=(T + 1, B, A))[:T]
    np.testing.assert_array_equal(bits(pi), bits(Y.tensor("logits", shape=(T + 1, B, A))[:T]))
    ref = kl.kl_reference(pi, X.tensor("mu", shape=(T, B, A)), Y.tensor("dlogits", shape=(T, B, A)), c)
    got = X.tensor("dlogits", shape=(T, B, A))
    r = worst(got, ref["dlogits"])
    print(f"{arch}: dlogits worst error / bar {r:.3f}; mean KL {ref['mean_kl']:.4f}")
    assert r <= 1.0 and worst(got, Y.tensor("dlogits", shape=(T, B, A))) > 100.0, "the penalty is in the gradient"
    for nm in ("vs", "pg_adv", "dvalue"):
        np.testing.assert_array_equal(bits(X.tensor(nm)), bits(Y.tensor(nm)), err_msg=nm)
    for k in ("pg_loss", "baseline_loss", "entropy_loss", "total_loss"):
        assert sx[k] == sy[k], "the penalty is not in fi_step_stats: " + k
    st = X.kl_state()
    assert (st["enabled"], st["reference"], st["adapt"]) == (True, "behaviour", True)
    mean_close(st, ref, arch)
    adapted(st, dict(coeff=c, mean_kl=0.0, kl_sum=0.0, rows=0, updates=0, raised=0, lowered=0), ref["mean_kl"], kl.params())
    assert st["updates"] == 1
    d = X.diagnostics()
    assert d["rows_used"] == d["rows"] == T * B
    err = abs(st["mean_kl"] - d["kl_mu_pi"]) / (TOL * max(1.0, abs(d["kl_mu_pi"])))
    print(f"{arch}: mean_kl {st['mean_kl']!r} against the diagnostics' kl_mu_pi {d['kl_mu_pi']!r}: error / bar {err:.3f}")
    assert err <= 1.0
    tags = kernel_tags(X)
    assert tags[tags.index("vtrace") + 1] == "kl_penalty" and tags.count("kl_penalty") == 1
    assert tags.index("optimizer") < tags.index("kl_adapt")
    assert tags[-2:] == (["kl_adapt", "weights_bf16"] if arch == "atari" else ["optimizer", "kl_adapt"]), tags
    X.close()
    Y.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_target_reference_under_the_surrogate(arch):
    """theta- a fixed perturbation away (test_gpu_target's case, whose clip decisions are safe: asserted): dlogits
    against target_reference's + c (pi - pi_tgt), the mean against kl_reference; kl_penalty stands behind target_stats."""
    from freeimpala_amd import kl, target
    c = 0.5
    L = target_learner(arch, period=1000)
    L.set_target_params(perturbed(L))
    L.enable_kl_penalty("target", coeff=c, kl_target=1e-6)
    L.synth(seed=11)
    L.set_profiling(True)
    L.step_resident()
    case = target_case(L)
    tref = target.target_reference(*case, L.cfg.hp, CLIP, False)
    assert target.near_rows(*case, L.cfg.hp, CLIP, False, ref=tref) == 0, "pick another seed"
    ref = kl.kl_reference(case[0], case[1], tref["dlogits"], c)
    got = learner_outputs(L)
    r = {k: worst(got[k], tref[k]) for k in ("vs", "pg_adv", "dvalue")}
    r["dlogits"] = worst(got["dlogits"], ref["dlogits"])
    print(f"{arch}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; mean KL {ref['mean_kl']:.5f}")
    assert max(r.values()) <= 1.0 and worst(got["dlogits"], tref["dlogits"]) > 1.0, "the penalty is in the gradient"
    st = L.kl_state()
    mean_close(st, ref, arch)
    assert ref["mean_kl"] > 1e-4, "the target differs from the learner"
    adapted(st, dict(coeff=c, mean_kl=0.0, kl_sum=0.0, rows=0, updates=0, raised=0, lowered=0), ref["mean_kl"],
            kl.params(kl_target=1e-6))
    assert (st["coeff"], st["raised"], st["reference"]) == (2 * c, 1, "target")
    tags = kernel_tags(L)
    assert tags[tags.index("target_stats") + 1] == "kl_penalty" and tags.index("optimizer") < tags.index("kl_adapt")
    assert "target_update" not in tags and "vtrace" not in tags
    L.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_period_one_halves_the_coefficient_three_times(arch):
    """period = 1, tau = 1: the target logits are the logits bit for bit (test_gpu_target shows it), so the penalty and
    its mean are exactly 0 and the coefficient goes 1 -> 1/8 in three steps."""
    L = target_learner(arch, period=1)
    L.enable_kl_penalty("target", coeff=1.0)
    L.set_profiling(True)
    for k in range(3):
        L.synth(seed=21 + k)
        L.step_resident()
        np.testing.assert_array_equal(bits(target_logits(L)), bits(L.tensor("logits")).reshape(L.T + 1, L.B, L.A))
    st = L.kl_state()
    assert (st["mean_kl"], st["kl_sum"], st["coeff"], st["lowered"], st["raised"], st["updates"]) == (0.0, 0.0, 0.125, 3, 0, 3)
    tags = kernel_tags(L)
    assert tags[tags.index("target_update") + 1] == "kl_adapt", tags
    L.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_without_the_target_logits_nothing_is_enqueued(arch):
    """Reference target under the V-trace objective, then under the surrogate with the target disabled: no kl_penalty
    or kl_adapt among the tags, the block keeps its bytes, and the steps are bit-equal to a twin's without the penalty."""
    X, Y = target_learner(arch, period=1000, surrogate=False), target_learner(arch, period=1000, surrogate=False)
    X.enable_kl_penalty("target", coeff=2.0)
    blk = kl_block(X)
    for L in (X, Y):
        L.set_profiling(True)
    sx, sy = step_pair(X, Y, 31)
    assert sx == sy
    for L in (X, Y):
        L.set_objective("surrogate", clip=CLIP)
        L.disable_target()
    sx, sy = step_pair(X, Y, 32)
    assert sx == sy
    assert_twins(X, Y)
    tx = kernel_tags(X)
    assert tx == kernel_tags(Y) and "vtrace" in tx and "surrogate_loss" in tx and not [t for t in tx if t.startswith("kl_")]
    np.testing.assert_array_equal(kl_block(X), blk)
    st = X.kl_state()
    assert (st["enabled"], st["coeff"], st["rows"], st["updates"]) == (True, 2.0, 0, 0)
    X.close()
    Y.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_disable_is_the_step_without_the_penalty(arch):
    """X takes a penalised step and disables; Y, which never enabled the penalty, is given X's state. From there their
    steps, parameters, moments, outputs and tag lists are bit-equal twice, and the block keeps its bytes."""
    X, Y = make_learner(arch), make_learner(arch)
    X.enable_kl_penalty("behaviour", coeff=2.0)
    X.synth(seed=41)
    X.step_resident()
    assert X.kl_state()["updates"] == 1
    X.disable_kl_penalty()
    blk = kl_block(X)
    assert X.kl_state()["enabled"] is False
    Y.load_state(X.save_state())
    for L in (X, Y):
        L.set_profiling(True)
    for k in range(2):
        sx, sy = step_pair(X, Y, 42 + k)
        assert sx == sy, k
        assert_twins(X, Y)
    assert kernel_tags(X) == kernel_tags(Y) and not [t for t in kernel_tags(X) if t.startswith("kl_")]
    np.testing.assert_array_equal(kl_block(X), blk)
    X.enable_kl_penalty("behaviour")  # on again, with the coefficient as the first step left it
    assert X.kl_state()["enabled"] is True and X.kl_state()["coeff"] == 4.0
    X.close()
    Y.close()


def test_async_steps_equal_waited_steps():
    """Four steps enqueued without a host wait, the target (period 2) as the reference: the penalty reads the
    coefficient where the finalize of the step before left it, so they equal four waited steps bit for bit, the block
    included -- and the coefficient moved on the way."""
    res = []
    for wait in (True, False):
        L = target_learner("mlp", period=2)
        L.enable_kl_penalty("target", coeff=1.0, kl_target=1e-6)
        for k in range(4):
            L.synth(seed=51 + k)
            assert (L.step_resident(stats=wait) is None) == (not wait)
        L.sync()
        res.append(state_of(L) + [kl_block(L), target_block(L)] + [bits(L.tensor(nm)) for nm in OUT])
        st = L.kl_state()
        print(f"wait {wait}: coeff {st['coeff']}, raised {st['raised']}, lowered {st['lowered']}, mean_kl {st['mean_kl']!r}")
        assert st["updates"] == 4 and st["raised"] + st["lowered"] >= 1, "the coefficient moved on the way"
        L.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_a_rejected_batch_leaves_the_coefficient_alone():
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")
    L.enable_kl_penalty("behaviour", coeff=2.0)
    L.synth(seed=61)
    L.step_resident()
    before, s0 = state_of(L), L.kl_state()
    assert (s0["updates"], s0["raised"], s0["coeff"]) == (1, 1, 4.0)
    good = L.tensor("actions", np.int32)
    bad = good.copy()
    bad[3] = L.A + 2
    L.upload("actions", bad)
    with pytest.raises(FiError, match="rc=-1"):
        L.step_resident()
    for a, b in zip(state_of(L), before):
        np.testing.assert_array_equal(a, b, err_msg="parameters unchanged")
    s1 = L.kl_state()
    assert {k: s1[k] for k in ("coeff", "updates", "raised", "lowered")} == {k: s0[k] for k in ("coeff", "updates", "raised", "lowered")}
    assert s1["rows"] == L.T * L.B, "the mean of the rejected step is still reported"
    L.upload("actions", good)
    L.step_resident()
    s2 = L.kl_state()
    assert (s2["updates"], s2["raised"], s2["coeff"]) == (2, 2, 8.0), "the next good step counts"
    L.close()


def test_column_weights_scale_the_penalty_too():
    """dlogits are w_b times the unweighted penalised step's: one fp32 product each, so the loss is
    sum_b w_b (L_b + c kl_b); the block's mean stays unweighted."""
    rs = np.random.RandomState(5)
    P, Q = make_learner("mlp"), make_learner("mlp")
    w = rs.uniform(0.2, 2.0, P.B).astype(np.float32)
    P.set_column_weights(w)
    for L in (P, Q):
        L.enable_kl_penalty("behaviour", coeff=3.0)
        L.synth(seed=71)
        L.step_resident()
    p, q = learner_outputs(P), learner_outputs(Q)
    np.testing.assert_array_equal(bits(p["dlogits"]), bits(q["dlogits"] * w[None, :, None]))
    np.testing.assert_array_equal(bits(p["dvalue"][:-1]), bits(q["dvalue"][:-1] * w[None, :]))
    assert P.kl_state() == Q.kl_state() and P.kl_state()["mean_kl"] > 1e-4
    P.close()
    Q.close()


def test_set_coeff_and_a_second_enable():
    """set_kl_coeff is ordered behind an enqueued step, which still ran at the old coefficient; a second enable keeps the
    block's coefficient and replaces the parameters."""
    X, Y = make_learner("mlp"), make_learner("mlp")
    for L in (X, Y):
        L.enable_kl_penalty("behaviour", coeff=1.0, adapt=False)
        L.synth(seed=81)
    X.step_resident(stats=False)
    X.set_kl_coeff(0.375)
    Y.step_resident()
    np.testing.assert_array_equal(bits(X.tensor("dlogits")), bits(Y.tensor("dlogits")))
    sx, sy = X.kl_state(), Y.kl_state()
    assert (sx["coeff"], sy["coeff"], sx["updates"], sx["raised"]) == (0.375, 1.0, 1, 0) and sx["mean_kl"] == sy["mean_kl"] > 0
    assert X.kl_state_dev() % 8 == 0
    X.enable_kl_penalty("behaviour", coeff=8.0, kl_target=4.0, adapt=True, band=2.0, factor=4.0, coeff_min=0.25, coeff_max=2.0)
    s = X.kl_state()
    assert (s["coeff"], s["kl_target"], s["adapt"], s["band"], s["factor"], s["coeff_min"], s["coeff_max"]) == \
        (0.375, 4.0, True, 2.0, 4.0, 0.25, 2.0)
    X.synth(seed=82)
    X.step_resident()  # KL(mu || pi) of six actions is below log 6 < 2 = kl_target / band: lowered, and clamped
    s = X.kl_state()
    assert s["mean_kl"] < 1.8 and (s["coeff"], s["lowered"], s["updates"]) == (0.25, 1, 2)
    X.set_kl_coeff(0.0)  # a coefficient of 0 is allowed: the step without a penalty in effect, the mean still measured
    assert X.kl_state()["coeff"] == 0.0
    X.close()
    Y.close()


def _check(rc):
    from freeimpala_amd._abi import check
    check(rc, "call")


def test_refusals():
    from freeimpala_amd import kl
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")

    def refused(match, call, *args, **kw):
        with pytest.raises(FiError, match=match):
            call(*args, **kw)

    for getter in (L.kl_state, L.kl_state_dev):
        refused(r"rc=-4: .*never on", getter)
    refused(r"rc=-4: .*never on", L.set_kl_coeff, 1.0)
    L.disable_kl_penalty()  # nothing to turn off
    nan, inf = float("nan"), float("inf")
    for why, kw in (("coeff ", dict(coeff=-1.0)), ("coeff ", dict(coeff=nan)), ("coeff ", dict(coeff=inf)),
                    ("kl_target", dict(kl_target=0.0)), ("kl_target", dict(kl_target=-1.0)), ("band", dict(band=1.0)),
                    ("factor", dict(factor=1.0)), ("bounds", dict(coeff_min=0.0)), ("bounds", dict(coeff_min=2.0, coeff_max=1.0))):
        refused(r"rc=-1: .*" + why, L.enable_kl_penalty, **kw)
    refused(r"rc=-1: .*reference", lambda: _check(kl.lib().fi_kl_enable(L._h, kl.params(2))))
    refused(r"rc=-1: .*null", lambda: _check(kl.lib().fi_kl_enable(L._h, None)))
    refused(r"rc=-1: .*null", lambda: _check(kl.lib().fi_kl_enable(None, kl.params())))
    with pytest.raises(ValueError):
        L.enable_kl_penalty("mu")
    refused(r"rc=-4: .*fi_target_enable", L.enable_kl_penalty, "target")
    refused(r"rc=-4: .*never on", L.kl_state)  # none of the refused calls made a block
    L.enable_target()
    L.enable_kl_penalty("target")
    s = L.kl_state()
    assert (s["enabled"], s["reference"], s["coeff"], s["rows"], s["updates"], s["raised"], s["lowered"]) == \
        (True, "target", 1.0, 0, 0, 0, 0)
    for c in (-0.5, nan, inf):
        refused(r"rc=-1: .*coeff", L.set_kl_coeff, c)
    refused(r"rc=-1: .*null", lambda: _check(kl.lib().fi_kl_state_dev(L._h, None)))
    assert L.kl_state()["coeff"] == 1.0
    L.close()


EXE = os.path.join(ROOT, "build", "host_kl_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_kl_check"], check=True)
    out = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("kl mlp:")])
    assert len(out[0]) == 1 and " updates 4 " in out[0][0] and out[0][0].endswith("bytes equal")
    assert out[0] == out[1], "two runs print the same bits"
