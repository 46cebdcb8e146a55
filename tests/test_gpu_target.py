"""The target network (include/fi_target.h) on the GPU: the loss kernels alone between guard bytes against
target_reference; their targets bit-equal to fi_surrogate_loss_fp32 on the target logits, and the step with
pi_tgt = pi against the oracle's V-trace, both independent of the new reference; two launches, the same bits; a bad
action; the refusals; the update kernel; then a handle on both policies: one step against the reference, the period
and the copy, the stale target against a twin, disable_target and the V-trace objective against twins, the tags,
asynchronous steps, a rejected batch on a due step, PopArt and column weights, the parameter round trip, the
refusals and the C++ check program.

The bars are the project's own, imported: TOL = 1e-5 max(1, |ref|) for tensors, 1e-5 relative for the loss scalars
(compare), 1e-6 relative for the fp64 moments. mean_log_r and mean_sq_log_r are fp64 sums of fp32 terms that each carry
the tensors' error: TOL. rows_clipped is exact on inputs without a row where fp32 may decide the clip the other way
(target.near_rows == 0: asserted, the seeds are chosen on the CPU for it)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_gpu_diag import BARS, make_learner
from test_gpu_popart import kernel_tags, stat_bars
from test_gpu_ring import Guarded
from test_gpu_surrogate import CLIP, OUT, SHAPES, Launch as SurrogateLaunch, bits, compare, hp, ids, learner_outputs, \
    orc_hp, rel, state_of, worst
from test_gpu_vtrace import TOL, rand_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (T, B, A) -> seed, where 1000 T + 10 B + A leaves a row near a threshold or, on a small shape, no clipped row
SEEDS = {(33, 72, 18): 10, (20, 136, 6): 4, (6, 67, 3): 1}
UPDATE_SIZES = (1, 3, 4, 1027, 65537, 2048 * 256 * 4 + 5)  # the last: past one quad per lane of the largest grid
UNTOUCHED = 0xA5A5A5A5A5A5A5A5  # `updates` of a stats block the loss kernels were given between guards


def make_case(T, B, A, seed=None):
    """rand_case of test_gpu_vtrace.py's pi with tgt = pi + 0.3 noise' and mu = tgt + 0.5 noise."""
    seed = SEEDS.get((T, B, A), 1000 * T + 10 * B + A) if seed is None else seed
    pi, noise, act, rew, disc, val = rand_case(seed, T, B, A)
    noise2 = np.random.RandomState(seed + 7919).randn(T, B, A).astype(np.float32)
    tgt = (pi + np.float32(0.3) * noise2).astype(np.float32)
    return pi, tgt, (tgt + np.float32(0.5) * noise).astype(np.float32), act, rew, disc, val


class Launch:
    """The inputs in device memory; every output, the two blocks, the workspace and the bad word between guards."""
    NAMES = ["vs", "pg_adv", "dlogits", "dvalue", "losses", "sur_stats", "tgt_stats", "ws", "bad"]

    def __init__(self, case):
        from freeimpala_amd import hip, target
        self.case = [np.ascontiguousarray(x) for x in case]
        self.T, self.B, self.A = case[0].shape
        T, B, A = self.T, self.B, self.A
        self.inp = [hip.DeviceBuffer.from_array(x) for x in self.case]
        self.ws_bytes = target.workspace_bytes(T, B, A)
        assert self.ws_bytes > 0
        self.g = Guarded([(T * B, np.float32), (T * B, np.float32), (T * B * A, np.float32), ((T + 1) * B, np.float32),
                          (3, np.float64), (32, np.uint8), (32, np.uint8), (self.ws_bytes, np.uint8), (1, np.int32)])

    def run(self, clip=CLIP, normalize=False, own_bad=False, **over):
        from freeimpala_amd import hip, surrogate, target
        p = self.g.ptr
        if own_bad:
            hip.upload_ptr(p[8], np.zeros(1, np.int32))
        kw = dict(T=self.T, B=self.B, A=self.A, pi=self.inp[0].ptr, tgt=self.inp[1].ptr, ws=p[7], ws_bytes=self.ws_bytes,
                  act=self.inp[3].ptr)
        kw.update(over)
        target.target_loss_dev(kw["T"], kw["B"], kw["A"], kw["pi"], kw["tgt"], self.inp[2].ptr, kw["act"],
                               *[b.ptr for b in self.inp[4:]], hp(), surrogate.params(clip, normalize), p[0], p[1], p[2], p[3],
                               p[4], p[5], p[6], kw["ws"], kw["ws_bytes"], p[8] if own_bad else None)
        return self

    def raw(self):
        """Every output's array, the guards checked, and the inputs bit-unchanged."""
        from freeimpala_amd import hip
        hip.synchronize()
        out = self.g.read(self.NAMES)
        for b, x in zip(self.inp, self.case):
            np.testing.assert_array_equal(b.download(np.uint8, (x.nbytes,)), x.view(np.uint8).reshape(-1), err_msg="an input")
        return out

    def read(self):
        from freeimpala_amd import surrogate, target
        T, B, A = self.T, self.B, self.A
        o = self.raw()
        t = target.unpack_stats(o["tgt_stats"])
        assert t.pop("updates") == UNTOUCHED and t.pop("rows") == T * B, "the loss kernels leave `updates` alone"
        return dict(vs=o["vs"].reshape(T, B), pg_adv=o["pg_adv"].reshape(T, B), dlogits=o["dlogits"].reshape(T, B, A),
                    dvalue=o["dvalue"].reshape(T + 1, B), losses=o["losses"], bad=int(o["bad"][0]),
                    **surrogate.unpack_stats(o["sur_stats"]), **t)

    def free(self):
        for b in self.inp:
            b.free()
        self.g.free()


@functools.lru_cache(maxsize=None)
def shape_run(shape, normalize):
    """One launch per shape and setting, shared by the tests below: (case, reference, device result, near rows)."""
    from freeimpala_amd import target
    case = make_case(*shape)
    ref = target.target_reference(*case, hp(), CLIP, normalize)
    L = Launch(case).run(normalize=normalize, own_bad=True)
    got = L.read()
    L.free()
    return case, ref, got, target.near_rows(*case, hp(), CLIP, normalize, ref=ref)


def moments_close(got, ref, what):
    """mean_log_r, mean_sq_log_r within TOL max(1, |ref|)."""
    r = {k: abs(got[k] - ref[k]) / (TOL * max(1.0, abs(ref[k]))) for k in ("mean_log_r", "mean_sq_log_r")}
    print(f"{what}: mean_log_r {got['mean_log_r']!r} ref {ref['mean_log_r']!r}, mean_sq_log_r {got['mean_sq_log_r']!r} "
          f"ref {ref['mean_sq_log_r']!r}; worst error / bar {max(r.values()):.3f}")
    assert max(r.values()) <= 1.0, r


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_match_reference(shape, normalize):
    """The conditions, on the reference alone: no row where fp32 may decide the clip or the sign of A~ the other way,
    the clip bites and spares (with more than one row), and with normalisation s >= 0.5 (A~ carries A's error divided
    by s). T * B = 1 with normalisation cannot meet them and does not need to: A - m is exactly 0 on both sides."""
    case, ref, got, near = shape_run(shape, normalize)
    n = shape[0] * shape[1]
    if normalize and n == 1:
        assert near == 1 and ref["adv_std"] == 0.0 and (ref["adv_used"] == 0.0).all()
    else:
        assert near == 0, f"pick another seed: {near} rows near a threshold"
        assert not normalize or ref["adv_std"] >= 0.5
        assert n == 1 or 0 < ref["rows_clipped"] < ref["rows"], "pick another seed: the clip bites and spares"
    assert (got["rows"], got["rows_clipped"], got["bad"]) == (n, ref["rows_clipped"], 0)
    compare(got, ref, ids(shape))
    assert (got["dvalue"][-1] == 0).all()
    moments_close(got, ref, ids(shape))
    assert rel(got["adv_mean"], ref["adv_mean"]) <= 1e-6 and rel(got["adv_std"], ref["adv_std"]) <= 1e-6
    assert (ref["beta"] < ref["rho"]).any() or n < 100, "pg_rho_bar bites"


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_targets_are_the_surrogate_kernels_on_the_target_logits(shape, normalize):
    """Independent of target_reference: vs and pg_adv are bit-equal to what fi_surrogate_loss_fp32(pi := tgt, mu, ...)
    writes, and so are the advantage moments and dvalue; dlogits is not (the control)."""
    case, _, got, _ = shape_run(shape, normalize)
    S = SurrogateLaunch(case[1:]).run(normalize=normalize, own_bad=True)
    sur = S.read()
    S.free()
    for k in ("vs", "pg_adv", "dvalue"):
        np.testing.assert_array_equal(bits(got[k]), bits(sur[k]), err_msg=k)
    assert (got["adv_mean"], got["adv_std"], got["losses"][1]) == (sur["adv_mean"], sur["adv_std"], sur["losses"][1])
    assert not np.array_equal(bits(got["dlogits"]), bits(sur["dlogits"]))


@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64), (9, 200, 5)], ids=ids)
def test_with_the_target_equal_to_pi_it_is_the_oracles_vtrace(orc, shape):
    """tgt = pi bit for bit: log r = 0 and r = 1 exactly, so no row is clipped whatever eps and both means are 0.0;
    vs, dlogits and dvalue are the oracle's V-trace at the same hyper-parameters, pg_rho_bar = 2.1 included."""
    pi, _, mu, act, rew, disc, val = make_case(*shape)
    o = orc.vtrace_loss(pi, mu, act, rew, disc, val, **orc_hp())
    L = Launch((pi, pi.copy(), mu, act, rew, disc, val))
    for eps in (0.01, 0.2):
        got = L.run(clip=eps).read()
        assert got["rows_clipped"] == 0 and got["mean_log_r"] == 0.0 and got["mean_sq_log_r"] == 0.0
        r = {k: worst(got[k], o[k]) for k in ("vs", "dlogits", "dvalue")}
        print(f"{ids(shape)} eps {eps}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0
        for i in (1, 2):
            assert abs(got["losses"][i] - o["losses"][i]) <= TOL * max(1.0, abs(o["losses"][i]))
    L.free()


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
def test_two_launches_return_the_same_bits(normalize):
    case = make_case(33, 72, 18)
    a, b = Launch(case).run(normalize=normalize), Launch(case).run(normalize=normalize)
    ra, rb = a.raw(), b.raw()
    rc = b.run(normalize=normalize).raw()  # and again over its own workspace: nothing depends on what it held
    a.free()
    b.free()
    for k in OUT + ("losses", "sur_stats", "tgt_stats"):
        np.testing.assert_array_equal(bits(ra[k]), bits(rb[k]), err_msg=k)
        np.testing.assert_array_equal(bits(rb[k]), bits(rc[k]), err_msg=k)


def test_an_out_of_range_action_poisons_the_losses():
    pi, tgt, mu, act, rew, disc, val = make_case(5, 24, 18)
    bad = act.copy()
    bad[3, 7], bad[0, 23] = 18, -1
    L = Launch((pi, tgt, mu, bad, rew, disc, val))
    got = L.run().read()
    assert np.isnan(got["losses"]).all() and np.isfinite(got["dlogits"]).all(), "the rows run on clamped actions"
    got = L.run(own_bad=True).read()
    assert got["bad"] == 2 and np.isnan(got["losses"]).all(), "each is counted once, in the caller's word"
    L.free()
    L = Launch((pi, tgt, mu, act, rew, disc, val))
    got = L.run(own_bad=True).read()
    assert got["bad"] == 0 and np.isfinite(got["losses"]).all()
    L.free()


def test_launcher_refusals():
    from freeimpala_amd import target
    from freeimpala_amd._abi import FiError
    L = Launch(make_case(5, 24, 18))
    for why, kw in (("A = 1", dict(A=1)), ("A = 65", dict(A=65)), ("16-byte", dict(pi=L.inp[0].ptr + 4)),
                    ("16-byte", dict(tgt=L.inp[1].ptr + 8)), ("ws_bytes", dict(ws_bytes=L.ws_bytes - 8)), ("T = 0", dict(T=0)),
                    ("null", dict(tgt=None)), ("null", dict(ws=None)), ("null", dict(act=None))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            L.run(**kw)
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))
    for prm in (dict(clip=0.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(clip=-0.1)):
        with pytest.raises(FiError, match=r"rc=-1: .*clip"):
            L.run(**prm)
    raw = L.raw()
    L.free()
    assert all((v.view(np.uint8) == 0xA5).all() for v in raw.values()), "nothing was launched"
    assert target.workspace_bytes(5, 24, 65) == 0


@pytest.mark.parametrize("n", UPDATE_SIZES)
def test_update_kernel(n):
    """tau = 1: the source's bits. tau = 0.25: the kernel's float is update_reference's double rounded once, so within
    one ulp (the spacing of floats at the reference's magnitude). A set skip word: the destination keeps its bytes."""
    from freeimpala_amd import hip, target
    rs = np.random.RandomState(n)
    p, t = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    src = hip.DeviceBuffer.from_array(p)
    g = Guarded([(n, np.float32), (2, np.int32)])
    dst, skip = g.ptr

    def run(tau, flags):
        hip.upload_ptr(dst, t)
        hip.upload_ptr(skip, np.array(flags, np.int32))
        target.target_update_dev(src.ptr, dst, n, tau, skip)
        hip.synchronize()
        return g.read(["dst", "skip"])["dst"]

    np.testing.assert_array_equal(bits(run(1.0, (0, 0))), bits(p))
    got, ref = run(0.25, (0, 0)).astype(np.float64), target.update_reference(p, t, 0.25)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"n {n}: worst error {(np.abs(got - ref) / ulp).max():.3f} ulp")
    assert (np.abs(got - ref) <= ulp).all() and not np.array_equal(got, t.astype(np.float64))
    for tau in (1.0, 0.25):
        for flags in ((1, 0), (0, 1)):
            np.testing.assert_array_equal(bits(run(tau, flags)), bits(t), err_msg=f"skipped, tau {tau}")
    hip.upload_ptr(dst, t)
    target.target_update_dev(src.ptr, dst, n, 1.0, None)  # no skip words: always
    hip.synchronize()
    np.testing.assert_array_equal(bits(g.read(["dst", "skip"])["dst"]), bits(p))
    np.testing.assert_array_equal(bits(src.download(np.float32, (n,))), bits(p), err_msg="the source")
    src.free()
    g.free()


def test_update_refusals():
    from freeimpala_amd import hip, target
    from freeimpala_amd._abi import FiError
    a, b = hip.DeviceBuffer(64), hip.DeviceBuffer(64)
    for tau in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(FiError, match=r"rc=-1: .*tau"):
            target.target_update_dev(a.ptr, b.ptr, 4, tau)
    with pytest.raises(FiError, match=r"rc=-1: .*16-byte"):
        target.target_update_dev(a.ptr + 4, b.ptr, 4, 1.0)
    for args in ((None, b.ptr), (a.ptr, None)):
        with pytest.raises(FiError, match=r"rc=-1: .*null"):
            target.target_update_dev(*args, 4, 1.0)
    a.free()
    b.free()


# ------------------------------------------------------------------ 2. on a handle
ARCHS = ["mlp", "atari"]


def target_learner(arch, period=4, tau=1.0, surrogate=True, normalize=False, **kw):
    L = make_learner(arch, **kw)
    if surrogate:
        L.set_objective("surrogate", clip=CLIP, normalize_advantages=normalize)
    L.enable_target(period, tau)
    return L


def target_logits(L):
    from freeimpala_amd import hip
    L.sync()
    return hip.download_ptr(L.target_logits_dev(), np.float32, (L.T + 1, L.B, L.A))


def target_block(L):
    from freeimpala_amd import hip
    L.sync()
    return hip.download_ptr(L.target_stats_dev(), np.uint64, (4,))


def learner_case(L):
    T, B, A = L.T, L.B, L.A
    return (L.tensor("logits", shape=(T + 1, B, A))[:T].copy(), target_logits(L)[:T].copy(), L.tensor("mu", shape=(T, B, A)),
            L.tensor("actions", np.int32, (T, B)), L.tensor("rewards", shape=(T, B)), L.tensor("discounts", shape=(T, B)),
            L.tensor("values", shape=(T + 1, B)))


def perturbed(L, seed=5):
    """The parameters a fixed perturbation away: a theta- whose policy differs from the learner's."""
    p = L.get_params()
    return p + (0.3 * np.abs(p).mean() * np.random.RandomState(seed).randn(p.size)).astype(np.float32)


def tag_counts(L):
    """Launch tag -> how often it was recorded since set_profiling(True), in first-seen order."""
    import ctypes as C
    from freeimpala_amd._abi import lib
    buf = C.create_string_buffer(8192)
    ms, cnt = (C.c_float * 128)(), (C.c_int * 128)()
    n = lib().fi_learner_kernel_times(L._h, buf, 8192, ms, cnt, 128)
    return {nm: cnt[i] for i, nm in enumerate(buf.value.decode().split("\n")[:n])}


TARGET_ONLY = {"target_weights_bf16", "target_forward", "target_weights_back", "target_update"}
FOLD = {"target_loss": "surrogate_loss", "target_stats": "surrogate_stats"}


def full_state(L):
    return state_of(L) + [bits(L.target_params())]


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("arch", ARCHS)
def test_one_step_matches_the_reference(arch, normalize):
    """theta- is set a fixed perturbation away from the parameters, so that pi_tgt differs from pi and the clip can
    bite. The handle's own logits, target logits, mu, ... fed to target_reference reproduce its vs, pg_adv, dlogits,
    dvalue and fi_step_stats; objective_state() and target_state() are the reference's; the tags are the new ones."""
    from freeimpala_amd import target
    L = target_learner(arch, period=1000, normalize=normalize)
    L.set_target_params(perturbed(L))
    L.synth(seed=11)
    L.set_profiling(True)
    st = L.step_resident()
    case = learner_case(L)
    assert not np.array_equal(case[0], case[1])
    ref = target.target_reference(*case, L.cfg.hp, CLIP, normalize)
    assert target.near_rows(*case, L.cfg.hp, CLIP, normalize, ref=ref) == 0, "pick another seed"
    assert not normalize or ref["adv_std"] >= 0.5
    got = learner_outputs(L)
    got["losses"] = [st["pg_loss"], st["baseline_loss"], st["entropy_loss"]]
    compare(got, ref, arch)
    total = ref["losses"][0] + L.cfg.hp.baseline_cost * ref["losses"][1] + L.cfg.hp.entropy_cost * ref["losses"][2]
    assert abs(st["total_loss"] - total) <= TOL * max(1.0, abs(total)) and st["grad_norm"] > 0
    s, t = L.objective_state(), L.target_state()
    print(f"{arch}: rows_clipped {s['rows_clipped']} of {s['rows']} (ref {ref['rows_clipped']})")
    assert (s["objective"], s["rows"], s["rows_clipped"]) == ("surrogate", L.T * L.B, ref["rows_clipped"])
    assert rel(s["adv_mean"], ref["adv_mean"]) <= 1e-6 and rel(s["adv_std"], ref["adv_std"]) <= 1e-6
    assert (t["enabled"], t["period"], t["tau"], t["updates"], t["rows"]) == (True, 1000, 1.0, 0, L.T * L.B)
    moments_close(t, ref, arch)
    assert ref["mean_sq_log_r"] > 1e-4, "the target differs from the learner"
    tags = kernel_tags(L)
    new = [x for x in tags if x.startswith(("target", "surrogate"))]
    fwd = ["target_forward"] if arch == "mlp" else ["target_weights_bf16", "target_forward", "target_weights_back"]
    assert new == fwd + ["surrogate_rows", "surrogate_scan", "target_loss", "target_stats"], tags
    assert "vtrace" not in tags and "target_update" not in tags
    first_fwd = "mlp_fwd_l1" if arch == "mlp" else tags[tags.index("target_weights_back") + 1]
    assert tags.index("target_forward") < tags.index(first_fwd), "the target forward stands in front of the learner's"
    L.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_period_one_is_the_learner_itself(arch):
    """period = 1, tau = 1: in every step theta- is the parameters, so the target logits are the logits bit for bit (on
    the Atari policy: through bf16 images converted from equal floats) and nothing is clipped; after the step theta- is
    the new parameters."""
    L = target_learner(arch, period=1)
    for k in range(3):
        L.synth(seed=21 + k)
        L.step_resident()
        np.testing.assert_array_equal(bits(target_logits(L)), bits(L.tensor("logits")).reshape(L.T + 1, L.B, L.A))
        np.testing.assert_array_equal(bits(L.target_params()), bits(L.tensor("params")))
        t = L.target_state()
        assert (t["updates"], t["mean_log_r"], t["mean_sq_log_r"]) == (k + 1, 0.0, 0.0)
        assert L.objective_state()["rows_clipped"] == 0
    L.close()


def test_period_three_over_seven_steps():
    L = target_learner("mlp", period=3)
    seen, theta = [bits(L.tensor("params"))], []
    for k in range(7):
        L.synth(seed=31 + k)
        L.step_resident()
        seen.append(bits(L.tensor("params")))
        theta.append(bits(L.target_params()))
    assert L.target_state()["updates"] == 2
    for k, due in enumerate((0, 0, 3, 3, 3, 6, 6)):  # after step k + 1: the parameters as read after step `due`
        np.testing.assert_array_equal(theta[k], seen[due], err_msg=f"after step {k + 1}")
    assert not np.array_equal(seen[3], seen[6]) and not np.array_equal(seen[0], seen[3])
    L.close()


def test_tau_moves_a_quarter_of_the_way():
    from freeimpala_amd import target
    L = target_learner("mlp", period=1, tau=0.25)
    before = L.target_params()
    L.synth(seed=41)
    L.step_resident()
    ref = target.update_reference(L.get_params(), before, 0.25)
    got = L.target_params().astype(np.float64)
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all() and L.target_state()["updates"] == 1
    assert not np.array_equal(got, before.astype(np.float64))
    L.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_a_stale_target_leaves_the_learners_forward_alone(arch):
    """period = 1000, two steps at the default rate: in the second theta- is two versions behind, and the logits of that
    step are bit-equal to those of a twin without a target given the same parameters and batch -- the bf16 weight
    images (Atari) and the activations are the learner's again in front of its own forward."""
    X, Y = target_learner(arch, period=1000), make_learner(arch)
    Y.set_objective("surrogate", clip=CLIP)
    X.synth(seed=51)
    X.step_resident()
    Y.load_state(X.save_state())
    for L in (X, Y):
        L.synth(seed=52)
        L.step_resident()
    for nm in ("logits", "values"):
        np.testing.assert_array_equal(bits(X.tensor(nm)), bits(Y.tensor(nm)), err_msg=nm)
    assert not np.array_equal(bits(target_logits(X)).reshape(-1), bits(X.tensor("logits")).reshape(-1))
    assert X.target_state()["mean_sq_log_r"] > 0.0 and X.target_state()["updates"] == 0
    X.close()
    Y.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_disable_target_is_the_plain_surrogate_step(arch):
    """X takes a target step and disables; Y, which never enabled a target, is given X's state. From there their
    steps, parameters, moments and tag lists are bit-equal, and theta- stays where the update left it. The target
    step's own tags, with the target's four taken out and its loss and stats renamed, are Y's tags of one step, name
    by name, in order and as often: no launch of the target forward shows under one of the learner's kernel names."""
    X, Y = target_learner(arch, period=1, normalize=True), make_learner(arch)
    Y.set_objective("surrogate", clip=CLIP, normalize_advantages=True)
    X.synth(seed=61)
    X.set_profiling(True)
    X.step_resident()
    on = {FOLD.get(k, k): v for k, v in tag_counts(X).items() if k not in TARGET_ONLY}
    assert TARGET_ONLY - set(tag_counts(X)) == ({"target_weights_bf16", "target_weights_back"} if arch == "mlp" else set())
    X.set_profiling(False)
    X.disable_target()
    theta = bits(X.target_params())
    assert X.target_state()["enabled"] is False
    Y.load_state(X.save_state())
    for L in (X, Y):
        L.set_profiling(True)
    for k in range(2):
        stats = []
        for L in (X, Y):
            L.synth(seed=62 + k)
            st = L.step_resident()
            st.pop("step_ms")
            stats.append(st)
        assert stats[0] == stats[1], k
    for a, b in zip(state_of(X), state_of(Y)):
        np.testing.assert_array_equal(a, b)
    for nm in OUT:
        np.testing.assert_array_equal(bits(X.tensor(nm)), bits(Y.tensor(nm)), err_msg=nm)
    assert kernel_tags(X) == kernel_tags(Y) and not [t for t in kernel_tags(X) if t.startswith("target")]
    two = tag_counts(Y)  # two steps
    assert tag_counts(X) == two and list(on) == list(two) and {k: 2 * v for k, v in on.items()} == two, (on, two)
    np.testing.assert_array_equal(bits(X.target_params()), theta)
    assert X.target_state()["updates"] == 1
    X.close()
    Y.close()


MLP_BACKWARD = {"mlp_heads_bwd", "mlp_wgrad_heads", "mlp_dgrad_heads", "reduce_slabs", "mlp_wgrad_l2", "mlp_dgrad_l2",
                "mlp_wgrad_l1"}


@pytest.mark.parametrize("arch", ARCHS)
def test_under_the_vtrace_objective_only_the_updates_go_on(arch):
    """Target on, objective "vtrace": bit-equal to a plain twin, no target forward among the tags, `updates` counts.
    The twin never called fi_target_*: its tag list is the one it had before there was a target network -- on the MLP
    the three forward launches, vtrace, the backward's, then allreduce_wait, grad_norm, optimizer; on the Atari policy
    it ends in optimizer, weights_bf16 -- and X's is that list with target_update behind the optimiser."""
    X, Y = target_learner(arch, period=1, surrogate=False), make_learner(arch)
    for L in (X, Y):
        L.set_profiling(True)
    for k in range(2):
        stats = []
        for L in (X, Y):
            L.synth(seed=71 + k)
            st = L.step_resident()
            st.pop("step_ms")
            stats.append(st)
        assert stats[0] == stats[1], k
    for a, b in zip(state_of(X), state_of(Y)):
        np.testing.assert_array_equal(a, b)
    tx, ty = kernel_tags(X), kernel_tags(Y)
    assert not [t for t in ty if "target" in t or "surrogate" in t] and "vtrace" in ty
    if arch == "mlp":
        assert ty[:4] == ["mlp_fwd_l1", "mlp_fwd_l2", "mlp_fwd_heads", "vtrace"]
        assert ty[-3:] == ["allreduce_wait", "grad_norm", "optimizer"] and set(ty[4:-3]) <= MLP_BACKWARD
        assert tx == ty + ["target_update"]
    else:
        assert ty[-4:] == ["allreduce_wait", "grad_norm", "optimizer", "weights_bf16"]
        assert tx == ty[:-1] + ["target_update", "weights_bf16"]
    cx, cy = tag_counts(X), tag_counts(Y)
    assert cx.pop("target_update") == 2 and cx == cy, "every launch of the plain step, as often, and nothing else"
    assert (cy["weights_bf16"] if arch == "atari" else cy["optimizer"]) == 2
    t = X.target_state()
    assert (t["updates"], t["rows"]) == (2, 0), "no target step was taken"
    np.testing.assert_array_equal(bits(X.target_params()), bits(X.tensor("params")))
    X.close()
    Y.close()


def test_async_steps_equal_waited_steps():
    """Four steps enqueued without a host wait, normalisation on, an update behind the second and the fourth (whose
    target is one version behind): bit-equal to four waited steps, theta-, both blocks and the outputs included."""
    res = []
    for wait in (True, False):
        L = target_learner("mlp", period=2, normalize=True)
        for k in range(4):
            L.synth(seed=81 + k)
            assert (L.step_resident(stats=wait) is None) == (not wait)
        L.sync()
        res.append(full_state(L) + [target_block(L), bits(target_logits(L))] + [bits(L.tensor(nm)) for nm in OUT])
        t = L.target_state()
        assert (t["updates"], t["rows"]) == (2, L.T * L.B) and t["mean_sq_log_r"] > 0.0
        assert L.objective_state()["rows"] == L.T * L.B
        L.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_a_rejected_batch_on_a_due_step_leaves_the_target_alone():
    from freeimpala_amd._abi import FiError
    L = target_learner("mlp", period=2)
    L.synth(seed=91)
    L.step_resident()
    before, theta, blk = state_of(L), bits(L.target_params()), target_block(L)
    assert blk[0] == 0
    good = L.tensor("actions", np.int32)
    bad = good.copy()
    bad[3] = L.A + 2
    L.upload("actions", bad)
    with pytest.raises(FiError, match="rc=-1"):
        L.step_resident()  # update number 2: due
    for a, b in zip(state_of(L), before):
        np.testing.assert_array_equal(a, b, err_msg="parameters unchanged")
    np.testing.assert_array_equal(bits(L.target_params()), theta)
    assert L.target_state()["updates"] == 0
    L.upload("actions", good)
    L.step_resident()  # the host corrected its count: this is update number 2 again
    assert L.target_state()["updates"] == 1
    np.testing.assert_array_equal(bits(L.target_params()), bits(L.tensor("params")))
    L.close()


def test_column_weights_scale_the_gradients():
    """dlogits and the first T rows of dvalue are w_b times the unweighted target step's: one fp32 product each."""
    rs = np.random.RandomState(5)
    P, Q = target_learner("mlp", period=1000), target_learner("mlp", period=1000)
    w = rs.uniform(0.2, 2.0, P.B).astype(np.float32)
    P.set_column_weights(w)
    theta = perturbed(P)
    for L in (P, Q):
        L.set_target_params(theta)
        L.synth(seed=101)
        L.step_resident()
    p, q = learner_outputs(P), learner_outputs(Q)
    np.testing.assert_array_equal(bits(p["dlogits"]), bits(q["dlogits"] * w[None, :, None]))
    np.testing.assert_array_equal(bits(p["dvalue"][:-1]), bits(q["dvalue"][:-1] * w[None, :]))
    for nm in ("vs", "pg_adv"):
        np.testing.assert_array_equal(bits(p[nm]), bits(q[nm]), err_msg=nm + " stays unweighted")
    assert P.objective_state() == Q.objective_state() and P.target_state() == Q.target_state()
    assert P.target_state()["mean_sq_log_r"] > 1e-4
    P.close()
    Q.close()


def test_popart_moves_with_this_steps_targets():
    from freeimpala_amd import popart, target
    MU0, NU0, BETA = 3.0, 9.0 + 6.25, 0.25
    L = target_learner("mlp", period=1)
    L.enable_popart(beta=BETA)
    L.set_popart_state(MU0, NU0)
    L.synth(seed=111)
    L.set_profiling(True)
    L.step_resident()
    tags = kernel_tags(L)
    assert tags[tags.index("surrogate_rows") - 1] == "popart_denorm" and tags[tags.index("target_stats") + 1] == "popart_scale"
    assert tags[tags.index("target_update") - 1] == "popart_update"
    ref = target.target_reference(*learner_case(L), L.cfg.hp, CLIP)  # on the denormalised values it was given
    vs = L.tensor("vs", shape=(L.T, L.B))
    assert worst(vs, ref["vs"]) <= 1.0
    x = vs.astype(np.float64).reshape(-1)
    pr = popart.popart_reference(np.zeros(1), x, np.zeros(1), 0.0, MU0, NU0, BETA)
    got = L.popart_state()
    d_mu, d_nu, d_sg = stat_bars(x, BETA, MU0, NU0, pr)
    ratio = max(abs(got["mu"] - pr["mu"]) / d_mu, abs(got["nu"] - pr["nu"]) / d_nu, abs(got["sigma"] - pr["sigma"]) / d_sg)
    print(f"popart statistics: worst error / bar {ratio:.3f}")
    assert got["updates"] == 1 and ratio <= 1.0
    # the update stands behind PopArt's: theta- holds the value head as PopArt rewrote it
    np.testing.assert_array_equal(bits(L.target_params()), bits(L.tensor("params")))
    L.close()


def test_sync_and_the_parameter_round_trip():
    L = target_learner("mlp", period=1000)
    p0 = L.get_params()
    np.testing.assert_array_equal(bits(L.target_params()), bits(p0))  # enable copied the parameters
    L.synth(seed=121)
    L.step_resident()
    assert not np.array_equal(bits(L.get_params()), bits(p0))
    np.testing.assert_array_equal(bits(L.target_params()), bits(p0))
    rs = np.random.RandomState(1)
    q = rs.randn(p0.size).astype(np.float32)
    q[:3] = [np.inf, -0.0, np.float32(1e-45)]  # the bytes travel, whatever they say
    L.set_target_params(q)
    np.testing.assert_array_equal(bits(L.target_params()), bits(q))
    assert L.target_params_dev() % 16 == 0 and L.target_stats_dev() % 8 == 0 and L.target_logits_dev() % 16 == 0
    L.sync_target()
    np.testing.assert_array_equal(bits(L.target_params()), bits(L.get_params()))
    assert L.target_state()["updates"] == 0, "a sync is not counted"
    L.load_state(L.save_state())  # does not touch theta-
    np.testing.assert_array_equal(bits(L.target_params()), bits(L.get_params()))
    L.enable_target(period=7, tau=0.5)  # a second call replaces the numbers and keeps theta-
    t = L.target_state()
    assert (t["period"], t["tau"], t["enabled"]) == (7, 0.5, True)
    L.close()


def test_refusals():
    from freeimpala_amd import target
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")

    def refused(match, call, *args, **kw):
        with pytest.raises(FiError, match=match):
            call(*args, **kw)

    for getter in (L.target_state, L.target_params, L.target_params_dev, L.target_logits_dev, L.target_stats_dev,
                   L.sync_target):
        refused(r"rc=-4: .*never on", getter)
    refused(r"rc=-4: .*never on", L.set_target_params, np.zeros(L.param_count, np.float32))
    L.disable_target()  # nothing to turn off
    refused(r"rc=-1: .*period", L.enable_target, 0)
    for tau in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        refused(r"rc=-1: .*tau", L.enable_target, 4, tau)
    refused(r"rc=-1: .*null", lambda: _check(target.lib().fi_target_enable(L._h, None)))
    refused(r"rc=-1: .*null", lambda: _check(target.lib().fi_target_enable(None, target.params())))
    refused(r"rc=-4: .*never on", L.target_state)  # none of the refused calls made a block
    L.enable_target()
    t = L.target_state()
    assert (t["enabled"], t["period"], t["tau"], t["updates"], t["rows"]) == (True, 4, 1.0, 0, 0)
    refused(r"rc=-1: .*n = ", L.set_target_params, np.zeros(L.param_count - 1, np.float32))
    refused(r"rc=-1: .*null", lambda: _check(target.lib().fi_target_get_params(L._h, None, L.param_count)))
    refused(r"rc=-1: .*null", lambda: _check(target.lib().fi_target_params_dev(L._h, None)))
    L.close()


def _check(rc):
    from freeimpala_amd._abi import check
    check(rc, "call")


EXE = os.path.join(ROOT, "build", "host_target_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_target_check"], check=True)
    out = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("target mlp:")])
    assert len(out[0]) == 1 and "updates 2 " in out[0][0] and out[0][0].endswith("bytes equal")
    assert out[0] == out[1], "two runs print the same bits"
