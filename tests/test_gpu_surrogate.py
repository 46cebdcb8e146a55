"""The clipped surrogate objective (include/fi_surrogate.h) on the GPU: the kernels alone between guard
bytes against surrogate_reference and, independently of it, against the oracle's V-trace where the two
rules coincide; the on-policy batch; two launches, the same bits; a bad action; then a handle on both
policies: one step against the reference, set_objective("vtrace") against a twin, asynchronous steps,
rejected batches, the coexistence with column weights, PopArt, a prioritised ring and the diagnostics,
the refusals and the C++ check program.

TOL = 1e-5 max(1, |ref|) for vs, pg_adv, dlogits, dvalue and 1e-5 relative for the loss scalars: the
project's bar for this same fp32 arithmetic against fp64 (tests/test_gpu_vtrace.py, tests/test_gpu_diag.py).
adv_mean and adv_std: 1e-6 relative, fp64 sums of fp32 terms. rows_clipped is exact on inputs without a
row where fp32 may decide the clip the other way (surrogate.near_rows == 0: asserted, the seeds are
chosen for it). Every comparison prints its worst error / bar ratio before it asserts."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_gpu_diag import BARS, TOL as DIAG_TOL, assert_runs_cover_the_pieces, make_learner
from test_gpu_popart import kernel_tags, stat_bars
from test_gpu_prio import ETA, bar as prio_bar
from test_gpu_ring import Guarded, make_entries, spaced
from test_gpu_ring import B as RING_B, T as RING_T, make_learner as ring_learner
from test_gpu_vtrace import TOL, rand_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (9, 200, 5)  # 4 column tiles x 3 slices in the rows and loss kernels, 4 workgroups in the scan
SHAPES = [(1, 1, 3), (1, 8, 2), (5, 24, 18), (33, 72, 18), (7, 65, 64), (20, 136, 6), BIG, (3, 5, 3), (6, 67, 3)]
SEEDS = {(20, 136, 6): 1}  # 1000 T + 10 B + A gives a row within 1e-4 of 1 + clip there
CLIP = 0.2
TAGS = ["surrogate_rows", "surrogate_scan", "surrogate_loss", "surrogate_stats"]
OUT = ("vs", "pg_adv", "dlogits", "dvalue")
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def hp():
    from freeimpala_amd import diag
    return diag.hparams(*BARS)


def orc_hp(**over):
    h = dict(rho_bar=BARS[0], c_bar=BARS[1], pg_rho_bar=BARS[2], lambda_=1.0, baseline_cost=0.5, entropy_cost=0.01)
    h.update(over)
    return h


def make_case(T, B, A, seed=None):
    """rand_case of test_gpu_vtrace.py with mu = pi + 0.5 noise: off-policy enough that the clip bites."""
    pi, noise, act, rew, disc, val = rand_case(SEEDS.get((T, B, A), 1000 * T + 10 * B + A) if seed is None else seed, T, B, A)
    return pi, (pi + np.float32(0.5) * noise).astype(np.float32), act, rew, disc, val


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


class Launch:
    """The inputs in device memory; every output, the stats block, the workspace and the bad word between guards."""
    NAMES = ["vs", "pg_adv", "dlogits", "dvalue", "losses", "stats", "ws", "bad"]

    def __init__(self, case):
        from freeimpala_amd import hip, surrogate
        self.case = [np.ascontiguousarray(x) for x in case]
        self.T, self.B, self.A = case[0].shape
        T, B, A = self.T, self.B, self.A
        self.inp = [hip.DeviceBuffer.from_array(x) for x in self.case]
        self.ws_bytes = surrogate.workspace_bytes(T, B, A)
        assert self.ws_bytes > 0
        self.g = Guarded([(T * B, np.float32), (T * B, np.float32), (T * B * A, np.float32), ((T + 1) * B, np.float32),
                          (3, np.float64), (32, np.uint8), (self.ws_bytes, np.uint8), (1, np.int32)])

    def run(self, clip=CLIP, normalize=False, own_bad=False, losses=True, **over):
        from freeimpala_amd import hip, surrogate
        p = self.g.ptr
        if own_bad:
            hip.upload_ptr(p[7], np.zeros(1, np.int32))
        kw = dict(T=self.T, B=self.B, A=self.A, pi=self.inp[0].ptr, ws_bytes=self.ws_bytes)
        kw.update(over)
        surrogate.surrogate_loss_dev(kw["T"], kw["B"], kw["A"], kw["pi"], *[b.ptr for b in self.inp[1:]], hp(),
                                     surrogate.params(clip, normalize), p[0], p[1], p[2], p[3], p[4] if losses else None, p[5],
                                     p[6], kw["ws_bytes"], p[7] if own_bad else None)
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
        from freeimpala_amd import surrogate
        T, B, A = self.T, self.B, self.A
        o = self.raw()
        return dict(vs=o["vs"].reshape(T, B), pg_adv=o["pg_adv"].reshape(T, B), dlogits=o["dlogits"].reshape(T, B, A),
                    dvalue=o["dvalue"].reshape(T + 1, B), losses=o["losses"], bad=int(o["bad"][0]),
                    **surrogate.unpack_stats(o["stats"]))

    def free(self):
        for b in self.inp:
            b.free()
        self.g.free()


def worst(got, ref, tol=TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / (tol * np.maximum(1.0, np.abs(ref)))).max())


def compare(got, ref, what=""):
    """vs, pg_adv, dlogits, dvalue within TOL, the three losses within 1e-5 relative."""
    r = {k: worst(got[k], ref[k]) for k in OUT}
    r["losses"] = max(abs(g - w) / (TOL * max(1.0, abs(w))) for g, w in zip(got["losses"], ref["losses"]))
    print(f"{what}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0.0 else (0.0 if got == 0.0 else math.inf)


@functools.lru_cache(maxsize=None)
def shape_run(shape, normalize):
    """One launch per shape and setting, shared by the tests below: (case, reference, device result, near rows)."""
    from freeimpala_amd import surrogate
    case = make_case(*shape)
    ref = surrogate.surrogate_reference(*case, hp(), CLIP, normalize)
    L = Launch(case).run(normalize=normalize, own_bad=True)
    got = L.read()
    L.free()
    return case, ref, got, surrogate.near_rows(*case, hp(), CLIP, normalize, ref=ref)


# ------------------------------------------------------------------ 1. the kernels alone
def test_shapes_cover_the_grids():
    from freeimpala_amd import surrogate
    blocks = {s: (surrogate.loss_blocks(*s), surrogate.scan_blocks(s[1])) for s in SHAPES}
    assert min(blocks[BIG]) >= 3, "a shape with three workgroups at least in every kernel"
    assert any(s[1] % 64 != 0 and blocks[s][1] > 1 for s in SHAPES), "a partial column tile behind whole ones"
    assert any(blocks[s][0] > blocks[s][1] for s in SHAPES), "more than one time slice"
    assert any(s[0] % 4 != 0 and s[0] > 4 for s in SHAPES), "a last round with idle waves"
    assert any(s[0] > 8 and s[0] % 8 != 0 for s in SHAPES), "a scan whose last run of eight steps is partial"
    assert_runs_cover_the_pieces(SHAPES)
    assert any(s[2] == 64 for s in SHAPES), "A = 64: the raised LDS limit"


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_match_reference(shape, normalize):
    """The condition: no row where fp32 may decide the clip the other way, and with normalisation s >= 0.5 (A~
    carries A's error divided by s). T * B = 1 with normalisation is the one case that cannot meet it and does
    not need to: A - m is exactly 0 on both sides, so A~ = 0, nothing is clipped and the policy term vanishes."""
    case, ref, got, near = shape_run(shape, normalize)
    n = shape[0] * shape[1]
    if normalize and n == 1:
        assert near == 1 and ref["adv_std"] == 0.0 and (ref["adv_used"] == 0.0).all()
    else:
        assert near == 0, f"pick another seed: {near} rows near a threshold"
        assert not normalize or ref["adv_std"] >= 0.5
    assert (got["rows"], got["rows_clipped"], got["bad"]) == (n, ref["rows_clipped"], 0)
    compare(got, ref, ids(shape))
    assert (got["dvalue"][-1] == 0).all()
    r_m, r_s = rel(got["adv_mean"], ref["adv_mean"]), rel(got["adv_std"], ref["adv_std"])
    print(f"adv_mean {got['adv_mean']!r} ref {ref['adv_mean']!r} ({r_m:.3e}), adv_std {got['adv_std']!r} "
          f"ref {ref['adv_std']!r} ({r_s:.3e}); bar 1e-6")
    assert r_m <= 1e-6 and r_s <= 1e-6
    if n >= 100:
        assert 0 < got["rows_clipped"] < got["rows"], "the clip bites"


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_without_a_clip_it_is_the_oracles_vtrace(orc, shape):
    """Independent of surrogate_reference: clip = 1e30, normalize = 0 against the oracle at pg_rho_bar = 1e30. The
    control: with clip = 0.2 on the same inputs dlogits leaves the oracle's by more than 100 TOL somewhere."""
    case = make_case(*shape)
    o = orc.vtrace_loss(*case, **orc_hp(pg_rho_bar=1e30))
    L = Launch(case).run(clip=1e30)
    got = L.read()
    r = {k: worst(got[k], o[k]) for k in ("vs", "dlogits", "dvalue")}
    print(f"{ids(shape)}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0 and got["rows_clipped"] == 0
    for i in (1, 2):
        assert abs(got["losses"][i] - o["losses"][i]) <= TOL * max(1.0, abs(o["losses"][i]))
    if shape[0] * shape[1] >= 100:
        control = worst(L.run(clip=CLIP).read()["dlogits"], o["dlogits"])
        print(f"control, clip = {CLIP}: {control:.1f} TOL")
        assert control > 100.0
    L.free()


@pytest.mark.parametrize("shape", [(5, 24, 18), (7, 65, 64), BIG], ids=ids)
def test_on_policy_nothing_is_clipped(orc, shape):
    """mu = pi bit for bit: log rho = 0 and rho = 1 exactly, so no row is clipped whatever eps, L_pg is minus the
    fp64 sum of the pg_adv the kernel wrote (to the summation order: 1e-12 of sum |A|), and dlogits is V-trace's."""
    from freeimpala_amd import surrogate
    pi, _, act, rew, disc, val = make_case(*shape)
    case = (pi, pi.copy(), act, rew, disc, val)
    ref = surrogate.surrogate_reference(*case, hp(), CLIP)
    o = orc.vtrace_loss(*case, **orc_hp())
    L = Launch(case)
    for eps in (0.01, 0.2):
        got = L.run(clip=eps).read()
        assert got["rows_clipped"] == 0 and got["rows"] == shape[0] * shape[1]
        a = got["pg_adv"].astype(np.float64)
        assert abs(got["losses"][0] + a.sum()) <= 1e-12 * np.abs(a).sum(), "rho is exactly 1"
        r = dict(pg_adv=worst(got["pg_adv"], ref["pg_adv"]), dlogits=worst(got["dlogits"], o["dlogits"]),
                 vs=worst(got["vs"], o["vs"]), dvalue=worst(got["dvalue"], o["dvalue"]))
        print(f"{ids(shape)} eps {eps}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0
    L.free()


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
def test_two_launches_return_the_same_bits(normalize):
    case = make_case(33, 72, 18)
    a, b = Launch(case).run(normalize=normalize), Launch(case).run(normalize=normalize)
    ra, rb = a.raw(), b.raw()
    rc = b.run(normalize=normalize).raw()  # and again over its own workspace: nothing depends on what it held
    a.free()
    b.free()
    for k in OUT + ("losses", "stats"):
        np.testing.assert_array_equal(bits(ra[k]), bits(rb[k]), err_msg=k)
        np.testing.assert_array_equal(bits(rb[k]), bits(rc[k]), err_msg=k)


def test_an_out_of_range_action_poisons_the_losses():
    pi, mu, act, rew, disc, val = make_case(5, 24, 18)
    bad = act.copy()
    bad[3, 7], bad[0, 23] = 18, -1
    L = Launch((pi, mu, bad, rew, disc, val))
    got = L.run().read()
    assert np.isnan(got["losses"]).all() and np.isfinite(got["dlogits"]).all(), "the rows run on clamped actions"
    got = L.run(own_bad=True).read()
    assert got["bad"] == 2 and np.isnan(got["losses"]).all(), "the caller's word counts them"
    L.free()
    L = Launch((pi, mu, act, rew, disc, val))
    got = L.run(own_bad=True).read()
    assert got["bad"] == 0 and np.isfinite(got["losses"]).all()
    L.free()


def test_launcher_refusals():
    from freeimpala_amd import surrogate
    from freeimpala_amd._abi import FiError
    L = Launch(make_case(5, 24, 18))
    for why, kw in (("A = 1", dict(A=1)), ("A = 65", dict(A=65)), ("16-byte", dict(pi=L.inp[0].ptr + 4)),
                    ("ws_bytes", dict(ws_bytes=L.ws_bytes - 8)), ("T = 0", dict(T=0))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            L.run(**kw)
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))
    for prm in (dict(clip=0.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(clip=-0.1)):
        with pytest.raises(FiError, match=r"rc=-1: .*clip"):
            L.run(**prm)
    raw = L.raw()
    L.free()
    assert all((v.view(np.uint8) == 0xA5).all() for v in raw.values()), "nothing was launched"
    assert surrogate.workspace_bytes(5, 24, 65) == 0


# ------------------------------------------------------------------ 2. on a handle
def learner_case(L):
    T, B, A = L.T, L.B, L.A
    return (L.tensor("logits", shape=(T + 1, B, A))[:T].copy(), L.tensor("mu", shape=(T, B, A)),
            L.tensor("actions", np.int32, (T, B)), L.tensor("rewards", shape=(T, B)), L.tensor("discounts", shape=(T, B)),
            L.tensor("values", shape=(T + 1, B)))


def learner_outputs(L):
    T, B, A = L.T, L.B, L.A
    return dict(vs=L.tensor("vs", shape=(T, B)), pg_adv=L.tensor("pg_adv", shape=(T, B)),
                dlogits=L.tensor("dlogits", shape=(T, B, A)), dvalue=L.tensor("dvalue", shape=(T + 1, B)))


def state_of(L):
    return [bits(L.tensor(nm)) for nm in ("params", "adam_m", "adam_v")]


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("arch", ["mlp", "atari"])
def test_one_step_matches_the_reference(arch, normalize):
    """The handle's own logits, mu, ... fed to surrogate_reference reproduce its vs, pg_adv, dlogits, dvalue and
    fi_step_stats; objective_state() is the reference's; the kernel tags hold the new names and not vtrace."""
    from freeimpala_amd import surrogate
    L = make_learner(arch)
    assert L.objective_state() == dict(objective="vtrace", normalize=False, clip=float(np.float32(0.2)),
                                       adv_eps=float(np.float32(1e-8)), rows=0, rows_clipped=0, adv_mean=0.0, adv_std=0.0)
    L.set_objective("surrogate", clip=CLIP, normalize_advantages=normalize)
    L.synth(seed=11)
    L.set_profiling(True)
    st = L.step_resident()
    case = learner_case(L)
    ref = surrogate.surrogate_reference(*case, L.cfg.hp, CLIP, normalize)
    assert surrogate.near_rows(*case, L.cfg.hp, CLIP, normalize, ref=ref) == 0, "pick another seed"
    assert not normalize or ref["adv_std"] >= 0.5
    got = learner_outputs(L)
    got["losses"] = [st["pg_loss"], st["baseline_loss"], st["entropy_loss"]]
    compare(got, ref, arch)
    total = ref["losses"][0] + L.cfg.hp.baseline_cost * ref["losses"][1] + L.cfg.hp.entropy_cost * ref["losses"][2]
    assert abs(st["total_loss"] - total) <= TOL * max(1.0, abs(total)) and st["grad_norm"] > 0
    s = L.objective_state()
    assert (s["objective"], s["normalize"], s["clip"], s["rows"]) == ("surrogate", normalize, float(np.float32(CLIP)), L.T * L.B)
    assert s["rows_clipped"] == ref["rows_clipped"]
    print(f"{arch}: rows_clipped {s['rows_clipped']} adv_mean {s['adv_mean']!r} ref {ref['adv_mean']!r} "
          f"adv_std {s['adv_std']!r} ref {ref['adv_std']!r}")
    assert rel(s["adv_mean"], ref["adv_mean"]) <= 1e-6 and rel(s["adv_std"], ref["adv_std"]) <= 1e-6
    tags = kernel_tags(L)
    assert [t for t in tags if t.startswith("surrogate")] == TAGS and "vtrace" not in tags and len(tags) > 5
    L.close()


@pytest.mark.parametrize("arch", ["mlp", "atari"])
def test_back_to_vtrace_is_the_plain_step(arch):
    """X takes a surrogate step and goes back; Y, which never enabled anything, is given X's state. From there
    their steps are bit-equal, and so are their tag lists: the surrogate step's, with its four tags folded into
    one, is that same list."""
    X, Y = make_learner(arch), make_learner(arch)
    X.set_objective("surrogate", clip=CLIP, normalize_advantages=True)
    X.synth(seed=21)
    X.set_profiling(True)
    X.step_resident()
    on = kernel_tags(X)
    X.set_profiling(False)
    X.set_objective("vtrace")
    assert X.objective_state()["objective"] == "vtrace" and X.objective_state()["rows"] == X.T * X.B
    Y.load_state(X.save_state())
    for L in (X, Y):
        L.set_profiling(True)
    for k in range(2):
        stats = []
        for L in (X, Y):
            L.synth(seed=22 + k)
            st = L.step_resident()
            st.pop("step_ms")
            stats.append(st)
        assert stats[0] == stats[1], k
    for a, b in zip(state_of(X), state_of(Y)):
        np.testing.assert_array_equal(a, b)
    for nm in OUT:
        np.testing.assert_array_equal(bits(X.tensor(nm)), bits(Y.tensor(nm)), err_msg=nm)
    tx, ty = kernel_tags(X), kernel_tags(Y)
    # set_profiling starts a fresh list: X's holds what it enqueued since it went back
    assert "vtrace" in ty and not [t for t in ty if "surrogate" in t] and tx == ty
    folded = []
    for t in on:
        if t in TAGS:
            if t == TAGS[0]:
                folded.append("vtrace")
        else:
            folded.append(t)
    assert folded == ty
    X.close()
    Y.close()


def test_async_steps_equal_waited_steps():
    """Three steps enqueued without a host wait, normalisation on: the loss kernel reads the moments' partial sums
    where the scan left them, so they equal three waited steps bit for bit, the stats block included."""
    from freeimpala_amd import hip
    res = []
    for wait in (True, False):
        L = make_learner("mlp")
        L.set_objective("surrogate", clip=CLIP, normalize_advantages=True)
        for k in range(3):
            L.synth(seed=31 + k)
            assert (L.step_resident(stats=wait) is None) == (not wait)
        L.sync()
        res.append(state_of(L) + [bits(hip.download_ptr(L.surrogate_stats_ptr(), np.uint8, (32,)).view(np.uint64))] +
                   [bits(L.tensor(nm)) for nm in OUT])
        s = L.objective_state()
        assert s["rows"] == L.T * L.B and 0 < s["rows_clipped"] < s["rows"]
        L.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("what", ["action", "reward"])
def test_rejected_batches(what):
    """A bad action rejects the batch, a NaN reward skips the update: the parameters keep their bits, as on the
    V-trace path; after the NaN reward the stats block reports NaN moments."""
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")
    L.set_objective("surrogate", clip=CLIP, normalize_advantages=True)
    L.synth(seed=41)
    L.step_resident()
    before, s0 = state_of(L), L.objective_state()
    assert math.isfinite(s0["adv_mean"]) and s0["adv_std"] > 0
    good = {nm: L.tensor(nm, dt) for nm, dt in (("actions", np.int32), ("rewards", np.float32))}
    bad = {k: v.copy() for k, v in good.items()}
    if what == "action":
        bad["actions"][3] = L.A + 2
    else:
        bad["rewards"][4] = np.nan
    for nm in bad:
        L.upload(nm, bad[nm])
    with pytest.raises(FiError, match="rc=-1" if what == "action" else "rc=-7"):
        L.step_resident()
    for a, b in zip(state_of(L), before):
        np.testing.assert_array_equal(a, b, err_msg="parameters unchanged")
    s1 = L.objective_state()
    if what == "reward":
        assert math.isnan(s1["adv_mean"]) and math.isnan(s1["adv_std"]) and s1["rows"] == L.T * L.B
    for nm in good:
        L.upload(nm, good[nm])
    L.step_resident()
    assert math.isfinite(L.objective_state()["adv_mean"])
    assert any(not np.array_equal(a, b) for a, b in zip(state_of(L), before)), "the repaired batch updates"
    L.close()


def test_column_weights_scale_the_gradients():
    """dlogits and the first T rows of dvalue are w_b times the unweighted step's: one fp32 product each."""
    rs = np.random.RandomState(5)
    P, Q = make_learner("mlp"), make_learner("mlp")
    w = rs.uniform(0.2, 2.0, P.B).astype(np.float32)
    P.set_column_weights(w)
    for L in (P, Q):
        L.set_objective("surrogate", clip=CLIP)
        L.synth(seed=51)
        L.step_resident()
    p, q = learner_outputs(P), learner_outputs(Q)
    np.testing.assert_array_equal(bits(p["dlogits"]), bits(q["dlogits"] * w[None, :, None]))
    np.testing.assert_array_equal(bits(p["dvalue"][:-1]), bits(q["dvalue"][:-1] * w[None, :]))
    for nm in ("vs", "pg_adv"):
        np.testing.assert_array_equal(bits(p[nm]), bits(q[nm]), err_msg=nm + " stays unweighted")
    assert P.objective_state() == Q.objective_state()
    P.close()
    Q.close()


def test_popart_moves_with_this_steps_targets():
    from freeimpala_amd import popart, surrogate
    MU0, NU0, BETA = 3.0, 9.0 + 6.25, 0.25
    L = make_learner("mlp")
    L.enable_popart(beta=BETA)
    L.set_popart_state(MU0, NU0)
    L.set_objective("surrogate", clip=CLIP)
    L.synth(seed=61)
    L.set_profiling(True)
    L.step_resident()
    tags = kernel_tags(L)
    assert tags[tags.index("surrogate_rows") - 1] == "popart_denorm" and tags[tags.index("surrogate_stats") + 1] == "popart_scale"
    ref = surrogate.surrogate_reference(*learner_case(L), L.cfg.hp, CLIP)  # on the denormalised values it was given
    vs = L.tensor("vs", shape=(L.T, L.B))
    assert worst(vs, ref["vs"]) <= 1.0
    x = vs.astype(np.float64).reshape(-1)
    pr = popart.popart_reference(np.zeros(1), x, np.zeros(1), 0.0, MU0, NU0, BETA)
    got = L.popart_state()
    d_mu, d_nu, d_sg = stat_bars(x, BETA, MU0, NU0, pr)
    ratio = max(abs(got["mu"] - pr["mu"]) / d_mu, abs(got["nu"] - pr["nu"]) / d_nu, abs(got["sigma"] - pr["sigma"]) / d_sg)
    print(f"popart statistics: worst error / bar {ratio:.3f}")
    assert got["updates"] == 1 and ratio <= 1.0 and abs(pr["mu"] - MU0) > 0.01
    # dvalue left the loss kernel as baseline_cost (V - vs) and was divided by sigma_f = 2.5 once: TOL, and
    # 2 u |ref| for the division's rounding and the product's here (test_gpu_popart.py's bar)
    dv, rd = L.tensor("dvalue", shape=(L.T + 1, L.B)).astype(np.float64) * 2.5, ref["dvalue"]
    assert (np.abs(dv - rd) <= TOL * np.maximum(1.0, np.abs(rd)) + 2 * 2.0 ** -24 * np.abs(rd)).all()
    L.close()


def test_a_prioritised_ring_step_refreshes_from_this_steps_targets():
    from freeimpala_amd import surrogate
    from freeimpala_amd.prio import td_priorities
    from freeimpala_amd.ring import EntryRing
    arch, A, T, B = "mlp", 3, RING_T, RING_B
    raw, _ = make_entries(arch, B, A, seed=95)
    R = ring_learner(arch, A)
    R.set_objective("surrogate", clip=CLIP)
    E = R.entry_bytes
    ring = EntryRing(E, 8, seed=4)
    ring.enable_priorities(ETA, 1.0)
    src = spaced(raw, E)
    ring.push(src.ptr, E, B)
    R.step_ring(ring, prioritized=True)
    vs, values = R.tensor("vs").reshape(T, B), R.tensor("values").reshape(T + 1, B)
    ref = surrogate.surrogate_reference(*learner_case(R), R.cfg.hp, CLIP)
    assert worst(vs, ref["vs"]) <= 1.0 and R.objective_state()["rows"] == T * B
    want, got = td_priorities(vs, values, ETA), ring.priorities().astype(np.int64)
    ratio = max(abs(int(g) - int(w)) / prio_bar(int(w), T) for g, w in zip(got, want))
    print(f"priorities: worst error / bar {ratio:.3f}")
    assert ratio <= 1.0
    for h in (ring, R):
        h.close()
    src.free()


def test_diagnostics_are_the_twins():
    """The diagnostics read pi, mu, the batch, V and vs. A V-trace twin of the same parameters on the same batch
    has the same bits in all of them but vs, which the two scans round differently: the summary is equal, and
    within test_gpu_diag's tolerance in the two fields that read vs."""
    X, Y = make_learner("mlp"), make_learner("mlp")
    X.set_objective("surrogate", clip=CLIP, normalize_advantages=True)
    for L in (X, Y):
        L.synth(seed=71)
        L.step_resident()
    dx, dy = X.diagnostics(columns=True), Y.diagnostics(columns=True)
    for k in dy:
        if k in ("mean_abs_td", "explained_variance"):
            assert abs(dx[k] - dy[k]) <= DIAG_TOL * max(1.0, abs(dy[k])), k
        elif k.startswith("col_"):
            np.testing.assert_array_equal(bits(dx[k]), bits(dy[k]), err_msg=k)
        else:
            assert dx[k] == dy[k], (k, dx[k], dy[k])
    assert dy["n_c_clipped"] > 0
    X.close()
    Y.close()


def test_refusals():
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")

    def refused(match, call, *args, **kw):
        with pytest.raises(FiError, match=match):
            call(*args, **kw)

    refused(r"rc=-4: .*never on", L.surrogate_stats_ptr)
    for c in (0.0, -0.2, float("nan"), float("inf")):
        refused(r"rc=-1: .*clip", L.set_objective, "surrogate", clip=c)
    for e in (-1e-8, float("nan"), float("inf")):
        refused(r"rc=-1: .*adv_eps", L.set_objective, "surrogate", adv_eps=e)
    with pytest.raises(ValueError):
        L.set_objective("ppo")
    assert L.objective_state()["objective"] == "vtrace"
    L.set_objective("vtrace")  # nothing to turn off
    L.set_objective("surrogate", clip=0.3, normalize_advantages=True, adv_eps=1e-6)
    assert L.surrogate_stats_ptr() % 8 == 0
    L.set_objective("surrogate", clip=0.1)  # a second call replaces the parameters
    s = L.objective_state()
    assert (s["objective"], s["clip"], s["normalize"], s["adv_eps"]) == ("surrogate", float(np.float32(0.1)), False,
                                                                         float(np.float32(1e-8)))
    L.close()


def test_normalisation_is_refused_on_two_ranks():
    from freeimpala_amd import hip
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import DeviceLearner
    if hip.device_count() < 2:
        pytest.skip("normalisation on a communicator of two ranks: RCCL takes one rank per device, and this machine "
                    "has one device")
    pair = [make_learner("mlp", device=d) for d in (0, 1)]
    DeviceLearner.comm_init_all(pair)
    with pytest.raises(FiError, match=r"rc=-4: .*all-reduce"):
        pair[0].set_objective("surrogate", normalize_advantages=True)
    pair[0].set_objective("surrogate")  # without normalisation any communicator is fine
    for p in pair:
        p.close()


EXE = os.path.join(ROOT, "build", "host_surrogate_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_surrogate_check"], check=True)
    out = []
    for _ in range(2):
        r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("surrogate mlp:")])
    assert len(out[0]) == 1 and "rows 120 " in out[0][0] and out[0][0].endswith("bytes equal")
    assert out[0] == out[1], "two runs print the same bits"
