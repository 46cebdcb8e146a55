"""Off-policy diagnostics on the device (include/fi_diag.h, freeimpala_amd/diag.py): the kernels alone
against the fp64 reference at shapes that cover a partial column tile, several column tiles and
several time slices; skipped rows; the on-policy case, exact; two launches, the same bits; guard
bytes around every output; the launcher's refusals; the handle on an MLP and an Atari learner; the
ordering against later steps; the step itself untouched; and the C++ check program.

The bar for every double and for the column arrays is |d| <= 1e-5 max(1, |ref|), the project's
fp32-kernel-against-fp64 bar (tests/test_gpu_vtrace.py): the rule evaluated per row in fp32 with fp64
sums stays within 1e-6 of the reference on these inputs, which leaves a factor of ten for the device's
exp and log. Counts are exact; a clip count may differ by the number of rows whose rho lies within
1e-4 (relative) of its threshold, and the seeds are chosen so that this number is 0."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 3), (1, 8, 2), (5, 24, 18), (33, 72, 18), (7, 65, 64), (20, 136, 6), (3, 5, 3), (6, 67, 3)]
BARS = (1.3, 0.9, 2.1)  # rho_bar, c_bar, pg_rho_bar: away from the rho = 1 cluster of saturated rows
G = 64                  # guard bytes on both sides of every output
TOL = 1e-5
NEAR = 1e-4
CLIPS = (("n_rho_clipped", 0), ("n_c_clipped", 1), ("n_pg_clipped", 2))
EXACT = ("rows", "rows_used", "rows_bad_action", "rows_nonfinite", "n_episode_ends")


def hp():
    from freeimpala_amd import diag
    return diag.hparams(*BARS)


SEEDS = {(20, 136, 6): 1}  # 1000 T + 10 B + A gives a row within NEAR of c_bar there


def make_case(T, B, A, seed=None):
    rs = np.random.RandomState(SEEDS.get((T, B, A), 1000 * T + 10 * B + A) if seed is None else seed)
    pi = (3 * rs.standard_normal((T, B, A))).astype(np.float32)
    mu = (pi + rs.standard_normal((T, B, A))).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    val, vs, rew = (rs.standard_normal((T, B)).astype(np.float32) for _ in range(3))
    disc = np.where(rs.rand(T, B) < 0.1, 0.0, 0.99).astype(np.float32)
    return dict(pi=pi, mu=mu, act=act, rew=rew, disc=disc, val=val, vs=vs)


INPUTS = ("pi", "mu", "act", "rew", "disc", "val", "vs")


class Launch:
    """The inputs in device memory, every output and the workspace between 0xA5 guards."""

    def __init__(self, case, columns=True):
        from freeimpala_amd import diag, hip
        self.T, self.B, self.A = case["pi"].shape
        self.inp = {k: hip.DeviceBuffer.from_array(case[k]) for k in INPUTS}
        self.ws_bytes = diag.workspace_bytes(self.T, self.B, self.A)
        assert self.ws_bytes > 0
        self.sizes = dict(out=160, col_kl=4 * self.B, col_log_rho=4 * self.B, ws=self.ws_bytes)
        self.out = {}
        for k, nb in self.sizes.items():
            b = hip.DeviceBuffer(nb + 2 * G)
            b.upload(np.full(nb + 2 * G, 0xA5, np.uint8))
            self.out[k] = b
        self.columns = columns

    def ptr(self, k):
        return self.out[k].ptr + G

    def run(self, T=None, B=None, A=None, pi_off=0, ws_bytes=None):
        from freeimpala_amd import diag
        i = self.inp
        diag.offpolicy_diag_dev(self.T if T is None else T, self.B if B is None else B, self.A if A is None else A,
                                i["pi"].ptr + pi_off, i["mu"].ptr, i["act"].ptr, i["rew"].ptr, i["disc"].ptr, i["val"].ptr,
                                i["vs"].ptr, hp(), self.ptr("out"), self.ptr("col_kl") if self.columns else None,
                                self.ptr("col_log_rho") if self.columns else None, self.ptr("ws"),
                                self.ws_bytes if ws_bytes is None else ws_bytes)
        return self

    def raw(self):
        """Every output's bytes, the guards checked."""
        from freeimpala_amd import hip
        hip.synchronize()
        got = {}
        for k, nb in self.sizes.items():
            a = self.out[k].download(np.uint8, (nb + 2 * G,))
            assert (a[:G] == 0xA5).all() and (a[G + nb:] == 0xA5).all(), k + ": guard overwritten"
            got[k] = a[G:G + nb].copy()
        return got

    def read(self):
        from freeimpala_amd import diag
        raw = self.raw()
        d = diag.OffPolicyDiag.from_buffer_copy(raw["out"].tobytes())
        assert d.struct_size == 160 and d.reserved == 0
        return d.as_dict(), raw["col_kl"].view(np.float32), raw["col_log_rho"].view(np.float32)

    def free(self):
        for b in list(self.inp.values()) + list(self.out.values()):
            b.free()


def near_counts(case, bars=BARS):
    """Per threshold, the used rows whose fp64 rho lies within NEAR of it: where fp32 may decide otherwise."""
    pi, mu = case["pi"].astype(np.float64), case["mu"].astype(np.float64)
    A = pi.shape[-1]
    ok = (case["act"] >= 0) & (case["act"] < A) & np.isfinite(pi).all(-1) & np.isfinite(mu).all(-1)
    a = np.where(ok, case["act"], 0)[..., None]

    def lsm(z):
        z = np.where(np.isfinite(z), z, 0.0)
        d = z - z.max(-1, keepdims=True)
        return d - np.log(np.exp(d).sum(-1, keepdims=True))
    rho = np.exp(np.take_along_axis(lsm(pi), a, -1)[..., 0] - np.take_along_axis(lsm(mu), a, -1)[..., 0])
    return [int((ok & (np.abs(rho / b - 1.0) <= NEAR)).sum()) for b in bars]


def compare(got, ref, near=(0, 0, 0)):
    d, ckl, clr = got
    rd, rkl, rlr = ref
    from freeimpala_amd.diag import DOUBLES
    for k in EXACT:
        assert d[k] == rd[k], (k, d[k], rd[k])
    for k, i in CLIPS:
        assert abs(d[k] - rd[k]) <= near[i], (k, d[k], rd[k], near[i])
    for k in DOUBLES:
        print(f"{k}: got {d[k]!r} ref {rd[k]!r}")
        if math.isnan(rd[k]):
            assert math.isnan(d[k]), (k, d[k])
        else:
            assert abs(d[k] - rd[k]) <= TOL * max(1.0, abs(rd[k])), (k, d[k], rd[k])
    for nm, g, r in (("col_kl", ckl, rkl), ("col_log_rho", clr, rlr)):
        assert g.shape == r.shape and g.dtype == np.float32
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=nm)
        m = ~np.isnan(r)
        err = np.abs(g[m].astype(np.float64) - r[m]) / np.maximum(1.0, np.abs(r[m]))
        print(f"{nm}: worst {err.max() if err.size else 0.0:.3g}")
        assert (err <= TOL).all(), (nm, err.max())


@functools.lru_cache(maxsize=None)
def shape_run(shape):
    """One launch per shape, shared by the tests below: (case, reference, device result, near counts)."""
    from freeimpala_amd import diag
    case = make_case(*shape)
    ref = diag.offpolicy_reference(case["pi"], case["mu"], case["act"], case["rew"], case["disc"], case["val"], case["vs"],
                                   hp())
    L = Launch(case).run()
    got = L.read()
    L.free()
    return case, ref, got, near_counts(case)


# ------------------------------------------------------------------ 1. the kernels alone
def run_pieces(shapes):
    """(head, n - head) of the run of every (t, column tile) of every shape: the run starts at float
    g0 = (t B + 64 c) A and has n = nb A floats; its head are the floats in front of the first 16-byte boundary."""
    for T, B, A in shapes:
        for t in range(T):
            for b0 in range(0, B, 64):
                g0, n = (t * B + b0) * A, min(64, B - b0) * A
                head = min(-g0 % 4, n)
                yield head, n - head


def assert_runs_cover_the_pieces(shapes):
    pieces = set(run_pieces(shapes))
    for h in (1, 2, 3):
        assert any(head == h for head, _ in pieces), f"a run that starts {h} floats in front of a 16-byte boundary"
    assert any(head and rest >= 4 and rest % 4 for head, rest in pieces), "a run with a head, 16-byte pieces and a tail"
    assert any(rest < 4 for _, rest in pieces), "a run without a 16-byte piece"


def test_shapes_cover_the_plan():
    from freeimpala_amd import diag
    plans = {s: diag.plan(*s) for s in SHAPES}
    assert any(s[1] % 64 != 0 and plans[s][0] == (s[1] + 63) // 64 for s in SHAPES), "a partial column tile"
    assert any(s[1] % 64 != 0 and plans[s][0] > 1 for s in SHAPES), "a partial tile behind whole ones"
    assert any(p[0] > 1 for p in plans.values()), "more than one column tile"
    assert any(p[1] > 1 for p in plans.values()), "more than one time slice"
    assert any(p[0] > 1 and p[1] > 1 for p in plans.values())
    assert_runs_cover_the_pieces(SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_reference(shape):
    case, ref, got, near = shape_run(shape)
    assert near == [0, 0, 0], f"pick another seed: rows within {NEAR} of a threshold {near}"
    assert ref[0]["rows_used"] == shape[0] * shape[1]
    compare(got, ref, near)
    if shape[0] * shape[1] >= 100:  # the thresholds bite: the counts are not trivially equal
        assert 0 < ref[0]["n_pg_clipped"] < ref[0]["n_rho_clipped"] < ref[0]["n_c_clipped"] < ref[0]["rows_used"]
        assert 0 < ref[0]["n_episode_ends"] < ref[0]["rows"] and 0 < ref[0]["ess"] < 1


def test_skipped_rows():
    from freeimpala_amd import diag
    T, B, A = 5, 24, 18
    case = make_case(T, B, A, seed=77)
    case["act"][0, 0], case["act"][4, 23] = -1, A
    case["pi"][1, 5, 17] = np.nan
    case["mu"][2, 9, 0] = np.inf
    case["pi"][0, 0, 3] = np.nan      # behind a bad action: still counted as a bad action
    case["act"][:, 7] = A + 1         # one whole column
    case["mu"][3, 7, 2] = -np.inf
    ref = diag.offpolicy_reference(case["pi"], case["mu"], case["act"], case["rew"], case["disc"], case["val"], case["vs"],
                                   hp())
    assert ref[0]["rows_bad_action"] == 2 + T and ref[0]["rows_nonfinite"] == 2 and ref[0]["rows_used"] == T * B - 4 - T
    near = near_counts(case)
    assert near == [0, 0, 0]
    L = Launch(case).run()
    got = L.read()
    L.free()
    compare(got, ref, near)
    assert np.isnan(got[1][7]) and np.isnan(got[2][7])
    assert np.isfinite(np.delete(got[1], 7)).all() and np.isfinite(np.delete(got[2], 7)).all()
    assert all(math.isfinite(got[0][k]) for k in diag.DOUBLES)


def test_every_row_skipped_is_nan():
    from freeimpala_amd import diag
    case = make_case(3, 9, 4, seed=5)
    case["act"][:] = 4
    L = Launch(case).run()
    d, ckl, clr = L.read()
    L.free()
    assert d["rows"] == 27 and d["rows_used"] == 0 and d["rows_bad_action"] == 27 and d["rows_nonfinite"] == 0
    assert d["n_episode_ends"] == int((case["disc"] == 0).sum())
    assert all(math.isnan(d[k]) for k in diag.DOUBLES) and np.isnan(ckl).all() and np.isnan(clr).all()


def test_on_policy_is_exact():
    case = dict(make_case(33, 72, 18))
    case["mu"] = case["pi"].copy()
    L = Launch(case)
    # the default thresholds: the strict tests report nothing at rho == 1
    from freeimpala_amd import diag
    i = L.inp
    diag.offpolicy_diag_dev(33, 72, 18, i["pi"].ptr, i["mu"].ptr, i["act"].ptr, i["rew"].ptr, i["disc"].ptr, i["val"].ptr,
                            i["vs"].ptr, diag.hparams(), L.ptr("out"), L.ptr("col_kl"), L.ptr("col_log_rho"), L.ptr("ws"),
                            L.ws_bytes)
    d, ckl, clr = L.read()
    L.free()
    assert d["rows_used"] == 33 * 72
    assert d["mean_log_rho"] == 0.0 and d["kl_mu_pi"] == 0.0
    assert d["n_rho_clipped"] == d["n_c_clipped"] == d["n_pg_clipped"] == 0
    assert d["max_rho"] == 1.0 and d["min_rho"] == 1.0 and d["ess"] == 1.0 and d["mean_rho"] == 1.0
    assert d["entropy_pi"] == d["entropy_mu"] > 0
    assert (ckl == 0).all() and (clr == 0).all()


def test_two_launches_return_the_same_bits():
    case = shape_run((33, 72, 18))[0]
    a, b = Launch(case).run(), Launch(case).run()
    ra, rb = a.raw(), b.raw()
    b.run()  # and again over its own workspace: nothing depends on what the workspace held
    rc = b.raw()
    a.free()
    b.free()
    for k in ("out", "col_kl", "col_log_rho"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
        np.testing.assert_array_equal(rb[k], rc[k], err_msg=k)


def test_null_column_pointers_write_nothing():
    case, ref, got, _ = shape_run((20, 136, 6))
    L = Launch(case, columns=False).run()
    raw = L.raw()
    L.free()
    assert (raw["col_kl"] == 0xA5).all() and (raw["col_log_rho"] == 0xA5).all()
    from freeimpala_amd import diag
    d = diag.OffPolicyDiag.from_buffer_copy(raw["out"].tobytes()).as_dict()
    assert d == got[0], "the summary does not depend on the column outputs"


def test_launcher_refusals():
    from freeimpala_amd._abi import FiError
    case = shape_run((5, 24, 18))[0]
    L = Launch(case)
    for why, kw in (("A = 1", dict(A=1)), ("A = 65", dict(A=65)), ("16-byte", dict(pi_off=4)),
                    ("ws_bytes", dict(ws_bytes=L.ws_bytes - 8)), ("T = 0", dict(T=0))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            L.run(**kw)
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))
    raw = L.raw()
    L.free()
    assert all((v == 0xA5).all() for v in raw.values()), "nothing was launched"


# ------------------------------------------------------------------ 2. the handle
def make_learner(arch, **kw):
    from freeimpala_amd.learner import DeviceLearner
    kw.setdefault("seed", 3)
    kw.setdefault("lr", 1e-3)
    return DeviceLearner(arch, seq_len=5, batch=16, num_actions=6 if arch == "mlp" else 18, obs_dim=128, hidden=256,
                         rho_bar=BARS[0], c_bar=BARS[1], pg_rho_bar=BARS[2], **kw)


def learner_case(L):
    T, B, A = L.T, L.B, L.A
    return dict(pi=L.tensor("logits", shape=(T + 1, B, A))[:T].copy(), mu=L.tensor("mu", shape=(T, B, A)),
                act=L.tensor("actions", np.int32, (T, B)), rew=L.tensor("rewards", shape=(T, B)),
                disc=L.tensor("discounts", shape=(T, B)), val=L.tensor("values", shape=(T + 1, B)),
                vs=L.tensor("vs", shape=(T, B)))


def learner_reference(L):
    from freeimpala_amd import diag
    c = learner_case(L)
    ref = diag.offpolicy_reference(c["pi"], c["mu"], c["act"], c["rew"], c["disc"], c["val"], c["vs"], L.cfg.hp)
    return ref, near_counts(c, (L.cfg.hp.rho_bar, L.cfg.hp.c_bar, L.cfg.hp.pg_rho_bar))


@pytest.mark.parametrize("arch", ["mlp", "atari"])
def test_handle_matches_reference(arch):
    from freeimpala_amd import diag
    from freeimpala_amd._abi import FiError
    L = make_learner(arch)
    with pytest.raises(FiError, match=r"rc=-4\b"):
        L.diagnostics()            # no step has run
    with pytest.raises(FiError, match=r"rc=-4\b"):
        L.enqueue_diagnostics()
    L.synth(seed=11)
    L.step_resident()
    with pytest.raises(FiError, match=r"rc=-4\b"):
        L.read_diagnostics()       # nothing was enqueued
    d = L.diagnostics(columns=True)
    ref, near = learner_reference(L)
    assert ref[0]["rows_used"] == L.T * L.B
    compare(({k: v for k, v in d.items() if not k.startswith("col_")}, d["col_kl"], d["col_log_rho"]), ref, near)
    assert (L.cfg.hp.rho_bar, L.cfg.hp.c_bar, L.cfg.hp.pg_rho_bar) == tuple(np.float32(b) for b in BARS)
    assert d["n_c_clipped"] >= d["n_rho_clipped"] >= d["n_pg_clipped"], "the handle's thresholds, 0.9 < 1.3 < 2.1"
    assert d["n_c_clipped"] > d["n_pg_clipped"]
    # read again: the same result, and without the columns
    again = L.read_diagnostics()
    assert again == {k: v for k, v in d.items() if not k.startswith("col_")}
    # column pointers with another count than B are refused
    buf, st = np.empty(L.B + 1, np.float32), diag.OffPolicyDiag()
    assert diag.lib().fi_diag_read(L._h, ctypes.byref(st), buf.ctypes.data, None, L.B + 1) == -1
    L.close()


def test_result_is_ordered_before_later_steps():
    X, Y = make_learner("mlp"), make_learner("mlp")
    X.synth(seed=1)
    X.step_resident(stats=False)
    X.enqueue_diagnostics()
    X.synth(seed=2)
    X.step_resident(stats=False)
    d = X.read_diagnostics(columns=True)
    Y.synth(seed=1)
    Y.step_resident(stats=False)
    ref, near = learner_reference(Y)
    compare(({k: v for k, v in d.items() if not k.startswith("col_")}, d["col_kl"], d["col_log_rho"]), ref, near)
    later, _ = learner_reference(X)  # X's tensors now hold the second step
    assert later[0]["mean_reward"] != ref[0]["mean_reward"] and later[0]["kl_mu_pi"] != ref[0]["kl_mu_pi"]
    X.close()
    Y.close()


def test_the_step_is_untouched():
    P, Q = make_learner("mlp"), make_learner("mlp")
    for k in range(3):
        for L in (P, Q):
            L.synth(seed=20 + k)
        sp, sq = P.step_resident(), Q.step_resident()
        Q.diagnostics(columns=True)
        sp.pop("step_ms"), sq.pop("step_ms")
        assert sp == sq, k
    for name in ("params", "adam_m", "adam_v"):
        np.testing.assert_array_equal(P.tensor(name).view(np.uint32), Q.tensor(name).view(np.uint32), err_msg=name)
    P.close()
    Q.close()


# ------------------------------------------------------------------ 3. C++ wrapper
EXE = os.path.join(ROOT, "build", "host_diag_check")


def test_cpp_check_program():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_diag_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("diag mlp:")]
    assert len(lines) == 1 and "on-policy kl 0 " in lines[0]
