"""The V-MPO objective (include/fi_vmpo.h) on the GPU: the radix select alone, exact against select_reference; the loss
against vmpo_reference; the temperature's Adam steps against eta_step_reference; two launches, the same bits; then a
handle on both policies: one step against the composition of surrogate_reference's targets and vmpo_reference, back to
V-trace against a twin, asynchronous steps, the target network with the KL penalty, and a rejected batch.

Bars: 1e-5 max(1, |ref|) for the tensors, 1e-5 relative for the losses, 1e-6 relative for S and W. psi's relative error
is about (|x| + 2) 2^-23, under the bar while |x| = |a - Amax| / eta <= 16 on D: asserted on the reference (x_max) before
every comparison. The selection is exact on float32 inputs; on a handle the seeds leave no fp64 advantage within 1e-4
of tau (vmpo.near_tau == 0, asserted)."""
import numpy as np
import pytest

from test_gpu_diag import make_learner
from test_gpu_popart import kernel_tags
from test_gpu_ring import Guarded
from test_gpu_surrogate import CLIP, OUT, bits, compare, hp, ids, learner_case, learner_outputs, rel, state_of, worst
from test_gpu_target import learner_case as target_case, perturbed
from test_gpu_vtrace import TOL, rand_case

pytestmark = pytest.mark.gpu

TAGS = ["surrogate_rows", "surrogate_scan", "vmpo_clear", "vmpo_hist0", "vmpo_hist1", "vmpo_hist2", "vmpo_sums", "vmpo_loss"]


# one lane, one wave, a tail, several workgroups, the second access of a trip, a second trip of the grid-stride loop
SIZES = [1, 2, 64, 65, 1000, 4097, 70001, 300001, 524293]
KINDS = ["normal", "equal", "ties", "exponent", "signs"]


def test_sizes_cover_the_grid():
    from freeimpala_amd import vmpo
    blocks = {n: vmpo.select_blocks(n) for n in SIZES}
    assert blocks[1000] == 1 and 1 < blocks[4097] < blocks[70001] < 256, "one and several workgroups"
    assert blocks[300001] == blocks[524293] == 256, "the grid's cap"
    assert 256 * 1024 < 300001 <= 256 * 2048 < 524293, "the second access of a trip, then a second trip"


def select_data(kind, n, f):
    from freeimpala_amd import vmpo
    rs = np.random.RandomState(n % 1000 + len(kind))
    a = rs.standard_normal(n).astype(np.float32)
    if kind == "equal":
        a[:] = np.float32(-1.25)
    elif kind == "ties":  # one value over the ranks k - 2 .. k + 3
        k, order = vmpo.rank(n, f), np.argsort(-a, kind="stable")
        a[order[max(0, k - 3):k + 3]] = a[order[k - 1]]
    elif kind == "exponent":  # one exponent: the top digit puts every row into four bins
        a = (1.0 + rs.random_sample(n)).astype(np.float32)
    elif kind == "signs":
        a[::7], a[3::7] = np.float32(0.0), np.float32(-0.0)
    return a


@pytest.mark.parametrize("f", [0.5, 1.0, 0.3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_select_is_exact(n, kind, f):
    from freeimpala_amd import hip, vmpo
    a = select_data(kind, n, f)
    ref = vmpo.select_reference(a, f)
    if kind == "ties" and n >= 64 and ref["k"] < n:
        assert ref["selected"] > ref["k"], "the tie group straddles rank k"
    adv = hip.DeviceBuffer.from_array(a)
    g = Guarded([(vmpo.STATE_BYTES, np.uint8), (vmpo.SELECT_WS_BYTES, np.uint8)])
    hip.upload_ptr(g.ptr[0], vmpo.pack_state(eta=1.0))
    vmpo.select_dev(n, adv.ptr, vmpo.params(top_fraction=f), g.ptr[0], g.ptr[1], vmpo.SELECT_WS_BYTES)
    hip.synchronize()
    out = g.read(["state", "ws"])
    adv.free()
    g.free()
    st, key_tau = vmpo.unpack_state(out["state"]), int(out["ws"][24576:].view(np.uint32)[1])
    fbits = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    got = (key_tau, st["selected"], st["rows"], fbits(st["threshold"]), fbits(st["adv_max"]))
    want = (ref["key_tau"], ref["selected"], n, fbits(ref["threshold"]), fbits(ref["adv_max"]))
    assert got == want, (got, want)


SHAPES = [(1, 1, 3), (3, 5, 3), (5, 24, 18), (7, 65, 64), (9, 200, 5)]


def make_case(T, B, A, eta):
    """pi, act, adv, vs, val: adv = 3 eta N(0, 1), so |x| stays near 10 on the better half whatever eta."""
    pi, noise, act, _, _, val = rand_case(1000 * T + 10 * B + A, T, B, A)
    adv = (np.float32(3.0 * eta) * noise[..., 0]).astype(np.float32)
    vs = (val[:T] + np.float32(0.5) * noise[..., 1]).astype(np.float32)
    return pi, act, adv, vs, val


class Launch:
    """The inputs in device memory; every output, the block, the workspace and the bad word between guards."""
    NAMES = ["dlogits", "dvalue", "losses", "state", "ws", "bad"]

    def __init__(self, case, eta=1.0):
        from freeimpala_amd import hip, vmpo
        self.case = [np.ascontiguousarray(x) for x in case]
        self.T, self.B, self.A = case[0].shape
        T, B, A = self.T, self.B, self.A
        self.inp = [hip.DeviceBuffer.from_array(x) for x in self.case]
        self.ws_bytes = vmpo.workspace_bytes(T, B, A)
        self.g = Guarded([(T * B * A, np.float32), ((T + 1) * B, np.float32), (3, np.float64), (vmpo.STATE_BYTES, np.uint8),
                          (self.ws_bytes, np.uint8), (1, np.int32)])
        hip.upload_ptr(self.g.ptr[3], vmpo.pack_state(eta=eta))

    def run(self, prm=None, eta_step=False, skip=None):
        from freeimpala_amd import hip, vmpo
        prm, p = prm or vmpo.params(), self.g.ptr
        pi, act, adv, vs, val = [b.ptr for b in self.inp]
        hip.upload_ptr(p[5], np.zeros(1, np.int32))
        vmpo.select_dev(self.T * self.B, adv, prm, p[3], p[4], self.ws_bytes)
        vmpo.vmpo_loss_dev(self.T, self.B, self.A, pi, act, adv, vs, val, hp(), prm, p[3], p[0], p[1], p[2], p[4],
                           self.ws_bytes, p[5])
        if eta_step:
            vmpo.eta_step_dev(p[3], prm, skip)
        return self

    def raw(self):
        from freeimpala_amd import hip
        hip.synchronize()
        out = self.g.read(self.NAMES)
        return out

    def read(self):
        from freeimpala_amd import vmpo
        T, B, A = self.T, self.B, self.A
        o = self.raw()
        return dict(dlogits=o["dlogits"].reshape(T, B, A), dvalue=o["dvalue"].reshape(T + 1, B), losses=o["losses"],
                    bad=int(o["bad"][0]), **vmpo.unpack_state(o["state"]))

    def free(self):
        for b in self.inp:
            b.free()
        self.g.free()


@pytest.mark.parametrize("eta", [1.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_loss_matches_reference(shape, eta):
    from freeimpala_amd import vmpo
    case = make_case(*shape, eta)
    ref = vmpo.vmpo_reference(*case, hp(), eta)
    assert ref["x_max"] <= 16.0, "the condition the bars hold under"
    L = Launch(case, eta)
    got = L.run().read()
    L.free()
    n = shape[0] * shape[1]
    assert (got["rows"], got["selected"], got["bad"]) == (n, ref["selected"], 0) and ref["selected"] >= max(1, n // 2)
    assert (got["threshold"], got["adv_max"]) == (ref["threshold"], ref["adv_max"]), "float32 inputs: exact"
    r = dict(dlogits=worst(got["dlogits"], ref["dlogits"]), dvalue=worst(got["dvalue"], ref["dvalue"]),
             losses=max(abs(g - w) / (TOL * max(1.0, abs(w))) for g, w in zip(got["losses"], ref["losses"])),
             S=rel(got["sum_e"], ref["sum_e"]) / 1e-6, W=(rel(got["sum_ea"], ref["sum_ea"]) / 1e-6 if n > 1 else 0.0))
    print(f"{ids(shape)} eta {eta}: worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert (got["dvalue"][-1] == 0).all()


def test_three_eta_steps_match_the_reference():
    """Select, loss and the temperature's step three times over one block: d_eta within 1e-5 max(1, the sum of its three
    terms' magnitudes), eta within 1e-5 relative; then the skip word and adapt = 0 leave eta, m1, m2, updates alone."""
    from freeimpala_amd import hip, vmpo
    case, prm = make_case(9, 200, 5, 1.0), vmpo.params(lr_eta=0.05)
    L = Launch(case)
    s = vmpo.unpack_state(vmpo.pack_state(eta=1.0))
    for k in range(3):
        ref = vmpo.vmpo_reference(*case, hp(), s["eta"])
        assert ref["x_max"] <= 16.0
        s = vmpo.eta_step_reference(s, ref["d_eta"], prm)
        got = L.run(prm, eta_step=True).read()
        e_d = abs(got["d_eta"] - ref["d_eta"]) / (TOL * max(1.0, sum(abs(t) for t in ref["d_eta_terms"])))
        e_l = abs(got["loss_eta"] - ref["loss_eta"]) / (TOL * max(1.0, abs(ref["loss_eta"])))
        print(f"step {k}: d_eta {got['d_eta']!r} ref {ref['d_eta']!r} ({e_d:.3f} bar), loss_eta ({e_l:.3f} bar), "
              f"eta {got['eta']!r} ref {s['eta']!r} ({rel(got['eta'], s['eta']):.3e})")
        assert e_d <= 1.0 and e_l <= 1.0 and rel(got["eta"], s["eta"]) <= 1e-5 and got["updates"] == k + 1
    assert s["eta"] != 1.0 and got["m1"] != 0.0
    before = L.raw()["state"][:32].copy()
    skip = hip.DeviceBuffer.from_array(np.array([0, 1], np.int32))
    L.run(prm, eta_step=True, skip=skip.ptr)
    np.testing.assert_array_equal(L.raw()["state"][:32], before, err_msg="the optimiser skipped")
    L.run(vmpo.params(lr_eta=0.05, adapt=False), eta_step=True)
    np.testing.assert_array_equal(L.raw()["state"][:32], before, err_msg="adapt = 0")
    skip.free()
    L.free()


def test_two_launches_return_the_same_bits():
    case = make_case(33, 72, 18, 1.0)
    a, b = Launch(case).run(eta_step=True), Launch(case).run(eta_step=True)
    ra, rb = a.raw(), b.raw()
    a.free()
    b.free()
    for k in ("dlogits", "dvalue", "losses", "state"):
        np.testing.assert_array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8), err_msg=k)


ARCHS = ["mlp", "atari"]
ETA0 = 2.0


def vmpo_block(L):
    from freeimpala_amd import hip
    L.sync()
    return hip.download_ptr(L.vmpo_state_dev(), np.uint8, (88,))


def composition(pi, front_pi, mu, act, rew, disc, val, hp_, eta):
    """surrogate_reference's targets on (front_pi, mu), then vmpo_reference on pi with them; near_tau of the advantages."""
    from freeimpala_amd import surrogate, vmpo
    s = surrogate.surrogate_reference(front_pi, mu, act, rew, disc, val, hp_, CLIP)
    r = vmpo.vmpo_reference(pi, act, s["pg_adv"], s["vs"], val, hp_, eta)
    assert r["x_max"] <= 16.0, r["x_max"]
    return dict(r, vs=s["vs"], pg_adv=s["pg_adv"]), vmpo.near_tau(s["pg_adv"])


@pytest.mark.parametrize("arch", ARCHS)
def test_one_step_matches_the_reference(arch):
    L = make_learner(arch)
    assert L.objective_state()["objective"] == "vtrace" and L.vmpo_state()["enabled"] is False
    L.set_objective("vmpo", eta_init=ETA0)
    assert L.objective_state()["objective"] == "vmpo"
    L.synth(seed=11)
    L.set_profiling(True)
    st = L.step_resident()
    pi, mu, act, rew, disc, val = learner_case(L)
    ref, near = composition(pi, pi, mu, act, rew, disc, val, L.cfg.hp, ETA0)
    assert near == 0, "pick another seed"
    got = learner_outputs(L)
    got["losses"] = [st["pg_loss"], st["baseline_loss"], st["entropy_loss"]]
    compare(got, ref, arch)
    s = L.vmpo_state()
    assert (s["rows"], s["selected"], s["updates"]) == (L.T * L.B, ref["selected"], 1) and s["eta"] != ETA0
    assert abs(s["d_eta"] - ref["d_eta"]) <= TOL * max(1.0, sum(abs(t) for t in ref["d_eta_terms"]))
    tags = kernel_tags(L)
    assert [t for t in tags if t.startswith(("surrogate", "vmpo_")) and t != "vmpo_eta"] == TAGS and "vtrace" not in tags
    assert tags.index("optimizer") < tags.index("vmpo_eta")
    L.set_objective("surrogate", clip=CLIP)
    assert L.objective_state()["objective"] == "surrogate" and L.vmpo_state()["enabled"] is False, "one objective at a time"
    L.set_objective("vmpo")
    assert L.objective_state()["objective"] == "vmpo" and L.vmpo_state()["eta"] == s["eta"], "the block is kept"
    L.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_back_to_vtrace_is_the_plain_step(arch):
    """X takes a V-MPO step and goes back; Y, which never enabled anything, is given X's state. From there their steps,
    parameters, outputs and tag lists are bit-equal."""
    X, Y = make_learner(arch), make_learner(arch)
    X.set_objective("vmpo")
    X.synth(seed=21)
    X.step_resident()
    X.set_objective("vtrace")
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
    for a, b in zip(state_of(X) + [bits(X.tensor(nm)) for nm in OUT], state_of(Y) + [bits(Y.tensor(nm)) for nm in OUT]):
        np.testing.assert_array_equal(a, b)
    assert kernel_tags(X) == kernel_tags(Y) and "vtrace" in kernel_tags(X)
    X.close()
    Y.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_async_steps_equal_waited_steps(arch):
    """Three steps enqueued without a host wait: the weights read eta where the step before left it."""
    res = []
    for wait in (True, False):
        L = make_learner(arch)
        L.set_objective("vmpo", lr_eta=0.05)
        for k in range(3):
            L.synth(seed=31 + k)
            assert (L.step_resident(stats=wait) is None) == (not wait)
        res.append(state_of(L) + [vmpo_block(L)] + [bits(L.tensor(nm)) for nm in OUT])
        s = L.vmpo_state()
        assert s["updates"] == 3 and s["eta"] != 1.0
        L.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("arch", ARCHS)
def test_with_a_target_and_the_kl_penalty(arch):
    """theta- = theta: the step with the target and the penalty equals the step without within the bars, and the penalty
    ran. theta- a perturbation away: vs and pg_adv are the targets on the target logits, not on the learner's."""
    X, Y = make_learner(arch), make_learner(arch)
    X.enable_target(period=2)
    for L in (X, Y):
        L.set_objective("vmpo", eta_init=ETA0)
    X.enable_kl_penalty("target", coeff=0.5)
    for L in (X, Y):
        L.synth(seed=41)
        L.step_resident()
    r = {k: worst(X.tensor(k), Y.tensor(k)) for k in OUT}
    print(f"{arch}: theta- = theta against no target, worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0 and X.kl_state()["rows"] == X.T * X.B
    Y.close()
    X.set_target_params(perturbed(X))
    X.disable_kl_penalty()
    X.synth(seed=42)
    X.set_profiling(True)
    X.step_resident()
    pi, tgt, mu, act, rew, disc, val = target_case(X)
    eta = X.vmpo_state()["eta"]  # what this step left; the step read the one before, a few 1e-3 away
    ref, near = composition(pi, tgt, mu, act, rew, disc, val, X.cfg.hp, eta)
    assert near == 0, "pick another seed"
    got = learner_outputs(X)
    r = {k: worst(got[k], ref[k]) for k in ("vs", "pg_adv", "dvalue")}
    print(f"{arch}: targets on the target logits, worst error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0
    tags = kernel_tags(X)
    assert tags.index("target_forward") < tags.index("surrogate_rows") and X.vmpo_state()["selected"] == ref["selected"]
    X.close()


@pytest.mark.parametrize("arch", ARCHS)
def test_a_rejected_batch_leaves_eta_alone(arch):
    from freeimpala_amd._abi import FiError
    L = make_learner(arch)
    L.set_objective("vmpo", lr_eta=0.05)
    L.synth(seed=61)
    L.step_resident()
    before, blk = state_of(L), vmpo_block(L)[:32].copy()
    good = L.tensor("actions", np.int32)
    bad = good.copy()
    bad[3] = L.A + 2
    L.upload("actions", bad)
    with pytest.raises(FiError, match="rc=-1"):
        L.step_resident()
    for a, b in zip(state_of(L), before):
        np.testing.assert_array_equal(a, b, err_msg="parameters unchanged")
    np.testing.assert_array_equal(vmpo_block(L)[:32], blk, err_msg="eta, m1, m2, updates")
    L.upload("actions", good)
    L.step_resident()
    assert L.vmpo_state()["updates"] == 2, "the next good step counts"
    L.close()
