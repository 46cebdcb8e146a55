"""The UPGO term (include/fi_upgo.h) on the GPU, held against upgo_reference (freeimpala_amd/upgo.py) alone: the scan at
T = 1, on both sides of the 64-step chunk edge, over two and three chunks with carry and over ragged column tiles;
exact ties, a NaN reward and g = 0 on exact inputs; the whole term onto non-zero dlogits with its block; the scan
against V-trace's vs where every link is up; a handle; the refusals.

up_t is a comparison: every random case is built, and then asserted on the fp64 reference, to keep
|r_{t+1} + g_{t+1} V_{t+2} - V_{t+1}| > 1e-3, so fp32 decides every link as fp64 does. The bars are the project's:
TOL = 1e-5 max(1, |ref|) for AU, G and dlogits (tests/test_gpu_surrogate.py's for its scan outputs and dlogits) and for
the block's two sums, which are fp64 sums of fp32 row terms; sum_au is also held to 1e-12 relative against the fp64
sum of the kernel's own AU, which is what the fixed-order fp64 reduction can be asked for. Counts are exact."""
import numpy as np
import pytest

from test_gpu_diag import learner_case, make_learner
from test_gpu_surrogate import bits, ids, state_of, worst
from vtrace_cases import TOL, run_vtrace

pytestmark = pytest.mark.gpu
MARGIN = 1e-3
SCAN_SHAPES = [(1, 1), (2, 8), (5, 24), (33, 72), (63, 5), (64, 67), (65, 65), (129, 3), (200, 136)]
TERM_SHAPES = [(1, 1, 3), (5, 24, 18), (7, 65, 64), (33, 72, 18), (6, 67, 3)]


def scan_case(T, B):
    """randn rewards and values, a tenth of the discounts 0, the rest 0.99; a link within 0.01 of a tie has its reward
    raised by 0.05."""
    rs = np.random.RandomState(1000 * T + B)
    rew, val = rs.randn(T, B).astype(np.float32), rs.randn(T + 1, B).astype(np.float32)
    disc = np.where(rs.rand(T, B) < 0.1, 0.0, 0.99).astype(np.float32)
    gap = rew[1:].astype(np.float64) + disc[1:].astype(np.float64) * val[2:] - val[1:T]
    rew[1:] += np.where(np.abs(gap) < 0.01, 0.05, 0.0).astype(np.float32)
    return rew, disc, val


def term_case(T, B, A):
    """scan_case with logits, behaviour logits half a unit of noise away (rho on both sides of rho_bar = 1), actions and
    the dlogits the term adds onto."""
    rs = np.random.RandomState(77 * T + 5 * B + A)
    pi = rs.randn(T, B, A).astype(np.float32)
    mu = (pi + 0.5 * rs.randn(T, B, A)).astype(np.float32)
    return (pi, mu, rs.randint(0, A, (T, B)).astype(np.int32)) + scan_case(T, B) + (rs.randn(T, B, A).astype(np.float32),)


def run_scan(rew, disc, val):
    from freeimpala_amd import hip, upgo
    T, B = rew.shape
    inp = [hip.DeviceBuffer.from_array(x) for x in (rew, disc, val)]
    out = [hip.DeviceBuffer(4 * T * B), hip.DeviceBuffer(4 * T * B), hip.DeviceBuffer(T * B)]
    upgo.returns_dev(T, B, *(b.ptr for b in inp + out))
    hip.synchronize()
    got = dict(AU=out[0].download(np.float32, (T, B)), G=out[1].download(np.float32, (T, B)),
               up=out[2].download(np.uint8, (T, B)))
    for b in inp + out:
        b.free()
    return got


def run_term(case, coeff=0.75, rho_bar=1.0, runs=1, **over):
    """fi_upgo_term_fp32 `runs` times from the same dlogits: [(dlogits, block bytes, AU from the workspace)]."""
    from freeimpala_amd import hip, upgo
    T, B, A = case[0].shape
    inp = [hip.DeviceBuffer.from_array(x) for x in case[:6]]
    wsb = upgo.workspace_bytes(T, B, A)
    dl, st, ws = hip.DeviceBuffer(case[6].nbytes), hip.DeviceBuffer(upgo.STATE_BYTES), hip.DeviceBuffer(wsb)
    kw = dict(T=T, B=B, A=A, prm=upgo.params(coeff, rho_bar), dlogits=dl.ptr, stats=st.ptr, ws=ws.ptr, ws_bytes=wsb)
    kw.update(zip(("logits", "mu", "actions", "rewards", "discounts", "values"), (b.ptr for b in inp)))
    kw.update(over)
    res = []
    try:
        for _ in range(runs):
            dl.upload(case[6])
            upgo.term_dev(**kw)
            hip.synchronize()
            res.append((dl.download(np.float32, (T, B, A)), st.download(np.uint8, (upgo.STATE_BYTES,)),
                        ws.download(np.float32, (T, B))))
    finally:
        for b in inp + [dl, st, ws]:
            b.free()
    return res


def block_close(st, ref, what):
    """Counts exact; loss_u and sum_au within TOL max(1, |ref|)."""
    assert {k: st[k] for k in ("rows", "links_up", "rows_positive")} == {k: ref[k] for k in ("rows", "links_up", "rows_positive")}
    r = max(abs(st[k] - ref[k]) / (TOL * max(1.0, abs(ref[k]))) for k in ("loss_u", "sum_au"))
    print(f"{what}: loss_u {st['loss_u']!r} ref {ref['loss_u']!r} sum_au {st['sum_au']!r} ref {ref['sum_au']!r}; "
          f"links_up {st['links_up']} of {st['rows']}; worst error / bar {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("shape", SCAN_SHAPES, ids=ids)
def test_scan_matches_reference(shape):
    from freeimpala_amd.upgo import upgo_returns
    case = scan_case(*shape)
    ref = upgo_returns(*case)
    assert ref["margin"] > MARGIN, ref["margin"]
    got = run_scan(*case)
    np.testing.assert_array_equal(got["up"], ref["up"].astype(np.uint8))
    r = {k: worst(got[k], ref[k]) for k in ("AU", "G")}
    print(f"{ids(shape)}: links up {int(ref['up'].sum())} of {ref['up'].size}, margin {ref['margin']:.4f}; worst error / bar {r}")
    assert max(r.values()) <= 1.0


@pytest.mark.parametrize("shape", [(130, 20), (70, 5)], ids=ids)
def test_exact_inputs_give_the_reference_bits(shape):
    """Integer r and V, g in {0, 1/2, 1} with at most eight halves per column: every quantity of the rule is exact in
    fp32 in any association, so G and AU equal the fp64 reference cast to fp32, NaN where it is NaN. Every seventh
    link of a column is an exact tie (up), one reward per column is NaN (the link below it is not up)."""
    from freeimpala_amd.upgo import upgo_returns
    T, B = shape
    rs = np.random.RandomState(T + B)
    rew, val = rs.randint(-2, 3, (T, B)).astype(np.float32), rs.randint(-3, 4, (T + 1, B)).astype(np.float32)
    disc = np.where(rs.rand(T, B) < 0.1, 0.0, 1.0).astype(np.float32)
    for b in range(B):
        disc[rs.choice(T, 8, replace=False), b] = 0.5
        ties = np.arange(1 + b % 7, T - 1, 7)
        disc[ties, b] = 1.0
        rew[ties, b] = val[ties, b] - val[ties + 1, b]
        rew[(11 * b + 9) % T, b] = np.nan
    ref = upgo_returns(rew, disc, val)
    ties = rew[1:] + disc[1:] * val[2:] == val[1:T]
    assert ties.sum() >= B * (T // 7 - 2) and ref["up"][:T - 1][ties].all() and (disc == 0).any()
    assert not ref["up"][:T - 1][np.isnan(rew[1:])].any() and np.isnan(ref["G"]).any()
    got = run_scan(rew, disc, val)
    np.testing.assert_array_equal(got["up"], ref["up"].astype(np.uint8))
    np.testing.assert_array_equal(got["G"], ref["G"].astype(np.float32))
    np.testing.assert_array_equal(got["AU"], ref["AU"].astype(np.float32))


@pytest.mark.parametrize("shape", TERM_SHAPES, ids=ids)
def test_term_matches_reference(shape):
    from freeimpala_amd import upgo
    case = term_case(*shape)
    ref = upgo.upgo_reference(*case[:6], coeff=0.75, rho_bar=1.0)
    assert ref["margin"] > MARGIN and np.abs(ref["AU"]).min() > 1e-5, "pick another seed: a link or an AU's sign is near a tie"
    assert shape[0] * shape[1] < 8 or ((ref["rho"] < 1.0).any() and (ref["rho"] == 1.0).any()), "rho crosses rho_bar"
    (d1, s1, au1), (d2, s2, au2) = run_term(case, runs=2)
    np.testing.assert_array_equal(bits(d1), bits(d2))
    np.testing.assert_array_equal(s1, s2)
    r = dict(dlogits=worst(d1, case[6].astype(np.float64) + ref["dlogits"]), AU=worst(au1, ref["AU"]))
    print(f"{ids(shape)}: worst error / bar {r}")
    assert max(r.values()) <= 1.0
    st = upgo.unpack_state(s1)
    block_close(st, ref, ids(shape))
    own = float(au1.astype(np.float64).sum())
    assert abs(st["sum_au"] - own) <= 1e-12 * abs(own)


def test_all_links_up_is_vtrace_on_policy():
    """pi = mu bit for bit and rewards of 5 and more: every link is up, and AU is vs - V of fi_vtrace_loss_fp32 at
    rho_bar = c_bar = lambda = 1, the n-step return to the bootstrap."""
    T, B, A = 33, 72, 6
    pi, _, act, rew, disc, val, _ = term_case(T, B, A)
    rew = (np.abs(rew) + 5.0).astype(np.float32)
    got = run_scan(rew, disc, val)
    assert got["up"][:T - 1].all() and not got["up"][T - 1].any()
    vt = run_vtrace(pi, pi.copy(), act, rew, disc, val, rho_bar=1.0, c_bar=1.0, lambda_=1.0)
    r = worst(got["AU"], vt["vs"].astype(np.float64) - val[:T])
    print(f"AU against vs - V: worst error / bar {r:.3f}")
    assert r <= 1.0


def stepped(upgo_on, seeds=(7,), wait=True, coeff=0.5, rho_bar=1.0):
    """An MLP handle stepped on synth batches whose rewards are replaced by +-3: against values of a fresh network no
    link is near a tie."""
    L = make_learner("mlp")
    if upgo_on:
        L.enable_upgo(coeff=coeff, rho_bar=rho_bar)
    for s in seeds:
        L.synth(seed=s)
        L.upload("rewards", np.random.RandomState(s).choice([-3.0, 3.0], (L.T, L.B)).astype(np.float32))
        L.step_resident(stats=wait)
    L.sync()
    return L


def test_handle_step_adds_the_reference_term():
    from freeimpala_amd.upgo import upgo_reference
    X, L = stepped(False), stepped(True)
    c = learner_case(L)
    ref = upgo_reference(c["pi"], c["mu"], c["act"], c["rew"], c["disc"], c["val"], coeff=0.5, rho_bar=1.0)
    assert ref["margin"] > MARGIN and 0 < ref["links_up"] < ref["rows"]
    st = L.upgo_state()
    assert (st["enabled"], st["coeff"], st["rho_bar"]) == (True, 0.5, 1.0)
    block_close(st, ref, "handle")
    shape = (L.T, L.B, L.A)
    r = worst(L.tensor("dlogits", shape=shape), X.tensor("dlogits", shape=shape).astype(np.float64) + ref["dlogits"])
    print(f"dlogits against the plain step's plus the reference term: worst error / bar {r:.3f}")
    assert r <= 1.0
    # disabled, L is the handle that never had the term: the same bits from the same state on
    L.disable_upgo()
    X.load_state(L.save_state())
    for Z in (X, L):
        Z.synth(seed=8)
        Z.step_resident()
    for a, b in zip(state_of(X), state_of(L)):
        np.testing.assert_array_equal(a, b)
    X.close()
    L.close()


def test_async_steps_equal_waited_steps():
    from freeimpala_amd import hip
    res = []
    for wait in (True, False):
        L = stepped(True, seeds=(21, 22, 23), wait=wait)
        res.append(state_of(L) + [bits(L.tensor("dlogits")), hip.download_ptr(L.upgo_state_dev(), np.uint8, (40,))])
        L.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("over", [dict(A=1), dict(A=65), dict(T=0), dict(logits=4), dict(values=8), dict(ws=16 + 4), dict(ws_bytes=-1),
                                  dict(coeff=-1.0), dict(coeff=float("nan")), dict(rho_bar=0.0), dict(rho_bar=-2.0)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_refusals(over):
    """FI_ERR_INVALID before any launch: dlogits and the block keep their bytes. Pointer entries are byte offsets
    onto the case's own buffers, ws_bytes = -1 is one byte short."""
    from freeimpala_amd import hip, upgo
    from freeimpala_amd._abi import FiError
    over, case = dict(over), term_case(5, 24, 18)
    T, B, A = case[0].shape
    bufs = {k: hip.DeviceBuffer.from_array(x) for k, x in zip(("logits", "mu", "actions", "rewards", "discounts", "values"), case)}
    wsb = upgo.workspace_bytes(T, B, A)
    bufs.update(dlogits=hip.DeviceBuffer.from_array(case[6]), stats=hip.DeviceBuffer(64), ws=hip.DeviceBuffer(wsb + 64))
    bufs["stats"].zero()
    kw = dict(T=T, B=B, A=A, ws_bytes=wsb, **{k: b.ptr for k, b in bufs.items()})
    prm = {k: over.pop(k) for k in ("coeff", "rho_bar") if k in over}
    for k, v in over.items():
        kw[k] = kw[k] + v if k in bufs or k == "ws_bytes" else v
    with pytest.raises(FiError, match="rc=-1:"):
        upgo.term_dev(prm=upgo.params(**prm), **kw)
    hip.synchronize()
    np.testing.assert_array_equal(bits(bufs["dlogits"].download(np.float32, case[6].shape)), bits(case[6]))
    assert not bufs["stats"].download(np.uint8, (64,)).any()
    for b in bufs.values():
        b.free()


def test_state_before_enable_and_refused_parameters():
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp")
    with pytest.raises(FiError, match="rc=-4:"):
        L.upgo_state()
    for bad in (dict(coeff=-0.5), dict(coeff=float("inf")), dict(rho_bar=0.0), dict(rho_bar=float("nan"))):
        with pytest.raises(FiError, match="rc=-1:"):
            L.enable_upgo(**bad)
    L.close()
