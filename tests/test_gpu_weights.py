"""Per-column loss weights and prioritised replay's exponents (include/fi_weights.h): the three
standalone kernels against the host rule (freeimpala_amd/weights.py), a learner whose prioritised
steps weigh their replayed columns against one fed the same entries and weights from the host, the
linearity of the step in the weights, the defaults that move nothing, and the refusals.

The scale is one fp32 multiply and compared exactly. A priority with the exponent alpha is compared
with the fp64 rule within 1 + q (T + 6 + 32) 2^-24: test_gpu_prio.py's bound plus 16 ulp = 32 * 2^-24
for powf, the OpenCL bound OCML implements; alpha <= 1 does not amplify the relative error of p. An
importance weight is compared within rtol 1e-5, the project's fp32 parity bound, above the derived
2 (32 + 2) 2^-24 = 4.1e-6: a cast, powf and a divide for both u and the maximum m."""
import numpy as np
import pytest

from test_gpu_ring import B, T, Guarded, learner_pair, make_entries, make_learner, same, snapshot, spaced

pytestmark = pytest.mark.gpu

Q_MAX = 2 ** 31 - 1
ETA = 0.9
RTOL = 1e-5


def bar(q_ref, t):
    return 1 + q_ref * (t + 6 + 32) * 2.0 ** -24


# ------------------------------------------------------------------ 1. the scale kernel alone
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 3), (2, 5, 18), (7, 67, 18)])
@pytest.mark.parametrize("dvalue_offset", [0, 1])  # floats behind a 16-byte boundary: the head piece
def test_scale_kernel_is_one_multiply_per_float(shape, dvalue_offset):
    from freeimpala_amd import hip, weights
    Tc, Bc, A = shape
    rs = np.random.RandomState(Tc * 10000 + Bc * 100 + A)
    dlog = rs.standard_normal((Tc, Bc, A)).astype(np.float32)
    dval = rs.standard_normal((Tc + 1, Bc)).astype(np.float32)
    w = rs.uniform(0.0, 2.0, Bc).astype(np.float32)
    w[0] = 0.0 if Bc > 1 else 0.75
    w[Bc // 2] = 1.0 if Bc > 1 else w[0]
    if Bc > 2:
        dlog[0, 2, 0], dval[0, 0] = -0.0, np.inf  # Inf * 0 = NaN on both sides
    out = Guarded([(dlog.size, np.float32), (dval.size + dvalue_offset, np.float32)])
    dw = hip.DeviceBuffer.from_array(w)
    hip.upload_ptr(out.ptr[0], dlog)
    hip.upload_ptr(out.ptr[1] + 4 * dvalue_offset, dval)
    weights.scale_columns(out.ptr[0], out.ptr[1] + 4 * dvalue_offset, dw.ptr, Tc, Bc, A)
    hip.synchronize()
    got = out.read(("dlogits", "dvalue"))
    out.free()
    dw.free()
    np.testing.assert_array_equal(got["dlogits"].reshape(Tc, Bc, A), dlog * w[None, :, None])
    if dvalue_offset:
        assert got["dvalue"][:1].view(np.uint8).tolist() == [0xA5] * 4, "the float in front of dvalue"
    gv = got["dvalue"][dvalue_offset:].reshape(Tc + 1, Bc)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(gv[:Tc], dval[:Tc] * w[None, :])
    np.testing.assert_array_equal(gv[Tc], dval[Tc], err_msg="row T of dvalue is not touched")
    if Bc > 1:
        assert not got["dlogits"].reshape(Tc, Bc, A)[:, 0].any() and (gv[:Tc, Bc // 2] == dval[:Tc, Bc // 2]).all()


# ------------------------------------------------------------------ 2. alpha
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (100, 70)])
def test_from_td_alpha_equals_the_fp64_rule(shape):
    """The inputs of test_gpu_prio.py::test_from_td_equals_the_fp64_rule."""
    from freeimpala_amd import hip, prio, weights
    Tc, Bc = shape
    rs = np.random.RandomState(Tc * 1000 + Bc)
    scale = (10.0 ** rs.uniform(-6, 2, Bc)).astype(np.float32)  # columns of very different magnitude
    values = (rs.standard_normal((Tc + 1, Bc)) * scale).astype(np.float32)
    vs = (values[:Tc] + rs.standard_normal((Tc, Bc)) * scale).astype(np.float32)
    if Bc >= 5:
        vs[:, 0] = values[:Tc, 0]  # p = 0
        vs[Tc // 2, 1] = np.nan
        vs[Tc - 1, 2] = np.inf
        vs[:, 3] = values[:Tc, 3] + np.float32(1e6)  # p above the table's range, p^0.6 inside it
    dv, dval = hip.DeviceBuffer.from_array(vs), hip.DeviceBuffer.from_array(values)

    def run(call, *args):
        out = Guarded([(Bc, np.uint32)])
        call(dv.ptr, dval.ptr, Tc, Bc, *args, out.ptr[0])
        hip.synchronize()
        got = out.read(("q",))["q"].astype(np.int64)
        out.free()
        return got

    worst_ratio = 0.0
    for eta in (0.0, 0.9, 1.0):
        np.testing.assert_array_equal(run(weights.from_td_alpha, eta, 1.0), run(prio.from_td, eta),
                                      err_msg="alpha = 1 is fi_prio_from_td")
        for alpha in (0.6, 0.0):
            got = run(weights.from_td_alpha, eta, alpha)
            want = weights.td_priorities_alpha(vs, values, eta, alpha)
            if Bc >= 5:
                assert want[1] == Q_MAX and got[1] == Q_MAX, "a NaN column"
                assert want[0] == got[0] == (1 if alpha else 65536), "p = 0"
                if alpha:
                    assert 65536 < want[3] < Q_MAX, "p = 1e6 is above the table's range, p^0.6 inside it"
                    assert want[2] == Q_MAX and got[2] == Q_MAX, "Inf^alpha, or 0 * Inf = NaN"
            if alpha == 0.0:
                fin = want != Q_MAX
                assert (want[fin] == 65536).all() and (got[fin] == 65536).all()
            err = np.abs(got - want)
            worst = int(np.argmax(err / bar(want, Tc)))
            ratio = float(err[worst] / bar(want[worst], Tc))
            worst_ratio = max(worst_ratio, ratio)
            print(f"T {Tc} B {Bc} eta {eta} alpha {alpha}: worst column {worst}: dev {got[worst]} ref {want[worst]} "
                  f"bar {bar(want[worst], Tc):.2f} err/bar {ratio:.4f}")
            assert (err <= bar(want, Tc)).all(), (eta, alpha, worst, got[worst], want[worst])
            assert (got >= 1).all() and (got <= Q_MAX).all()
    print(f"T {Tc} B {Bc}: worst err/bar {worst_ratio:.4f}")
    dv.free()
    dval.free()


# ------------------------------------------------------------------ 3. the importance weights alone
def table_with(C, lo, q_window, rest=0xDEADBEEF):
    """(C,) uint32: q_window at the slots of the entries lo .., a value no draw may use elsewhere."""
    t = np.full(C, rest, np.uint32)
    t[(lo + np.arange(len(q_window))) % C] = q_window
    return t


def is_case(Bc, C, n_fresh, head, tail, seed, draw, q_window, beta):
    """fi_prio_fill_columns, then fi_prio_is_weights on the same stream, against the fp64 rule on the
    entries and the integers read back. The window is [max(0, head - C), tail); the kernels take the
    numbers as given, so head = tail makes the whole ring the window. Returns (w, w_ref, entries)."""
    from freeimpala_amd import hip, prio, weights
    lo = max(0, head - C)
    n_valid = tail - lo
    assert len(q_window) == n_valid
    table = table_with(C, lo, q_window)
    dt, ws = hip.DeviceBuffer.from_array(table), hip.DeviceBuffer(prio.CHUNK_WS_BYTES)
    out = Guarded([(Bc, np.uint64), (Bc, np.uint64), (2, np.uint64), (Bc, np.float32)])
    prio.fill_columns(out.ptr[0], out.ptr[1], out.ptr[2], 0x7F0000001000, 1024, C, Bc, n_fresh, tail, lo, n_valid, dt.ptr,
                      ws.ptr, seed, draw)
    weights.is_weights_dev(out.ptr[1], Bc, n_fresh, dt.ptr, C, lo, n_valid, ws.ptr, beta, out.ptr[3])
    hip.synchronize()
    got = out.read(("cols", "entries", "versions", "w"))
    np.testing.assert_array_equal(dt.download(np.uint32, (C,)), table, err_msg="the weights write no priority")
    for h in (out, dt, ws):
        h.free()
    entries = got["entries"].astype(np.int64)
    assert (entries[:n_fresh] == tail + np.arange(n_fresh)).all() and ((entries[n_fresh:] >= lo) & (entries[n_fresh:] < tail)).all()
    q_cols = np.ones(Bc, np.int64)
    q_cols[n_fresh:] = table[entries[n_fresh:] % C]
    Q = int(np.asarray(q_window, np.uint64).sum(dtype=np.uint64))
    ref = weights.is_weights(q_cols, n_fresh, n_valid, Q, beta)
    w = got["w"]
    worst = int(np.argmax(np.abs(w - ref) / ref))
    print(f"B {Bc} n_fresh {n_fresh} n_valid {n_valid} beta {beta}: worst column {worst}: dev {w[worst]!r} ref {ref[worst]!r} "
          f"rel {abs(w[worst] - ref[worst]) / ref[worst]:.2e}")
    np.testing.assert_allclose(w, ref, rtol=RTOL, atol=0)
    assert w.max() == np.float32(1.0) and (w > 0).all(), "the largest weight is exactly 1"
    assert len(set(w[:n_fresh].tolist())) <= 1, "every fresh column holds the same 1 / m"
    ratio32 = (q_cols[n_fresh:] * float(n_valid) / float(Q)).astype(np.float32)
    if n_fresh and (ratio32 >= 1).all():
        assert (w[:n_fresh] == 1.0).all(), "no replayed u above 1: the fresh columns are the maximum"
    return w, ref, entries


@pytest.mark.parametrize("beta", [0.4, 1.0])
def test_is_weights_kernel_equals_the_fp64_rule(beta):
    # B = 1
    w, _, _ = is_case(1, 8, 0, 3, 3, 1, 0, [1, 2, 5], beta)
    assert w.tolist() == [1.0]
    w, _, _ = is_case(1, 8, 1, 4, 3, 1, 0, [1, 2, 5], beta)
    assert w.tolist() == [1.0]
    # B = 5, two fresh columns, the window (1, 2, 5): seeds until a batch names two different entries
    for seed in range(1, 50):
        w, ref, e = is_case(5, 8, 2, 5, 3, seed, 0, [1, 2, 5], beta)
        if len(set(e[2:].tolist())) > 1:
            break
    assert len(set(e[2:].tolist())) > 1 and (w < 1).any() and len(set(w[2:].tolist())) > 1
    # a wrapped window of 1025 entries: two chunk sums
    C, n_valid = 4096, 1025
    lo = C - 1000
    rs = np.random.RandomState(1025)
    q = rs.randint(1, 2 ** 16 + 1, n_valid).astype(np.uint32)
    q[-1] = 2 ** 24  # in the second chunk: left out of Q, every ratio would be off by a third
    w, _, e = is_case(64, C, 3, lo + C, lo + n_valid, 21, 4, q, beta)
    assert len(set(w.tolist())) > 20 and (e == lo + n_valid - 1).any()
    # one Q_MAX among ones in a full ring of 2048 slots: every replayed column names it
    C = 2048
    q = np.ones(C, np.uint32)
    q[777] = Q_MAX
    w, ref, e = is_case(64, C, 2, 2 * C + 123, 2 * C + 123, 22, 0, q, beta)
    assert (e[2:] == C + 123 + 777).all() and (w[:2] == 1.0).all()
    np.testing.assert_allclose(w[2:], (Q_MAX * 2048.0 / (Q_MAX + 2047.0)) ** -float(np.float32(beta)), rtol=RTOL)
    # more columns than twice the workgroup: the strided loops run three times, the last with 3 lanes
    Bc = 2 * 256 + 3
    C, n_valid = 4096, 3000
    q = rs.randint(1, 2 ** 16 + 1, n_valid).astype(np.uint32)
    w, _, _ = is_case(Bc, C, 100, 500 + C, 500 + n_valid, 51, 9, q, beta)
    assert len(set(w[100:].tolist())) > 100
    # every replayed column above the mean priority: the fresh columns hold the maximum
    q = np.ones(C, np.uint32)
    q[5] = 2 ** 30  # 4,095 of the total 2^30 + 4,095 lie elsewhere: no column of 508 is expected to land there
    w, _, e = is_case(Bc, C, 7, 2 * C, 2 * C, 52, 1, q, beta)
    assert (e[7:] == C + 5).all() and (w[:7] == 1.0).all() and (w[7:] < 1).all()


# ------------------------------------------------------------------ 4. end to end
def lo_of(i):
    return max(0, i["head"] - i["capacity"])


def columns_scaled(R, U, w, A):
    """R's dlogits / dvalue are U's (the unweighted learner on the same entries) times w_b, exactly;
    what V-trace reports besides is unweighted."""
    for nm in ("vs", "pg_adv", "logits", "values"):
        np.testing.assert_array_equal(R.tensor(nm), U.tensor(nm), err_msg=nm)
    w = np.asarray(w, np.float32)
    np.testing.assert_array_equal(R.tensor("dlogits").reshape(T, B, A), U.tensor("dlogits").reshape(T, B, A) * w[None, :, None])
    dv, du = R.tensor("dvalue").reshape(T + 1, B), U.tensor("dvalue").reshape(T + 1, B)
    np.testing.assert_array_equal(dv[:T], du[:T] * w[None, :])
    np.testing.assert_array_equal(dv[T], du[T])


@pytest.mark.parametrize("arch,A", [("mlp", 3), ("atari", 18)])
def test_weighted_prioritised_steps_equal_the_host_rule_and_the_host_fed_learner(arch, A, orc):
    from freeimpala_amd.prio import prio_batch_entries
    from freeimpala_amd.ring import EntryRing
    from freeimpala_amd.weights import is_weights, td_priorities_alpha
    C, ALPHA, BETA = 16, 0.6, 0.5
    raw, _ = make_entries(arch, 15, A, seed=200 + A)
    R, Hh = learner_pair(arch, A)
    U = make_learner(arch, A)  # unweighted, on the same entries from the same parameters
    E = R.entry_bytes
    ring = EntryRing(E, C, seed=17)
    ring.enable_priorities(ETA, 1.0)
    assert ring.priority_exponents() == dict(alpha=1.0, beta=0.0, weights_valid=False)
    ring.set_priority_exponents(ALPHA, BETA)
    assert ring.priority_exponents() == dict(alpha=float(np.float32(ALPHA)), beta=BETA, weights_valid=False)
    assert ring.priority_info()["q_init"] == 65536, "init_priority stays in the table's own domain"
    src = spaced(raw[:10], E + 48)
    ring.push(src.ptr, E + 48, 10)

    def step(n_fresh):
        i = ring.info()
        lo = lo_of(i)
        n_valid = i["tail"] - lo
        window = ring.priorities() if n_valid else np.zeros(0, np.uint32)
        seed = i["seed"]
        if n_fresh < B:
            # a seed for which the replayed columns do not all share one priority: a weight below 1
            def spread(s):
                e = prio_batch_entries(orc.philox4, s, i["draw"], B, n_fresh, i["head"], i["tail"], C, window)[n_fresh:]
                return len(set(int(window[x - lo]) for x in e)) > 1
            found = [s for s in range(1, 400) if spread(s)]
            assert found, "a non-uniform table gives such a seed below 400"
            seed = found[0]
            ring.seed(seed, i["draw"])
        want = prio_batch_entries(orc.philox4, seed, i["draw"], B, n_fresh, i["head"], i["tail"], C, window)
        q_cols = np.array([1] * n_fresh + [int(window[e - lo]) for e in want[n_fresh:]], np.int64)
        w_ref = is_weights(q_cols, n_fresh, n_valid, int(window.astype(np.uint64).sum()), BETA)
        p_before = R.get_params()
        st = R.step_ring(ring, n_fresh=n_fresh, prioritized=True)
        w = ring.last_weights(B)
        assert ring.last_entries(B) == want
        assert ring.priority_exponents()["weights_valid"] == (n_fresh < B)
        print(f"n_fresh {n_fresh}: entries {want} w {w.tolist()} ref {w_ref.tolist()}")
        np.testing.assert_allclose(w, w_ref, rtol=RTOL, atol=0)
        assert w.max() == 1.0
        if n_fresh < B:
            assert (w < 1).any()
        else:
            assert (w == 1).all()
        rows = [raw[e] for e in want]
        Hh.set_column_weights(w)
        np.testing.assert_array_equal(Hh.column_weights(), w)
        same(snapshot(R, st), snapshot(Hh, Hh.step(rows)), f"weighted step, n_fresh {n_fresh}")
        for nm in ("dlogits", "dvalue", "grads", "values", "pg_adv"):
            np.testing.assert_array_equal(R.tensor(nm), Hh.tensor(nm), err_msg=nm)
        U.set_params(p_before)
        U.step(rows)
        columns_scaled(R, U, w, A)
        # the refresh stores p^alpha: the maximum over the columns that name an entry
        q_new = td_priorities_alpha(R.tensor("vs").reshape(T, B), R.tensor("values").reshape(T + 1, B), ETA, ALPHA)
        after = ring.info()
        now = ring.priorities().astype(np.int64)
        for e in range(lo, after["tail"]):
            cols = [b for b in range(B) if want[b] == e]
            if cols:
                ref = int(max(q_new[b] for b in cols))
                print(f"entry {e}: columns {cols}: dev {now[e - lo]} ref {ref} bar {bar(ref, T):.2f}")
                assert abs(int(now[e - lo]) - ref) <= bar(ref, T), (e, cols, now[e - lo], ref)
            else:
                assert now[e - lo] == (window[e - lo] if e < i["tail"] else 65536), e
        return want, w

    e, w = step(5)
    assert e == [0, 1, 2, 3, 4]
    ring.set_priorities(0, [1, 70000, 3 * 65536, 500, 2 ** 20])
    e, w = step(2)
    assert e[:2] == [5, 6] and w[0] == w[1]
    step(0)
    step(3)
    assert ring.info()["tail"] == 10
    # beta = 0 again: the next step computes nothing
    ring.set_priority_exponents(ALPHA, 0.0)
    R.step_ring(ring, n_fresh=0, prioritized=True)
    assert (ring.last_weights(B) == 1).all() and not ring.priority_exponents()["weights_valid"]
    src.free()
    for h in (ring, R, Hh, U):
        h.close()


# ------------------------------------------------------------------ 5. linearity
@pytest.mark.parametrize("arch,A", [("mlp", 3), ("atari", 18)])
def test_half_weights_halve_the_gradient(arch, A):
    raw, _ = make_entries(arch, B, A, seed=300 + A)
    X, U = learner_pair(arch, A, max_grad_norm=1e9)
    X.set_column_weights([0.5] * B)
    rows = [r for r in raw]
    sx, su = X.step(rows), U.step(rows)
    columns_scaled(X, U, [0.5] * B, A)
    gx, gu = X.tensor("grads"), U.tensor("grads")
    assert np.isfinite(gu).all() and gu.any()
    np.testing.assert_array_equal(gx, gu * np.float32(0.5))
    # the reported losses are V-trace's unweighted sums, the norm is the weighted gradient's
    for k in ("pg_loss", "baseline_loss", "entropy_loss", "total_loss"):
        assert sx[k] == su[k], k
    assert sx["grad_norm"] == pytest.approx(0.5 * su["grad_norm"], rel=1e-12)
    X.close()
    U.close()


@pytest.mark.parametrize("arch,A", [("mlp", 3), ("atari", 18)])
def test_a_zero_weight_masks_its_column(arch, A):
    """w = (1, 0, 1, 0, 1): two batches that differ only in the rewards and actions of the columns
    1 and 3 give the same gradient and the same parameters."""
    from freeimpala_amd import _abi
    raw, _ = make_entries(arch, B, A, seed=310 + A)
    rec, act_off, rew_off = (_abi.ATARI_PLANE_RECORD_BYTES, _abi.PLANE_REC_ACT, _abi.PLANE_REC_REW) if arch == "atari" \
        else (1024, 768, 772)
    other = raw.copy()
    for b in (1, 3):
        for t in range(T):
            a = other[b, t * rec + act_off:t * rec + act_off + 4].view(np.int32)
            a[:] = (a + 1) % A
            r = other[b, t * rec + rew_off:t * rec + rew_off + 4].view(np.float32)
            r[:] = r * np.float32(-3.0) + np.float32(1.25)
    assert (other[[1, 3]] != raw[[1, 3]]).any() and (other[[0, 2, 4]] == raw[[0, 2, 4]]).all()
    X, Y = learner_pair(arch, A)
    mask = np.array([1, 0, 1, 0, 1], np.float32)
    for L in (X, Y):
        L.set_column_weights(mask)
        np.testing.assert_array_equal(L.column_weights(), mask)
    X.step([r for r in raw])
    Y.step([r for r in other])
    assert (X.tensor("rewards") != Y.tensor("rewards")).any() and (X.tensor("actions", np.int32) != Y.tensor("actions", np.int32)).any()
    assert (X.tensor("vs") != Y.tensor("vs")).any(), "the masked columns' own numbers do differ"
    gx = X.tensor("grads")
    assert gx.any()
    np.testing.assert_array_equal(gx, Y.tensor("grads"))
    np.testing.assert_array_equal(X.get_params(), Y.get_params())
    # without the mask the same two batches do not
    X.set_column_weights(None)
    Y.set_column_weights(None)
    assert (X.column_weights() == 1).all()
    X.step([r for r in raw])
    Y.step([r for r in other])
    assert (X.tensor("grads") != Y.tensor("grads")).any()
    X.close()
    Y.close()


# ------------------------------------------------------------------ 6. nothing moves by default
def test_neutral_exponents_and_cleared_weights_move_nothing():
    """As test_gpu_prio.py::test_async_steps_leave_the_same_table: a ring with exponents (1, 0) and a
    learner whose column weights were set and cleared reproduce, step for step, a run that never
    called either."""
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, 10, A, seed=120)
    runs = {}
    for wait in (True, False):
        for neutral in (False, True):
            R = make_learner(arch, A)
            E = R.entry_bytes
            ring = EntryRing(E, 16, seed=5)
            ring.enable_priorities(ETA, 0.25)
            if neutral:
                ring.set_priority_exponents(1.0, 0.0)
                R.set_column_weights(np.linspace(0.0, 2.0, B))
                R.set_column_weights(None)
            src = spaced(raw, E)
            ring.push(src.ptr, E, 10)
            steps = []
            for n_fresh in (5, 2, 0, 3):
                st = R.step_ring(ring, n_fresh=n_fresh, wait=wait, prioritized=True)
                if not wait:
                    st = R.wait()
                steps.append((ring.last_entries(B), ring.priorities().copy(), R.get_params(),
                              {k: v for k, v in st.items() if k != "step_ms"}, R.tensor("dlogits"), R.tensor("dvalue")))
                assert (ring.last_weights(B) == 1).all() and (R.column_weights() == 1).all()
            assert ring.priority_exponents() == dict(alpha=1.0, beta=0.0, weights_valid=False)
            runs[wait, neutral] = (steps, ring.priority_info(), ring.info(), ring.read_slots())
            src.free()
            ring.close()
            R.close()
    for wait in (True, False):
        plain, neutral = runs[wait, False], runs[wait, True]
        assert plain[1] == neutral[1] and plain[2] == neutral[2]
        np.testing.assert_array_equal(plain[3], neutral[3])
        for k, (a, b) in enumerate(zip(plain[0], neutral[0])):
            assert a[0] == b[0] and a[3] == b[3], (wait, k)
            for x, y in zip(a[1:3] + a[4:], b[1:3] + b[4:]):
                np.testing.assert_array_equal(x, y, err_msg=f"wait {wait}, step {k}")
    assert len(set(int(q) for q in runs[True, False][0][-1][1])) > 3, "the table holds refreshed values"


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_everything_as_it_was():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, 10, A, seed=330)
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    src = spaced(raw, E)
    ring = EntryRing(E, 16, seed=2)
    ring.push(src.ptr, E, 10)
    with pytest.raises(FiError, match=r"rc=-4: .*priorities are not enabled"):
        ring.set_priority_exponents(0.5, 0.5)
    with pytest.raises(FiError, match=r"rc=-4: .*priorities are not enabled"):
        ring.priority_exponents()
    with pytest.raises(FiError, match=r"rc=-4: .*priorities are not enabled"):
        ring.last_weights(B)
    ring.enable_priorities(ETA, 1.0)
    ring.set_priority_exponents(0.75, 0.25)
    R.step_ring(ring, prioritized=True)  # entries 0 .. 4: tail = 5
    ring.set_priorities(0, [1, 70000, 3 * 65536, 500, 2 ** 20])
    held = np.array([1.0, 0.5, 0.0, 2.0, 0.25], np.float32)
    R.set_column_weights(held)

    def refused(match, call, *args, **kw):
        before = ring.info(), ring.priority_info(), ring.priority_exponents()
        table, params, w = ring.priorities(), R.get_params(), R.column_weights()
        with pytest.raises(FiError, match=match):
            call(*args, **kw)
        assert (ring.info(), ring.priority_info(), ring.priority_exponents()) == before
        np.testing.assert_array_equal(ring.priorities(), table)
        np.testing.assert_array_equal(R.get_params(), params)
        np.testing.assert_array_equal(R.column_weights(), w)
        np.testing.assert_array_equal(w, held)

    refused(r"rc=-1: .*alpha 1.5\d* outside \[0, 1\]", ring.set_priority_exponents, 1.5, 0.5)
    refused(r"rc=-1: .*alpha -0.1\d* outside \[0, 1\]", ring.set_priority_exponents, -0.1, 0.5)
    refused(r"rc=-1: .*beta 1.0+1\d* outside \[0, 1\]", ring.set_priority_exponents, 0.5, 1.001)
    refused(r"rc=-1: .*beta -1.0\d* outside \[0, 1\]", ring.set_priority_exponents, 0.5, -1.0)
    refused(r"rc=-1: .*alpha -?nan outside", ring.set_priority_exponents, float("nan"), 0.5)
    refused(r"rc=-1: .*weight -0.5\d* at index 3 is negative or not finite", R.set_column_weights, [1, 1, 1, -0.5, 1])
    refused(r"rc=-1: .*weight -?nan at index 0", R.set_column_weights, [np.nan, 1, 1, 1, 1])
    refused(r"rc=-1: .*weight inf at index 4", R.set_column_weights, [1, 1, 1, 1, np.inf])
    refused(rf"rc=-1: .*n = {B - 1} != the learner's batch {B}", R.set_column_weights, [1.0] * (B - 1))
    refused(rf"rc=-1: .*n = {B + 1} != the learner's batch {B}", R.set_column_weights, [1.0] * (B + 1))
    # one source of weights per step: beta > 0 and column weights, whatever n_fresh and wait are
    for kw in (dict(n_fresh=2), dict(n_fresh=0, wait=False), dict(n_fresh=B)):
        refused(r"rc=-4: .*beta = 0.25\d* and the learner has column weights set", R.step_ring, ring, prioritized=True, **kw)
    # the uniform step and a beta = 0 prioritised step take the learner's weights
    ring.set_priority_exponents(0.75, 0.0)
    Hh.load_state(R.save_state())
    Hh.set_column_weights(held)
    got = snapshot(R, R.step_ring(ring, n_fresh=2, prioritized=True))
    same(got, snapshot(Hh, Hh.step([raw[e] for e in ring.last_entries(B)])), "beta = 0 with column weights")
    assert (ring.last_weights(B) == 1).all()
    # cleared, beta > 0 steps; the wrong n for its weights is refused
    ring.set_priority_exponents(0.75, 0.25)
    R.set_column_weights(None)
    R.step_ring(ring, n_fresh=1, prioritized=True)
    assert ring.priority_exponents()["weights_valid"] and ring.last_weights(B).max() == 1.0
    with pytest.raises(FiError, match=rf"rc=-1: .*n = {B + 1} != the last step's batch {B}"):
        ring.last_weights(B + 1)
    for h in (ring, R, Hh):
        h.close()
    src.free()
