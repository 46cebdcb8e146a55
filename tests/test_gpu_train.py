"""The training recipe (include/fi_train.h) on the device: the RMSProp kernel alone and inside the
learner against the fp64 rule (freeimpala_amd/train.py), the learning-rate schedule, the reward clip,
resume, the handles that never call any of it, and the C++ check program.

The error bars of one RMSProp update, u = 2^-24, by counting fp32 roundings (first order; the
reference is the fp64 rule fed the same fp32 numbers, `scale` included, so it carries no error of its
own at this scale). FMA contraction only removes roundings, so the count holds either way.
  g' = fl(g scale)                                   1 rounding: u
  (1 - decay)                                        u (exact for decay >= 1/2)
  t2 = ((1 - decay) g') g'                           2u from g' twice, u from (1 - decay), 2 products: 5u
  t1 = decay v                                       u
  v' = fl(t1 + t2)                                   both terms >= 0, so the relative errors do not amplify:
                                                     max(5u, u) + u = 6u                  bar:  8u v'
  d  = fl(fl(sqrt v') + eps)                         sqrt halves 6u and rounds: 4u; the sum of two
                                                     non-negative terms: 5u (eps inside the root: 4.5u)
  q  = fl(g' / d)                                    u + 5u + u = 7u
  m' = fl(fl(momentum m) + q)                        2u |momentum m| + 8u |q|             bar: 12u (|momentum m| + |q|)
  p' = fl(p - fl(lr m'))                             u |p'| + lr (3u |momentum m| + 9u |q|)
                                                                                          bar: u |p'| + 16u lr (|momentum m| + |q|)
The count stays inside the three bars the feature was specified with (8u, 12u, 16u), which are kept:
they leave room for the second-order terms. Each bar also carries 4 * 2^-149: a product or sum that
lands below 2^-126 is rounded to a multiple of 2^-149, not relatively, and the learner's own
gradients (unlike the inputs of the kernel test, which avoid it) hold elements whose square does.
sqrt(4 * 2^-149) = 7.5e-23 next to eps >= 1e-3 does not reach d. A first step from v = m = 0 is also
compared with its closed form, q = g' / (sqrt(1 - decay) |g'| + eps), under the same bars.

The clamp, the schedule's effect (lr travels by value) and everything about resume are compared
exactly."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_ring import B, T, Guarded, learner_pair, make_entries, make_learner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TINY = 4 * 2.0 ** -149
ARCHS = [("mlp", 3), ("atari", 18)]
WORST = {"v": 0.0, "m": 0.0, "p": 0.0}


def f32(x):
    return float(np.float32(x))


def within_bars(what, got_p, got_v, got_m, p, g, v, m, lr, decay, momentum, eps, eps_in_sqrt, scale):
    """The device's p, v, m after one update of the before-state (p, g, v, m) against the fp64 rule;
    prints and returns the worst ratio to each bar."""
    from freeimpala_amd.train import rmsprop_reference
    lr, decay, momentum, eps, scale = f32(lr), f32(decay), f32(momentum), f32(eps), f32(scale)
    p64, g64, v64 = (np.asarray(x, np.float64) for x in (p, g, v))
    m64 = np.asarray(m, np.float64) if momentum > 0 else None
    rp, rv, rm = rmsprop_reference(p64, g64, v64, m64, lr, decay, momentum, eps, eps_in_sqrt, scale)
    gs = g64 * scale
    q = np.abs(gs / (np.sqrt(rv + eps) if eps_in_sqrt else np.sqrt(rv) + eps))
    mm = np.abs(momentum * m64) if momentum > 0 else 0.0
    bars = {"v": 8 * U * rv + TINY, "m": 12 * U * (mm + q) + TINY, "p": U * np.abs(rp) + 16 * U * lr * (mm + q) + TINY}
    pairs = {"v": (got_v, rv), "p": (got_p, rp)}
    if momentum > 0:
        pairs["m"] = (got_m, rm)
    ratios = {}
    for k, (got, ref) in pairs.items():
        err = np.abs(np.asarray(got, np.float64) - ref)
        r = err / bars[k]
        i = int(np.argmax(r))
        ratios[k] = float(r[i])
        WORST[k] = max(WORST[k], ratios[k])
        assert (err <= bars[k]).all(), (what, k, i, got[i], ref[i], float(err[i]), float(bars[k][i]))
    print(f"{what}: worst err/bar " + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    return ratios


# ------------------------------------------------------------------ 1. the RMSProp kernel alone
SENTINEL = np.uint32(0x7FC12345)


def kernel_inputs(n, seed):
    """|g| in [1e-6, 10] plus exact zeros, v >= 0 (some zeros), m of mixed sign: nothing is denormal."""
    rs = np.random.RandomState(seed)
    g = (10.0 ** rs.uniform(-6, 1, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rs.rand(n) < 0.1] = 0.0
    v = (10.0 ** rs.uniform(-8, 2, n)).astype(np.float32)
    v[rs.rand(n) < 0.1] = 0.0
    m = (rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 2, n)).astype(np.float32)
    p = rs.standard_normal(n).astype(np.float32)
    if n >= 4:
        g[0], v[0] = 0.0, 0.0  # d = eps (or sqrt(eps)), q = 0
    return p, g, v, m


def run_kernel(p, g, v, m, lr, decay, momentum, eps, eis, sqnorm=None, max_norm=0.0, skip=None, offset=0):
    """fi_train_rmsprop_update between guards; `offset` floats behind a 16-byte boundary. m = None: the
    buffer holds SENTINEL. Returns (p, v, m as uint32, skip words)."""
    from freeimpala_amd import hip, train
    n = p.size
    out = Guarded([(n + offset, np.float32), (n + offset, np.float32), (n + offset, np.uint32)])
    ptr = [q + 4 * offset for q in out.ptr]
    hip.upload_ptr(ptr[0], p)
    hip.upload_ptr(ptr[1], v)
    hip.upload_ptr(ptr[2], np.full(n, SENTINEL, np.uint32) if m is None else m.view(np.uint32))
    dg = hip.DeviceBuffer.from_array(np.concatenate([np.zeros(offset, np.float32), g]))
    dn = hip.DeviceBuffer.from_array(np.array([sqnorm], np.float64)) if sqnorm is not None else None
    ds = hip.DeviceBuffer.from_array(np.asarray(skip, np.int32)) if skip is not None else None
    train.rmsprop_update(ptr[0], dg.ptr + 4 * offset, ptr[1], ptr[2], n, lr, decay, momentum, eps, eis,
                         dn.ptr if dn else None, max_norm, ds.ptr if ds else None)
    hip.synchronize()
    got = out.read(("p", "v", "m"))
    words = ds.download(np.int32, (4,)) if ds else None
    for k in ("p", "v", "m"):
        assert (got[k][:offset].view(np.uint8) == 0xA5).all(), k + ": the floats in front"
    for h in (out, dg, dn, ds):
        if h:
            h.free()
    return got["p"][offset:], got["v"][offset:], got["m"][offset:], words


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 1027, 70001])
def test_rmsprop_kernel_meets_the_derived_bars(n):
    lr, decay, eps = 4.8e-4, 0.99, 0.01
    for momentum in (0.0, 0.9):
        for eis in (False, True):
            for clip in (False, True):
                p, g, v, m = kernel_inputs(n, n * 8 + int(momentum * 10) * 4 + eis * 2 + clip)
                # norm = 80 > max_norm = 40: scale = (float)(40 / (80 + 1e-6)) < 1
                scale = f32(40.0 / (80.0 + 1e-6)) if clip else 1.0
                gp, gv, gm, words = run_kernel(p, g, v, m if momentum else None, lr, decay, momentum, eps, eis,
                                               sqnorm=6400.0 if clip else None, max_norm=40.0 if clip else 0.0,
                                               skip=[0, 0, 0, 0] if clip else None)
                within_bars(f"n {n} momentum {momentum} eps_in_sqrt {eis} clip {clip}", gp, gv, gm.view(np.float32), p, g, v, m,
                            lr, decay, momentum, eps, eis, scale)
                if not momentum:
                    assert (gm == SENTINEL).all(), "momentum 0 never touches m"
                if clip:
                    assert words.tolist() == [0, 0, 0, 0]
                    assert scale < 1
                if n >= 4 and not momentum:  # g = 0, v = 0: nothing moves
                    assert gv[0] == 0 and gp[0] == p[0]
    print(f"n {n}: worst err/bar so far {WORST}")


def test_rmsprop_kernel_off_a_16_byte_boundary_and_by_grid_stride():
    """Pointers one float behind a 16-byte boundary take the element-wise path; 2^21 + 4 * 256 + 3
    quads-and-tail is more than the 8192 x 256 lanes of the largest grid, so lanes take a second quad."""
    p, g, v, m = kernel_inputs(1027, 99)
    gp, gv, gm, _ = run_kernel(p, g, v, m, 1e-3, 0.9, 0.5, 1e-3, False, offset=1)
    within_bars("offset 1", gp, gv, gm.view(np.float32), p, g, v, m, 1e-3, 0.9, 0.5, 1e-3, False, 1.0)
    n = 4 * (8192 * 256 + 256) + 3
    p, g, v, m = kernel_inputs(n, 100)
    gp, gv, gm, _ = run_kernel(p, g, v, None, 1e-3, 0.9, 0.0, 1e-3, True)
    within_bars(f"n {n}", gp, gv, None, p, g, v, None, 1e-3, 0.9, 0.0, 1e-3, True, 1.0)
    assert (gm == SENTINEL).all() and (gp[-3:] != p[-3:]).any()


@pytest.mark.parametrize("n", [5, 1027])
def test_rmsprop_kernel_skips_a_rejected_update(n):
    p, g, v, m = kernel_inputs(n, 7 * n)
    for flags, why in (([1, 0, 0, 0], 1), ([0, 1, 0, 0], 2)):
        gp, gv, gm, words = run_kernel(p, g, v, m, 1e-2, 0.9, 0.9, 0.01, False, sqnorm=6400.0, max_norm=40.0, skip=flags)
        for got, was, nm in ((gp, p, "p"), (gv, v, "v"), (gm.view(np.float32), m, "m")):
            np.testing.assert_array_equal(got.view(np.uint32), was.view(np.uint32), err_msg=nm)
        assert words.tolist() == flags[:2] + [1, why], "counted once, with its reason"


def test_standalone_entry_points_refuse_bad_arguments():
    from freeimpala_amd import hip, train
    from freeimpala_amd._abi import FiError
    buf = hip.DeviceBuffer.from_array(np.ones(16, np.float32))
    a = (buf.ptr, buf.ptr, buf.ptr, buf.ptr, 4, 1e-3)
    for args, match in (((1.0, 0.0, 0.01), r"rc=-1: .*decay 1.0+ outside \[0, 1\)"),
                        ((-0.5, 0.0, 0.01), r"rc=-1: .*decay -0.50* outside"),
                        ((0.9, 1.0, 0.01), r"rc=-1: .*momentum 1.0+ outside \[0, 1\)"),
                        ((0.9, 0.0, 0.0), r"rc=-1: .*eps 0.0+ is not positive and finite"),
                        ((0.9, 0.0, float("inf")), r"rc=-1: .*eps inf is not positive"),
                        ((0.9, float("nan"), 0.01), r"rc=-1: .*momentum -?nan outside")):
        with pytest.raises(FiError, match=match):
            train.rmsprop_update(*a, *args)
    with pytest.raises(FiError, match=r"rc=-1: .*momentum 0.50* needs m"):
        train.rmsprop_update(buf.ptr, buf.ptr, buf.ptr, None, 4, 1e-3, 0.9, 0.5, 0.01)
    with pytest.raises(FiError, match=r"rc=-1: .*max_norm 40.0+ needs sqnorm_dev"):
        train.rmsprop_update(*a, 0.9, 0.0, 0.01, max_norm=40.0)
    for c in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(FiError, match=r"rc=-1: .*is not positive and finite"):
            train.clip_rewards_dev(buf.ptr, 4, c)
    hip.synchronize()
    assert (buf.download(np.float32, (16,)) == 1).all()
    buf.free()


# ------------------------------------------------------------------ 2. RMSProp in the learner
def batches_of(arch, A, k, seed):
    raw, _ = make_entries(arch, k * B, A, seed=seed)
    return [[r for r in raw[i * B:(i + 1) * B]] for i in range(k)]


@pytest.mark.parametrize("arch,A", ARCHS)
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_learner_steps_meet_the_bars(arch, A, momentum):
    from freeimpala_amd._abi import FiError
    lr, decay, eps, eis = 2e-3, 0.95, 1e-3, bool(momentum)
    max_norm = 0.05 if momentum else 40.0  # the first is below these batches' gradient norms: scale < 1
    L = make_learner(arch, A, optimizer="rmsprop", lr=lr, max_grad_norm=max_norm)
    st = L.train_state()
    assert st["optimizer"] == "rmsprop" and (st["decay"], st["momentum"], st["eps"], st["eps_in_sqrt"]) == \
        (f32(0.99), 0.0, f32(0.01), False), "optimizer='rmsprop' is set_rmsprop() with monobeast's numbers"
    L.set_rmsprop(decay, momentum, eps, eis)  # still before the first step: allowed again
    st = L.train_state()
    assert (st["decay"], st["momentum"], st["eps"], st["eps_in_sqrt"]) == (f32(decay), f32(momentum), f32(eps), eis)
    scales = []
    for k, rows in enumerate(batches_of(arch, A, 3, seed=400 + A)):
        p0, v0, m0 = L.tensor("params"), L.tensor("adam_v"), L.tensor("adam_m")
        stats = L.step(rows)
        g, p1, v1, m1 = L.tensor("grads"), L.tensor("params"), L.tensor("adam_v"), L.tensor("adam_m")
        norm = stats["grad_norm"]
        scale = f32(max_norm / (norm + 1e-6)) if norm > max_norm else 1.0
        scales.append(scale)
        assert np.isfinite(g).all() and g.any() and (v1 >= 0).all()
        within_bars(f"{arch} momentum {momentum} step {k + 1} scale {scale:.4f}", p1, v1, m1, p0, g, v0, m0, lr, decay,
                    momentum, eps, eis, scale)
        if not momentum:
            assert not m1.any(), "momentum 0 leaves the momentum slab at zero"
        if k == 0:  # from v = m = 0: q = g' / (sqrt((1 - decay) g'^2 [+ eps]) [+ eps])
            assert not v0.any() and not m0.any()
            gs = g.astype(np.float64) * scale
            v_cf = (1.0 - f32(decay)) * gs * gs
            q = gs / (np.sqrt(v_cf + f32(eps)) if eis else np.sqrt(1.0 - f32(decay)) * np.abs(gs) + f32(eps))
            p_cf = p0.astype(np.float64) - f32(lr) * q
            assert (np.abs(v1 - v_cf) <= 8 * U * v_cf + TINY).all()
            assert (np.abs(p1 - p_cf) <= U * np.abs(p_cf) + 16 * U * f32(lr) * np.abs(q) + TINY).all()
            if momentum:
                assert (np.abs(m1 - q) <= 12 * U * np.abs(q) + TINY).all()
    if momentum:
        assert min(scales) < 1, scales
    assert L.train_state()["next_update"] == 4
    before = L.train_state(), L.get_params()
    with pytest.raises(FiError, match=r"rc=-4: .*an update has been enqueued \(step_count 3\)"):
        L.set_rmsprop()
    assert L.train_state() == before[0]
    np.testing.assert_array_equal(L.get_params(), before[1])
    L.close()
    print(f"worst err/bar so far {WORST}")


def test_rmsprop_arguments_out_of_range_are_refused():
    from freeimpala_amd._abi import FiError
    L = make_learner("mlp", 3, optimizer="sgd")
    for kw, match in ((dict(decay=1.0), r"rc=-1: .*decay 1.0+ outside \[0, 1\)"),
                      (dict(decay=-0.25), r"rc=-1: .*decay -0.250* outside"),
                      (dict(momentum=1.5), r"rc=-1: .*momentum 1.50* outside \[0, 1\)"),
                      (dict(momentum=-0.1), r"rc=-1: .*momentum -0.1\d* outside"),
                      (dict(eps=0.0), r"rc=-1: .*eps 0.0+ is not positive and finite"),
                      (dict(eps=-1.0), r"rc=-1: .*eps -1.0+ is not positive"),
                      (dict(eps=float("inf")), r"rc=-1: .*eps inf is not positive"),
                      (dict(eps=float("nan")), r"rc=-1: .*eps -?nan is not positive")):
        with pytest.raises(FiError, match=match):
            L.set_rmsprop(**kw)
        assert L.train_state()["optimizer"] == "sgd"
    for call, arg, match in ((L.set_lr, -1e-3, r"rc=-1: .*lr -0.0010* is negative or not finite"),
                             (L.set_lr, float("inf"), r"rc=-1: .*lr inf is negative or not finite"),
                             (L.set_reward_clip, -1.0, r"rc=-1: .*c -1.0+ is negative or not finite"),
                             (L.set_reward_clip, float("nan"), r"rc=-1: .*c -?nan is negative or not finite")):
        with pytest.raises(FiError, match=match):
            call(arg)
    with pytest.raises(FiError, match=r"rc=-1: .*lr_end -0.50* is negative or not finite"):
        L.set_lr_schedule(-0.5, 10)
    with pytest.raises(FiError, match=r"rc=-1: .*n_steps 0"):
        L.set_lr_schedule(0.0, 0)
    st = L.train_state()
    assert st == dict(optimizer="sgd", eps_in_sqrt=False, decay=0.0, momentum=0.0, eps=0.0, lr_base=f32(1e-3), lr_end=0.0,
                      lr_next=f32(1e-3), reward_clip=0.0, schedule_on=0, lr_steps=0, next_update=1)
    L.close()


# ------------------------------------------------------------------ 3. the schedule
def test_schedule_to_zero_stops_the_parameters_while_the_version_advances():
    from freeimpala_amd.train import lr_at
    lr = 0.01
    L = make_learner("mlp", 3, optimizer="sgd", lr=lr, max_grad_norm=0.0)
    L.set_lr_schedule(lr_end=0.0, n_steps=2)
    params = [L.get_params()]
    for s, rows in enumerate(batches_of("mlp", 3, 4, seed=500), start=1):
        st = L.train_state()
        assert st["schedule_on"] == 1 and st["next_update"] == s and st["lr_steps"] == 2
        assert st["lr_next"] == lr_at(s, lr, 0.0, 2) == [f32(lr), f32(f32(lr) / 2), 0.0, 0.0][s - 1]
        stats = L.step(rows)
        assert stats["version"] == s and stats["grad_norm"] > 0
        params.append(L.get_params())
    assert (params[1] != params[0]).any() and (params[2] != params[1]).any()
    # update 1 ran at lr_base: p1 = fl(p0 - lr g) is what sgd_kernel computes; 3 and 4 at 0
    np.testing.assert_array_equal(params[3].view(np.uint32), params[2].view(np.uint32))
    np.testing.assert_array_equal(params[4].view(np.uint32), params[2].view(np.uint32))
    L.clear_lr_schedule()
    st = L.train_state()
    assert st["schedule_on"] == 0 and st["lr_next"] == f32(lr) and st["next_update"] == 5
    L.close()


@pytest.mark.parametrize("optimizer", ["sgd", "adam", "rmsprop"])
def test_a_schedule_is_set_lr_before_every_step(optimizer):
    from freeimpala_amd.train import lr_at
    lr, end, n = 3e-3, 5e-4, 3
    S, M = learner_pair("mlp", 3, optimizer=optimizer, lr=lr)
    S.set_lr_schedule(end, n)
    data = batches_of("mlp", 3, 5, seed=510)
    for s, rows in enumerate(data, start=1):
        M.set_lr(lr_at(s, lr, end, n))
        assert M.train_state()["lr_next"] == S.train_state()["lr_next"] == lr_at(s, lr, end, n)
        a, b = S.step(rows), M.step(rows)
        assert {k: v for k, v in a.items() if k != "step_ms"} == {k: v for k, v in b.items() if k != "step_ms"}
        np.testing.assert_array_equal(S.get_params().view(np.uint32), M.get_params().view(np.uint32), err_msg=f"update {s}")
    assert S.train_state()["lr_next"] == f32(end) and M.train_state()["schedule_on"] == 0
    for nm in ("adam_m", "adam_v"):
        np.testing.assert_array_equal(S.tensor(nm), M.tensor(nm), err_msg=nm)
    # a constant-rate learner on the same data ends elsewhere: the schedule did change the updates
    P, Q = learner_pair("mlp", 3, optimizer=optimizer, lr=lr)
    Q.set_lr_schedule(end, n)
    for rows in data[:2]:
        P.step(rows)
        Q.step(rows)
    assert (P.get_params() != Q.get_params()).any()
    for h in (S, M, P, Q):
        h.close()


def test_async_steps_keep_the_rate_they_were_enqueued_with():
    lr, end, n = 0.02, 0.0, 3
    X, Y = learner_pair("mlp", 3, optimizer="sgd", lr=lr, max_grad_norm=0.0)
    for L in (X, Y):
        L.set_lr_schedule(end, n)
    data = batches_of("mlp", 3, 3, seed=520)
    for rows in data:
        X.step(rows)
    for rows in data:
        Y.step_async(rows)
    assert Y.train_state()["next_update"] == 4, "the numbers are given at enqueue time"
    st = Y.wait()
    assert st["version"] == 3
    np.testing.assert_array_equal(X.get_params().view(np.uint32), Y.get_params().view(np.uint32))
    assert X.train_state() == Y.train_state()
    X.close()
    Y.close()


# ------------------------------------------------------------------ 4. the reward clip
def clip_data(n, c):
    rs = np.random.RandomState(n)
    r = (rs.standard_normal(n) * 2 * c).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, c, -c, -0.0, 0.0, np.nextafter(np.float32(c), np.float32(9))], np.float32)
    k = min(n, special.size)
    r[rs.permutation(n)[:k]] = special[rs.permutation(special.size)[:k]]
    return r


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_clip_kernel_equals_the_host_rule(n):
    from freeimpala_amd import hip, train
    c = 0.7
    for offset in (0, 1):
        for rep in range(3 if n < 8 else 1):  # the small sizes see every special value over the repeats
            r = clip_data(n, c) if rep == 0 else np.roll(clip_data(8, c), rep)[:n]
            out = Guarded([(n + offset, np.float32)])
            hip.upload_ptr(out.ptr[0] + 4 * offset, r)
            train.clip_rewards_dev(out.ptr[0] + 4 * offset, n, c)
            hip.synchronize()
            got = out.read(("r",))["r"]
            out.free()
            assert (got[:offset].view(np.uint8) == 0xA5).all()
            np.testing.assert_array_equal(got[offset:].view(np.uint32), train.clip_rewards(r, c).view(np.uint32))
    r = clip_data(257, c)
    ref = train.clip_rewards(r, c)
    assert np.isnan(ref).sum() == 1 and (np.abs(ref[~np.isnan(ref)]) <= np.float32(c)).all() and (ref != r)[~np.isnan(r)].any()


def host_clipped(arch, raw, c):
    """The entries with their rewards clamped on the host."""
    from freeimpala_amd import _abi
    from freeimpala_amd.train import clip_rewards
    rec, off = (_abi.ATARI_PLANE_RECORD_BYTES, _abi.PLANE_REC_REW) if arch == "atari" else (1024, 772)
    out = raw.copy()
    for t in range(T):
        r = out[:, t * rec + off:t * rec + off + 4].copy().view(np.float32)
        out[:, t * rec + off:t * rec + off + 4] = clip_rewards(r, c).view(np.uint8)
    return out


@pytest.mark.parametrize("arch,A", ARCHS)
def test_clipped_step_equals_a_step_on_host_clipped_rewards(arch, A):
    c = 0.25
    raw, _ = make_entries(arch, B, A, seed=600 + A)
    X, Y = learner_pair(arch, A)
    X.set_reward_clip(c)
    assert X.train_state()["reward_clip"] == c and Y.train_state()["reward_clip"] == 0
    sx, sy = X.step([r for r in raw]), Y.step([r for r in host_clipped(arch, raw, c)])
    rx = X.tensor("rewards")
    assert (np.abs(rx) <= c).all() and (np.abs(rx) == c).any()
    for nm in ("rewards", "vs", "pg_adv", "dlogits", "dvalue", "grads"):
        np.testing.assert_array_equal(X.tensor(nm).view(np.uint32), Y.tensor(nm).view(np.uint32), err_msg=nm)
    np.testing.assert_array_equal(X.get_params().view(np.uint32), Y.get_params().view(np.uint32))
    assert {k: v for k, v in sx.items() if k != "step_ms"} == {k: v for k, v in sy.items() if k != "step_ms"}
    # off again: the next step sees the raw rewards
    X.set_reward_clip(0)
    X.step([r for r in raw])
    assert (np.abs(X.tensor("rewards")) > c).any()
    X.close()
    Y.close()


def test_resident_steps_are_clipped_once_in_effect():
    from freeimpala_amd.train import clip_rewards
    c = 0.25
    X, Y = learner_pair("mlp", 3)
    X.synth(seed=9)
    Y.synth(seed=9)
    r = X.tensor("rewards")
    assert (np.abs(r) > c).any()
    Y.upload("rewards", clip_rewards(r, c))  # clipped once, by upload
    X.set_reward_clip(c)
    for k in range(2):
        sx, sy = X.step_resident(), Y.step_resident()
        assert sx["total_loss"] == sy["total_loss"] and sx["grad_norm"] == sy["grad_norm"], k
        np.testing.assert_array_equal(X.tensor("rewards").view(np.uint32), Y.tensor("rewards").view(np.uint32))
        np.testing.assert_array_equal(X.get_params().view(np.uint32), Y.get_params().view(np.uint32))
    X.close()
    Y.close()


def test_a_nan_reward_is_still_rejected_under_the_clip():
    from freeimpala_amd._abi import FiError
    raw, _ = make_entries("mlp", B, 3, seed=610)
    raw[2, 772:776] = np.array([np.nan], np.float32).view(np.uint8)  # column 2, t = 0
    L = make_learner("mlp", 3)
    L.set_reward_clip(0.5)
    p0 = L.get_params()
    with pytest.raises(FiError, match=r"rc=-7: .*not finite"):
        L.step([r for r in raw])
    assert np.isnan(L.tensor("rewards")).sum() == 1
    np.testing.assert_array_equal(L.get_params(), p0)
    assert L.train_state()["next_update"] == 1
    L.close()


# ------------------------------------------------------------------ 5. resume
@pytest.mark.parametrize("arch,A", ARCHS)
def test_resume_continues_the_recipe(arch, A):
    def configured():
        L = make_learner(arch, A, optimizer="rmsprop", lr=2e-3)
        L.set_rmsprop(decay=0.9, momentum=0.9, eps=1e-3)
        L.set_lr_schedule(lr_end=2e-4, n_steps=4)
        L.set_reward_clip(0.5)
        return L
    data = batches_of(arch, A, 5, seed=700 + A)
    X = configured()
    for rows in data[:3]:
        X.step(rows)
    blob = X.save_state()
    Y = configured()
    assert Y.train_state()["next_update"] == 1
    Y.load_state(blob)
    assert Y.train_state() == X.train_state() and X.train_state()["next_update"] == 4
    for rows in data[3:]:
        sx, sy = X.step(rows), Y.step(rows)
        assert sx["version"] == sy["version"] and sx["total_loss"] == sy["total_loss"]
    assert X.train_state()["lr_next"] == f32(2e-4)
    np.testing.assert_array_equal(X.get_params().view(np.uint32), Y.get_params().view(np.uint32))
    for nm in ("adam_m", "adam_v"):
        a = X.tensor(nm)
        assert a.any()
        np.testing.assert_array_equal(a.view(np.uint32), Y.tensor(nm).view(np.uint32), err_msg=nm)
    X.close()
    Y.close()


# ------------------------------------------------------------------ 6. untouched handles
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_untouched_handles_report_their_configuration(optimizer):
    L = make_learner("mlp", 3, optimizer=optimizer, lr=7e-4)
    st = L.train_state()
    assert st["optimizer"] == optimizer and st["schedule_on"] == 0 and st["reward_clip"] == 0
    assert st["lr_next"] == st["lr_base"] == f32(7e-4) == float(L.cfg.lr) and st["next_update"] == 1
    L.close()


# ------------------------------------------------------------------ 7. the C++ check program
EXE = os.path.join(ROOT, "build", "host_train_check")


def test_cpp_check_program_resumes_byte_for_byte():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_train_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "OK"
