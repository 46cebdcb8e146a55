"""FarmerLstm's bf16 LSTM mode (include/fi_farmer_lstm.h, csrc/farmer_lstm_bf16.hip) on the device: every kernel on
its own against fp64 from the tensors one SGD step leaves behind, one time step at a time, with the derived bounds
of tests/test_gpu_atari_kernels.py; run-to-run equality; the setter's rules.

The one figure that is measured, not derived: the relative error of the device's expf / tanhf in the activations.
On the parent's fp32 kernel (lstm_fwd_reg_kernel) at (B, T) = (70, 5), its fp32 gates and c against fp64 from its
own xp and hprev differ by at most 2.65e-7 relative (gates 2.65e-7, c 2.28e-7; scripts/farmer_lstm_bench.py
--activation-error prints both). ACT allows twice that on top of the derived bound of the product in front of the
activation."""
import numpy as np
import pytest

import atari_ref as R
from test_gpu_atari_kernels import check_bf16, check_f32, check_wgrad

pytestmark = pytest.mark.gpu

ACT = 2 * 2.65e-7
U = R.U32
# (B, T). The first four are the issue's: a one-row tile without a recurrent product; a full tile plus a one-row
# tile, both LDS buffers; an exact tile, the buffer parity wraps; three tiles. The last two stand on either side of
# the weight-gradient slice boundary of the kernel as built: a slice holds at least 8 chunks of 64 rows (splits =
# chunks / 8), so 950 rows (15 chunks, the last one partial) are one slice and 970 rows (16 chunks) two.
CASES = [(1, 1), (33, 2), (32, 3), (70, 5), (95, 10), (97, 10)]


def case_inputs(B, T):
    """Structured parameters: z in [0, 1); every unit u has a sign t_u; W_ih[n] shares the sign s_n of its gate
    column (+ for i, f, o; t_u for g), W_hh[n][k] = s_n t_k |w|, dense1.weight[:, u] = t_u |w|, so h_u and c_u carry
    t_u, the terms of every LSTM sum share one sign forward and backward, and pre-activations stay O(1). The forget
    gate's bias keeps c from growing with T."""
    from oracle import farmer_oracle as fo
    rs = np.random.RandomState(1000 + 7 * B + T)
    p = fo.gen_params(11).copy()
    v = fo.views(p)
    tu = np.where(rs.random_sample(128) < 0.5, 1.0, -1.0)
    sn = np.ones(512)
    sn[256:384] = tu
    v["lstm.weight_ih_l0"][:] = sn[:, None] * (0.5 + rs.random_sample((512, 162))) * (0.6 / 81)
    v["lstm.weight_hh_l0"][:] = sn[:, None] * tu[None, :] * (0.5 + rs.random_sample((512, 128))) * (0.6 / 38)
    v["lstm.bias_ih_l0"][:] = 0.05 * rs.standard_normal(512)
    v["lstm.bias_hh_l0"][:] = 0.05 * rs.standard_normal(512)
    v["lstm.bias_hh_l0"][128:256] -= 2.0  # f near 0.3: c stays below 1 at T = 10 and 1 - tanh^2(c) keeps its digits
    v["dense1.weight"][:, :128] = tu[None, :] * np.abs(v["dense1.weight"][:, :128])
    z = rs.random_sample((B, T, 162)).astype(np.float32)
    x, y = rs.standard_normal((B, 484)).astype(np.float32), rs.standard_normal((B, 1)).astype(np.float32)
    return p, z, x, y


def step(B, T, prec="bf16"):
    from freeimpala_amd.farmer import FarmerLstmModel
    p0, z, x, y = case_inputs(B, T)
    M = FarmerLstmModel(B, T, "mse", "sgd", 1e-2, params=p0)
    if prec:
        M.set_lstm_precision(prec)
    M.train_step(z, x, y)
    return M, p0, z


def terms(x, w, b=0.0):
    return x @ w + b, np.abs(x) @ np.abs(w) + np.abs(b)


def span(lo, hi):
    """An interval as check_*'s (r, S) with K = 1, c = 0: r +- u S."""
    return (lo + hi) / 2, (hi - lo) / 2 / U


def act(k, a):
    return np.tanh(a) if k == 2 else 1.0 / (1.0 + np.exp(-a))


@pytest.mark.parametrize("B,T", CASES)
def test_every_kernel_vs_fp64(B, T):
    from freeimpala_amd import farmer_lstm as FL
    from oracle import farmer_oracle as fo
    M, p0, z = step(B, T)
    assert M.lstm_precision == "bf16"
    BT, H = B * T, 128
    xp, c = M.tensor_array("xp", (B, T, 512)).astype(np.float64), M.tensor_array("cst", (B, T, H)).astype(np.float64)
    gb, hb, db = (M.tensor_array(n, (B, T, w), np.uint16) for n, w in (("gates", 512), ("hprev", H), ("dG", 512)))
    gates, hp, dG = (R.bf16_bits_to_f64(a) for a in (gb, hb, db))
    cat, dcat = M.tensor_array("h_last", (B, 612)), M.tensor_array("dcat", (B, 612)).astype(np.float64)
    g = fo.views(M.get_grads())
    M.close()
    P = FL.split_lstm_params(p0)
    W_ih, W_hh, zq = FL.rne(P["W_ih"]), FL.rne(P["W_hh"]), FL.rne(z)
    out = dict(fails=[], stats={})
    # projection
    check_f32(out, "xp", xp, terms(zq, W_ih.T, P["b"]), 176, 1)
    # forward, every (row, t) from the stored xp_t, hprev_t and c_{t-1}
    np.testing.assert_array_equal(hb[:, 0], 0)
    r, S = terms(hp, W_hh.T)
    r, e = xp + r, 129 * U * (np.abs(xp) + S)
    lo, hi = [], []
    for k in range(4):
        a, b = act(k, (r - e)[..., k * H:(k + 1) * H]), act(k, (r + e)[..., k * H:(k + 1) * H])
        lo.append(a - ACT * np.abs(a))
        hi.append(b + ACT * np.abs(b))
    check_bf16(out, "gates", gb, span(np.concatenate(lo, -1), np.concatenate(hi, -1)), 1, 0)
    cprev = np.concatenate([np.zeros((B, 1, H)), c[:, :-1]], 1)
    fc = [lo[1] * cprev, hi[1] * cprev]
    ig = [lo[0] * lo[2], lo[0] * hi[2], hi[0] * lo[2], hi[0] * hi[2]]
    rnd = 3 * U * (np.maximum(*np.abs(fc)) + np.max(np.abs(ig), 0))
    check_f32(out, "c", c, span(np.minimum(*fc) + np.min(ig, 0) - rnd, np.maximum(*fc) + np.max(ig, 0) + rnd), 1, 0)
    th = np.tanh(c)
    hs = [o * (th + s * (ACT + 2 * U) * np.abs(th)) for o in (lo[3], hi[3]) for s in (-1, 1)]
    h_lo, h_hi = np.min(hs, 0), np.max(hs, 0)
    if T > 1:
        check_bf16(out, "hprev", hb[:, 1:], span(h_lo[:, :-1], h_hi[:, :-1]), 1, 0)
    check_f32(out, "h_T", cat[:, :H], span(h_lo[:, -1], h_hi[:, -1]), 1, 0)
    # BPTT: dh_t from the stored dG_{t+1}; dc is the one carried value, with its bound carried beside it
    dh, Edh = np.zeros((B, T, H)), np.zeros((B, T, H))
    dh[:, -1] = dcat[:, :H]
    if T > 1:
        dh[:, :-1], S = terms(dG[:, 1:], W_hh)
        Edh[:, :-1] = 512 * U * S
    i, f, gg, o = (gates[..., k * H:(k + 1) * H] for k in range(4))
    rG, EG = np.zeros((B, T, 512)), np.zeros((B, T, 512))
    dc, Edc = np.zeros((B, H)), np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        it, ft, gt, ot, d, Ed, tc = i[:, t], f[:, t], gg[:, t], o[:, t], dh[:, t], Edh[:, t], th[:, t]
        a = ot * (1 - tc * tc)
        Edc = Edc + Ed * np.abs(a) + np.abs(d * ot) * (2 * ACT * tc * tc + 2 * U) + 5 * U * (np.abs(dc) + np.abs(d * a))
        dc = dc + d * a
        fac = [gt * it * (1 - it), cprev[:, t] * ft * (1 - ft), it * (1 - gt * gt)]
        rG[:, t] = np.concatenate([dc * k for k in fac] + [d * tc * ot * (1 - ot)], 1)
        EG[:, t] = np.concatenate([Edc * np.abs(k) for k in fac] + [Ed * np.abs(tc * ot * (1 - ot))], 1)
        EG[:, t] += (ACT + 4 * U) * np.abs(rG[:, t])
        dc, Edc = dc * ft, Edc * ft + U * np.abs(dc * ft)
    check_bf16(out, "dG", db, (rG, EG / U), 1, 0)
    # weight gradients
    d2 = dG.reshape(BT, 512)
    check_wgrad(out, "gW_ih", g["lstm.weight_ih_l0"], terms(d2.T, zq.reshape(BT, 162)))
    check_wgrad(out, "gW_hh", g["lstm.weight_hh_l0"], terms(d2.T, hp.reshape(BT, H)))
    check_wgrad(out, "gb", g["lstm.bias_ih_l0"].reshape(1, -1), (d2.sum(0, keepdims=True), None))
    np.testing.assert_array_equal(g["lstm.bias_hh_l0"], g["lstm.bias_ih_l0"])
    for nm, s in out["stats"].items():
        print(f"  {nm}: {s}")
    assert not out["fails"], "\n".join(out["fails"])


def test_two_runs_give_equal_bits():
    got = []
    for _ in range(2):
        M, _, _ = step(70, 5)
        got.append((M.get_grads().view(np.uint32), M.get_params().view(np.uint32)))
        M.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])


def test_setter_rules():
    from freeimpala_amd import farmer_lstm as FL
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.farmer import FarmerLstmModel
    B, T = 33, 2
    p0, z, x, y = case_inputs(B, T)
    M = FarmerLstmModel(B, T, "mse", "sgd", 1e-2, params=p0)
    assert M.lstm_precision == "fp32" and M.tensor("gates")[1] == B * T * 512 * 4 and M.tensor("dG")[1] == B * T * 512 * 4
    with pytest.raises(FiError, match="rc=-1:"):
        M.tensor("whh_bf16")
    assert FL.lib().fi_farmer_set_lstm_precision(M._h, 2) == -1
    for prec in ("bf16", "fp32", "bf16"):  # back and forth before the first step
        M.set_lstm_precision(prec)
        assert M.lstm_precision == prec
    assert M.tensor("gates")[1] == B * T * 512 * 2 and M.tensor("dG")[1] == B * T * 512 * 2
    assert M.tensor("hprev")[1] == B * T * 128 * 2 and M.tensor("wih_bf16")[1] == 512 * 176 * 2
    assert np.isfinite(M.train_step(z, x, y))
    with pytest.raises(FiError, match="rc=-4:"):
        M.set_lstm_precision("fp32")
    assert M.lstm_precision == "bf16"
    M.close()
