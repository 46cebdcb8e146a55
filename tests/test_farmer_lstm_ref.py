"""FarmerLstm's bf16 LSTM mode (include/fi_farmer_lstm.h) without a device: the exports, and the rule in fp64
(freeimpala_amd/farmer_lstm.py, lstm_bf16_reference) against the plain fp64 LSTM, product by product."""
import subprocess

import numpy as np


def test_exports_and_methods():
    from freeimpala_amd import _abi, farmer_lstm
    from freeimpala_amd.farmer import FarmerLstmModel
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert set(farmer_lstm.SIGNATURES) <= exported and len(farmer_lstm.SIGNATURES) == 2
    L = farmer_lstm.lib()
    assert L.fi_farmer_lstm_precision(None) == -1 and L.fi_farmer_set_lstm_precision(None, 1) == -1
    assert callable(FarmerLstmModel.set_lstm_precision) and isinstance(FarmerLstmModel.lstm_precision, property)
    assert (farmer_lstm.FP32, farmer_lstm.BF16) == (0, 1) and farmer_lstm.precision("bf16") == 1


def test_reference_rounds_every_operand_and_nothing_else():
    """(B, T) = (3, 4). u = 2^-8 is bf16's unit roundoff: a rounded operand is within u relative of its fp32 source, a
    product of two rounded operands within 2 u + u^2 of the unrounded product and a product with one within u, so a
    sum moves by at most that times S, the sum of the terms' absolute values. Each step is taken from the
    reference's own stored inputs of that step (xp_t, the handed-on h, c_{t-1}), so the bound is that of one product:
    the pre-activation moves by E = u S (h is bf16 already), a gate by its Lipschitz constant (1/4 for the sigmoids,
    1 for tanh) times E, and the stored gate by u of itself on top."""
    from freeimpala_amd import farmer_lstm as FL
    from oracle import farmer_oracle as fo
    B, T, H = 3, 4, 128
    p = fo.gen_params(4)
    z, _, _ = fo.gen_inputs(5, B, T)
    dcat = np.random.RandomState(6).standard_normal((B, H))
    ref, plain = FL.lstm_bf16_reference(z, p, dcat), FL.lstm_bf16_reference(z, p, dcat, rounded=False)
    P = FL.split_lstm_params(p)
    u = 2.0 ** -8
    S = np.abs(z.astype(np.float64)) @ np.abs(P["W_ih"]).T
    assert (np.abs(ref["xp"] - plain["xp"]) <= (2 * u + u * u) * S).all()
    pre = ref["xp"] + ref["hprev"] @ P["W_hh"].T  # the plain step from the reference's own inputs
    E = u * (np.abs(ref["hprev"]) @ np.abs(P["W_hh"]).T)
    lip = np.repeat([0.25, 0.25, 1.0, 0.25], H)
    want = np.concatenate([np.tanh(pre[..., k * H:(k + 1) * H]) if k == 2 else FL.sigmoid(pre[..., k * H:(k + 1) * H])
                           for k in range(4)], -1)
    assert (np.abs(ref["gates"] - want) <= lip * E + u * (np.abs(want) + lip * E)).all()
    # stored values are bf16 values, and the rounding is really applied
    for nm in ("gates", "hprev", "dG"):
        np.testing.assert_array_equal(FL.rne(ref[nm]), ref[nm])
        assert np.abs(ref[nm] - plain[nm]).max() > 0
    assert np.abs(ref["xp"] - plain["xp"]).max() > 1e-5 and np.abs(ref["gW_hh"] - plain["gW_hh"]).max() > 0
    # the plain LSTM is the oracle's (which adds the two biases in fp64, not in fp32): h_T against its forward
    _, saved = fo.forward(p, z, np.zeros((B, 484), np.float32))
    np.testing.assert_allclose(plain["h_T"], saved["acts"][0][:, :H], rtol=1e-6, atol=1e-7)
    for nm, sh in (("gW_ih", (512, 162)), ("gW_hh", (512, H)), ("gb", (512,)), ("dG", (B, T, 512)), ("c", (B, T, H))):
        assert ref[nm].shape == sh and np.isfinite(ref[nm]).all()
