"""FarmerLstm's acting branch (include/fi_farmer_act.h, csrc/farmer_act.hip) on the device: h against the bf16
learner's, bit for bit; every layer of the torso and the value against fp64 from the tensors the traced call stores,
with the derived (K + c) u S intervals of tests/test_gpu_atari_kernels.py; the pick against pick_reference on the
device's own values, exactly; bit equality; the refusals. No measured tolerance anywhere."""
import numpy as np
import pytest

import atari_ref as R
from test_gpu_atari_kernels import check_bf16, check_f32
from test_gpu_farmer_lstm_bf16 import case_inputs as lstm_inputs

pytestmark = pytest.mark.gpu

RANDOM_SIZES = [int(n) for n in np.random.RandomState(5).randint(0, 10, 40)]
# (T, segment sizes): one row of a partial tile without a recurrent product; the 32-row boundary; a full 64-row tile
# plus a partial one with a decision point across the tile edge; exact tiles; more candidates than lanes in the pick
# and a partial fourth tile; two LSTM batch tiles with empty decision points
CASES = [(1, [1]), (2, [33]), (2, [1, 64, 5]), (3, [64, 64]), (2, [200]), (5, RANDOM_SIZES)]


def case_inputs(T, sizes):
    """The LSTM part of test_gpu_farmer_lstm_bf16.case_inputs (h_u carries the sign t_u); x in [0, 1); dense1's
    h-columns carry t_u and every other torso weight is (0.5 + rand) c / K >= 0, so no sum cancels: c = 2 into layer
    1 (its inputs average below 1/2) and 1.1 behind it keep the activations O(1). Biases 0.02 N(0, 1)."""
    from oracle import farmer_oracle as fo
    S, N = len(sizes), sum(sizes)
    p, z, _, _ = lstm_inputs(S, T)
    v = fo.views(p)
    rs = np.random.RandomState(300 + 11 * N + T)
    tu = np.sign(v["dense1.weight"][0, :128])
    v["dense1.weight"][:] = (0.5 + rs.random_sample((512, 612))) * (2.0 / 612)
    v["dense1.weight"][:, :128] *= tu[None, :]
    for l in range(2, 6):
        v[f"dense{l}.weight"][:] = (0.5 + rs.random_sample((512, 512))) * (1.1 / 512)
    v["dense6.weight"][:] = (0.5 + rs.random_sample((1, 512))) * (1.1 / 512)
    for l in range(1, 7):
        v[f"dense{l}.bias"][:] = 0.02 * rs.standard_normal(v[f"dense{l}.bias"].shape)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return p, z, rs.random_sample((N, 484)).astype(np.float32), offsets


def make_actor(T, sizes, p, **kw):
    from freeimpala_amd.farmer_act import FarmerActor
    A = FarmerActor(len(sizes), max(1, sum(sizes)), T, **kw)
    A.set_params(p)
    return A


@pytest.mark.parametrize("T,sizes", CASES, ids=[f"T{T}_S{len(s)}_N{sum(s)}" for T, s in CASES])
def test_every_stage_vs_fp64(T, sizes):
    from freeimpala_amd import farmer_act as FA
    from freeimpala_amd.farmer import FarmerLstmModel
    S, N = len(sizes), sum(sizes)
    p, z, x, offsets = case_inputs(T, sizes)
    A = make_actor(T, sizes, p, seed=3)
    A.set_trace(True)
    got = A.act(z, x, offsets, 0.0)
    h, trace = A.tensor_array("h")[:S, :128], A.tensor_array("trace")
    assert A.nonfinite == 0
    A.close()
    M = FarmerLstmModel(S, T, params=p)
    M.set_lstm_precision("bf16")
    M(z, np.zeros((S, 484), np.float32))
    np.testing.assert_array_equal(h.view(np.uint32), M.tensor_array("h_last", (S, 612))[:, :128].view(np.uint32))
    M.close()
    out = dict(fails=[], stats={})
    P = FA.split_torso_params(p)
    a = np.concatenate([FA.rne(h)[FA.row_table(offsets)], FA.rne(x)], 1)
    for l in range(5):
        check_bf16(out, f"a{l + 1}", trace[l], FA.layer_terms(a, *P[l]), 624 if l == 0 else 512, 1, relu=True)
        a = R.bf16_bits_to_f64(trace[l])
    w6, b6 = P[5]
    check_f32(out, "values", got["values"], (a @ w6 + b6, np.abs(a) @ np.abs(w6) + abs(b6)), 512, 1)
    for nm, s in out["stats"].items():
        print(f"  {nm}: {s}")
    assert not out["fails"], "\n".join(out["fails"])
    ref = FA.pick_reference(got["values"], offsets, 0.0, 3, 0)
    for k in ("actions", "explored", "best_value"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


def test_exploration_matches_the_reference_draw_by_draw():
    from freeimpala_amd.farmer_act import pick_reference
    sizes = [int(n) for n in np.random.RandomState(9).randint(0, 12, 64)]
    p, z, x, offsets = case_inputs(2, sizes)
    eps = np.tile(np.float32([0.0, 1.0, 0.5]), 22)[:64]
    A = make_actor(2, sizes, p, seed=2 ** 40 + 5)
    seen = []
    for draw in range(2):
        got = A.act(z, x, offsets, eps)
        ref = pick_reference(got["values"], offsets, eps, 2 ** 40 + 5, draw)
        for k in ("actions", "explored", "best_value"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{k}, draw {draw}")
        assert not got["explored"][eps == 0].any()
        assert (got["explored"][eps == 1] == (np.diff(offsets)[eps == 1] > 0)).all()
        seen.append(got["actions"])
    assert (seen[0] != seen[1]).any()  # the second call draws other words
    A.close()


def test_ties_take_the_lowest_row_and_a_nan_row_is_never_picked():
    from oracle import farmer_oracle as fo
    sizes = [3, 0, 70, 1, 2]
    p, z, x, offsets = case_inputs(2, sizes)
    v = fo.views(p)
    for l in range(1, 7):
        v[f"dense{l}.weight"][:] = 0
        v[f"dense{l}.bias"][:] = 0
    v["dense6.bias"][:] = 1
    A = make_actor(2, sizes, p)
    got = A.act(z, x, offsets)
    np.testing.assert_array_equal(got["values"], np.ones(76, np.float32))
    np.testing.assert_array_equal(got["actions"], [0, -1, 0, 0, 0])
    x[3, 17] = np.nan  # row 0 of the 70-row decision point
    bad = A.act(z, x, offsets)
    assert np.isnan(bad["values"][3]) and A.nonfinite == 1
    np.testing.assert_array_equal(np.delete(bad["values"], 3), np.ones(75, np.float32))
    np.testing.assert_array_equal(bad["actions"], [0, -1, 1, 0, 0])
    A.close()


def test_bit_equality_across_trace_runs_and_parameter_routes():
    from freeimpala_amd.farmer import FarmerLstmModel
    T, sizes = 2, [1, 64, 5]
    p, z, x, offsets = case_inputs(T, sizes)
    A = make_actor(T, sizes, p)
    plain = A.act(z, x, offsets)["values"].view(np.uint32)
    np.testing.assert_array_equal(A.act(z, x, offsets)["values"].view(np.uint32), plain)
    A.set_trace(True)
    np.testing.assert_array_equal(A.act(z, x, offsets)["values"].view(np.uint32), plain)
    A.set_trace(False)
    M = FarmerLstmModel(70, T, "mse", "sgd", 1e-2, params=p)
    rs = np.random.RandomState(1)
    M.train_step(rs.random_sample((70, T, 162)), x, rs.standard_normal((70, 1)))
    A.set_params_from(M)
    dev = A.act(z, x, offsets)["values"].view(np.uint32)
    np.testing.assert_array_equal(A.tensor_array("params").view(np.uint32), M.get_params().view(np.uint32))
    A.set_params(M.get_params())
    np.testing.assert_array_equal(A.act(z, x, offsets)["values"].view(np.uint32), dev)
    assert (dev != plain).any()  # the step moved the parameters
    M.close()
    A.close()


def test_refusals_leave_the_handle_usable():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.farmer_act import FarmerActor
    T, sizes = 2, [2, 3]
    p, z, x, offsets = case_inputs(T, sizes)
    A = FarmerActor(2, 5, T)
    with pytest.raises(FiError, match="rc=-4:"):
        A.act(z, x, offsets)
    A.set_params(p)
    want = A.act(z, x, offsets)
    z3, x6 = np.concatenate([z, z[:1]]), np.concatenate([x, x[:1]])
    for zz, xx, off, eps in [(z3, x, [0, 2, 3, 5], 0.0),              # S above max_states
                             (z, x6, [0, 2, 6], 0.0),                 # N above max_rows
                             (z, x[:3], [1, 2, 3], 0.0),              # offsets[0] is not 0
                             (z, x[:1], [0, 2, 1], 0.0),              # offsets decrease
                             (z, x, offsets, 1.5), (z, x, offsets, -0.1), (z, x, offsets, np.nan),
                             (z, x, offsets, np.float32([0.5, np.nan]))]:
        with pytest.raises(FiError, match="rc=-1:"):
            A.act(zz, xx, off, eps)
    again = A.act(z, x, offsets)
    for k in want:
        np.testing.assert_array_equal(again[k], want[k], err_msg=k)
    A.close()
