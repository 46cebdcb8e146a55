"""The fc data gradient's default kernel (W in registers, only dh through LDS:
fc_dgrad_wreg_kernel) against the LDS-ring kernel it replaced (FI_FC_DGRAD_RING=1), bit for bit.

Both run the same MFMA with W on the A side, dh on the B side and k ascending in steps of 32, so
da3 and every gradient computed from it must be identical. One full Atari step per kernel on the
same synthetic batch. The kernel walks the first T * B frames (the bootstrap frames carry no
gradient), 64 rows per slot, 19 streams:

  N = (T + 1) B of 21, 64, 65, 1,216 and 3,653 frames (one ragged slot with 18 streams empty; one
  slot; one slot plus a row; one slot per stream; three slots per stream plus a ragged fourth, so
  the two LDS slots wrap), and the same counts as the kernel's own row count T * B (T = 1), where
  exactly 64, 65 and 1,216 rows meet the slot edges. Every case runs the last column slice, in
  which six of the eight waves own no columns. Rows past T * B must stay the zeros of creation.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 7), (1, 32), (4, 13), (18, 64), (12, 281),   # N = 21, 64, 65, 1216, 3653
         (1, 21), (1, 64), (1, 65), (1, 1216), (1, 3653)]  # T * B = the same counts


def _step(T, B, ring, monkeypatch):
    from freeimpala_amd.learner import DeviceLearner
    if ring:
        monkeypatch.setenv("FI_FC_DGRAD_RING", "1")
    else:
        monkeypatch.delenv("FI_FC_DGRAD_RING", raising=False)
    L = DeviceLearner("atari", seq_len=T, batch=B, num_actions=18, optimizer="sgd", lr=1e-3, max_grad_norm=0.0, seed=4)
    L.synth(seed=31)
    L.step_resident()
    N = (T + 1) * B
    out = (L.tensor("dh", np.uint16, (N, 512)), L.tensor("da3", np.uint16, (N, 3136)), L.tensor("grads"))
    L.close()
    return out


@pytest.mark.parametrize("T,B", CASES)
def test_wreg_dgrad_is_bit_identical_to_the_ring_kernel(T, B, monkeypatch):
    dh0, da3_ring, g_ring = _step(T, B, True, monkeypatch)
    dh1, da3, g = _step(T, B, False, monkeypatch)
    np.testing.assert_array_equal(dh0, dh1)  # same input to both kernels
    assert dh1[:T * B].any()
    np.testing.assert_array_equal(da3, da3_ring)
    np.testing.assert_array_equal(g, g_ring)
    assert da3[:T * B].any() and not da3[T * B:].any()
    # every row slot and every 32-column unit was written (a missed one would still hold zeros)
    live = dh1[:T * B].any(axis=1)
    assert da3[:T * B][live].reshape(-1, 98, 32).any(axis=2).all()
