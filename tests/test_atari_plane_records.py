"""Single-plane Atari records on the host side: the pack / unpack pair, the
entry-size arithmetic and stack_planes, the sequential frame-stack rule the device ingest is held
to (tests/test_gpu_atari_planes.py). No GPU here.
"""
import numpy as np
import pytest

REC, PLANE, HIST = 7168, 84 * 84, 21504


def rand_planes(T, B, A, seed, density=0.3):
    rs = np.random.RandomState(seed)
    planes = rs.randint(0, 256, (T + 1, B, 84, 84)).astype(np.uint8)
    history = rs.randint(0, 256, (3, B, 84, 84)).astype(np.uint8)
    start = rs.rand(T + 1, B) < density
    mu = rs.randn(T, B, A).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.randint(-1, 2, (T, B)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.1)).astype(np.float32)
    return planes, history, start, mu, act, rew, disc


def closed_form(planes, history, start):
    """The rule as DESIGN.md section 3 states it: channel c of frame t has nominal source time
    s = t-3+c; with r the last episode_start in [0, t], s < r reads p_r, else s < 0 reads h_{s+3},
    else p_s."""
    T1, B = planes.shape[:2]
    out = np.empty((T1, B, 84, 84, 4), np.uint8)
    for b in range(B):
        for t in range(T1):
            rr = [k for k in range(t + 1) if start[k, b]]
            r = rr[-1] if rr else None
            for c in range(4):
                s = t - 3 + c
                if r is not None and s < r:
                    src = planes[r, b]
                elif s < 0:
                    src = history[s + 3, b]
                else:
                    src = planes[s, b]
                out[t, b, :, :, c] = src
    return out


def test_signatures_present():
    from freeimpala_amd import _abi
    assert "fi_ingest_atari_planes" in _abi.SIGNATURES
    assert "fi_learner_set_record_format" in _abi.SIGNATURES
    assert _abi.ATARI_PLANE_RECORD_BYTES == REC == 7 * 1024 and _abi.ATARI_HISTORY_BYTES == HIST == 21 * 1024
    assert _abi.ATARI_PLANE_BYTES == PLANE == 16 * 441
    assert (_abi.FI_RECORDS_STACKED, _abi.FI_RECORDS_PLANES) == (0, 1)


def test_header_constants_match_the_c_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fi_learner.h")).read()
    want = {"FI_ATARI_PLANE_RECORD_ELEMENTS": 7, "FI_ATARI_PLANE_RECORD_BYTES": 7168,
            "FI_ATARI_HISTORY_ELEMENTS": 21, "FI_ATARI_HISTORY_BYTES": 21504}
    for name, val in want.items():
        m = re.search(rf"#define\s+{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    assert re.search(r"FI_RECORDS_STACKED\s*=\s*0\s*,\s*FI_RECORDS_PLANES\s*=\s*1", hdr)


@pytest.mark.parametrize("T", [1, 2, 5, 100])
def test_entry_size_arithmetic(T):
    from freeimpala_amd.learner import pack_atari_plane_records, plane_entry_elements
    assert plane_entry_elements(T) == 7 * (T + 1) + 21
    assert plane_entry_elements(T) * 1024 == (T + 1) * REC + HIST == 1024 * (7 * T + 28)
    assert (1024 * (7 * T + 28)) % 16 == 0
    if T <= 5:
        src = rand_planes(T, 2, 6, seed=T)
        e = pack_atari_plane_records(*src)
        assert len(e) == 2 and all(len(x) == 1024 * (7 * T + 28) for x in e)
        with pytest.raises(ValueError, match=rf"{7 * (T + 1) + 21} = 7\*\(T\+1\)\+21"):
            pack_atari_plane_records(*src, entry_size=7 * (T + 1) + 20)


def test_more_than_18_actions_do_not_fit_the_header():
    from freeimpala_amd.learner import pack_atari_plane_records
    with pytest.raises(ValueError, match="mu\\[18\\]"):
        pack_atari_plane_records(*rand_planes(1, 1, 19, seed=0))
    pack_atari_plane_records(*rand_planes(1, 1, 18, seed=0))


@pytest.mark.parametrize("T,B,A,spare", [(1, 1, 6, 0), (2, 3, 18, 0), (3, 2, 6, 5)])
def test_pack_unpack_round_trip(T, B, A, spare):
    """Round trip with a spare tail; the reserved bytes, the flags, mu's unused slots, the header
    of record T (but its episode_start), the history padding and the entry padding are poisoned
    and must not show in what unpack returns."""
    from freeimpala_amd.learner import pack_atari_plane_records, unpack_atari_plane_records
    src = rand_planes(T, B, A, seed=10 * T + B)
    S = 7 * (T + 1) + 21 + spare
    raw = np.stack([np.frombuffer(e, np.uint8) for e in pack_atari_plane_records(*src, entry_size=S)]).copy()
    assert raw.shape == (B, S * 1024)
    # the layout, byte for byte, for entry 0
    np.testing.assert_array_equal(raw[0, REC:REC + PLANE], src[0][1, 0].ravel())
    np.testing.assert_array_equal(raw[0, (T + 1) * REC + PLANE:(T + 1) * REC + 2 * PLANE], src[1][1, 0].ravel())
    np.testing.assert_array_equal(raw[0, 7056:7056 + 4 * A].view(np.float32), src[3][0, 0])
    assert raw[0, 7128:7132].view(np.int32)[0] == src[4][0, 0]
    assert raw[0, 7132:7136].view(np.float32)[0] == src[5][0, 0]
    assert raw[0, 7136:7140].view(np.float32)[0] == src[6][0, 0]
    assert raw[0, T * REC + 7144:T * REC + 7148].view(np.uint32)[0] == int(src[2][T, 0])
    rec = raw[:, :(T + 1) * REC].reshape(B, T + 1, REC)
    rec[:, :, 7148:] = 0xDD                       # reserved
    rec[:, :, 7140:7144] = 0xDD                   # flags
    rec[:, T, PLANE:7144] = 0xEE                  # record T: only its plane and episode_start count
    rec[:, :T, PLANE + 4 * A:7128] = 0xCC         # mu slots past A
    raw[:, (T + 1) * REC + 3 * PLANE:(T + 1) * REC + HIST] = 0xBB  # history padding
    raw[:, (T + 1) * REC + HIST:] = 0xFF          # entry padding
    for form in (raw, [r.tobytes() for r in raw], raw.tobytes()):
        got = unpack_atari_plane_records(form, T, B, A)
        assert len(got) == 7
        for g, w, nm in zip(got, src, ("planes", "history", "episode_start", "mu", "actions", "rewards", "discounts")):
            assert g.dtype == w.dtype and g.shape == w.shape, nm
            np.testing.assert_array_equal(g, w, err_msg=nm)
    with pytest.raises(ValueError):
        unpack_atari_plane_records(raw[:, :(T + 1) * REC + HIST - 16], T, B, A)


def _planes(T):
    """T+1 planes and 3 history planes, each a constant: p_t = 10 + t, h_i = 200 + i."""
    planes = np.stack([np.full((1, 84, 84), 10 + t, np.uint8) for t in range(T + 1)])
    history = np.stack([np.full((1, 84, 84), 200 + i, np.uint8) for i in range(3)])
    return planes, history


def _channels(frames, t):
    f = frames[t, 0]
    assert (f == f[0, 0]).all()  # every pixel holds the same four channel values
    return [int(x) for x in f[0, 0]]


def _starts(T, *at):
    s = np.zeros((T + 1, 1), bool)
    for t in at:
        s[t, 0] = True
    return s


H0, H1, H2 = 200, 201, 202
P = [10 + t for t in range(8)]


def test_stack_planes_no_starts_reads_the_history():
    from freeimpala_amd.learner import stack_planes
    planes, history = _planes(1)
    fr = stack_planes(planes, history, _starts(1))
    assert fr.shape == (2, 1, 84, 84, 4) and fr.dtype == np.uint8
    assert _channels(fr, 0) == [H0, H1, H2, P[0]]
    assert _channels(fr, 1) == [H1, H2, P[0], P[1]]
    planes, history = _planes(4)
    fr = stack_planes(planes, history, _starts(4))
    assert _channels(fr, 2) == [H2, P[0], P[1], P[2]]
    assert _channels(fr, 3) == [P[0], P[1], P[2], P[3]]  # the first frame without history
    assert _channels(fr, 4) == [P[1], P[2], P[3], P[4]]


def test_stack_planes_start_at_zero_ignores_the_history():
    from freeimpala_amd.learner import stack_planes
    planes, history = _planes(3)
    fr = stack_planes(planes, history, _starts(3, 0))
    assert _channels(fr, 0) == [P[0]] * 4
    assert _channels(fr, 1) == [P[0], P[0], P[0], P[1]]
    assert _channels(fr, 2) == [P[0], P[0], P[1], P[2]]
    assert _channels(fr, 3) == [P[0], P[1], P[2], P[3]]
    other = stack_planes(planes, history[::-1] + 1, _starts(3, 0))
    np.testing.assert_array_equal(fr, other)


def test_stack_planes_start_mid_entry():
    from freeimpala_amd.learner import stack_planes
    planes, history = _planes(4)
    fr = stack_planes(planes, history, _starts(4, 2))
    assert _channels(fr, 0) == [H0, H1, H2, P[0]]
    assert _channels(fr, 1) == [H1, H2, P[0], P[1]]
    assert _channels(fr, 2) == [P[2]] * 4
    assert _channels(fr, 3) == [P[2], P[2], P[2], P[3]]
    assert _channels(fr, 4) == [P[2], P[2], P[3], P[4]]


def test_stack_planes_consecutive_starts():
    from freeimpala_amd.learner import stack_planes
    planes, history = _planes(4)
    fr = stack_planes(planes, history, _starts(4, 1, 2))
    assert _channels(fr, 1) == [P[1]] * 4
    assert _channels(fr, 2) == [P[2]] * 4
    assert _channels(fr, 3) == [P[2], P[2], P[2], P[3]]


def test_stack_planes_start_on_the_bootstrap_record():
    from freeimpala_amd.learner import stack_planes
    planes, history = _planes(2)
    fr = stack_planes(planes, history, _starts(2, 2))
    assert _channels(fr, 1) == [H1, H2, P[0], P[1]]
    assert _channels(fr, 2) == [P[2]] * 4


def test_stack_planes_is_nhwc_and_per_entry():
    """Random planes, several entries with different start patterns: byte c of pixel (y, x) of
    frame (t, b) is channel c, against the closed-form statement of the rule."""
    from freeimpala_amd.learner import stack_planes
    planes, history, start = rand_planes(6, 5, 6, seed=3)[:3]
    assert start.any() and not start.all()
    fr = stack_planes(planes, history, start)
    np.testing.assert_array_equal(fr, closed_form(planes, history, start))
    np.testing.assert_array_equal(fr[..., 3], planes)  # channel 3 is always the newest plane
    # integer flags count as booleans
    np.testing.assert_array_equal(stack_planes(planes, history, start.astype(np.uint32) * 7), fr)
