"""The Atari policy fed from single-plane records (7-element records + a 3-plane history block,
DESIGN.md section 3): the planes ingest kernel alone against stack_planes, and every host entry
point on a records="planes" handle against a stacked handle fed the stacked form of the same
batch. The ingest is a byte shuffle, so everything here is bit-exact.
"""
import numpy as np
import pytest

from test_atari_plane_records import rand_planes

pytestmark = pytest.mark.gpu

REC, PLANE, HIST, FRAME = 7168, 84 * 84, 21504, 84 * 84 * 4
# ingest_planes_kernel (csrc/ingest_kernels.h) launches 7 one-wave workgroups per entry (runs of 64 of a
# plane's 441 16-byte pieces) with no grid cap and walks all of T in one pass: no grid-stride
# wrap and no segment boundary to cover. (1, 300) puts 2,100 workgroups on the device.
PLANE_RUNS = 7
SHAPES = [(1, 1), (2, 7), (3, 32), (6, 5), (1, 300)]


def mk(T, B, A=18, **kw):
    from freeimpala_amd.learner import DeviceLearner
    kw.setdefault("optimizer", "sgd")
    kw.setdefault("lr", 1e-3)
    kw.setdefault("max_grad_norm", 0.0)
    return DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, **kw)


def resident(L, T, B, A):
    return (L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4)), L.tensor("mu", shape=(T, B, A)),
            L.tensor("actions", np.int32, (T, B)), L.tensor("rewards", shape=(T, B)),
            L.tensor("discounts", shape=(T, B)))


def draw(T, B, A, mode):
    """A batch whose episode_start is all zero, all ones, or random at 30 % density. The random
    draw must hold a start at 0, a start at T and two consecutive starts, and an entry without a
    start at 0 (whose first frames read the history); (1, 1) has two flags only: it is drawn
    without a start, so the history feeds both of its frames."""
    src = list(rand_planes(T, B, A, seed=T * 1000 + B))
    if mode == "zeros" or (T, B) == (1, 1):
        src[2] = np.zeros((T + 1, B), bool)
    elif mode == "ones":
        src[2] = np.ones((T + 1, B), bool)
    else:
        s = src[2]
        assert s[0].any() and not s[0].all(), "starts at 0, and entries that read the history"
        assert s[T].any(), "a start on the bootstrap record"
        assert (s[1:] & s[:-1]).any(), "consecutive starts"
        assert (s[1:T] & ~s[:T - 1]).any() if T >= 2 else True, "a start after a step without one"
        assert 0.15 < s.mean() < 0.45
    return tuple(src)


def stacked_of(src):
    from freeimpala_amd.learner import stack_planes
    return (stack_planes(*src[:3]),) + tuple(src[3:])


CASES = [(T, B, "random") for T, B in SHAPES] + [(2, 7, "zeros"), (2, 7, "ones"), (3, 32, "ones")]


@pytest.mark.parametrize("spare", [0, 5])
@pytest.mark.parametrize("T,B,mode", CASES)
def test_standalone_planes_ingest_is_bit_exact(T, B, mode, spare):
    """fi_ingest_atari_planes on uploaded entries: frames equal stack_planes, mu / actions /
    rewards / discounts come out as packed, bit for bit. Every byte the kernels must not use is
    poisoned first -- the header of record T except its episode_start, the flags and reserved
    bytes of every record, mu's slots past A, the history padding, the entry padding -- and the
    outputs sit between guard words that must survive."""
    from freeimpala_amd import hip
    from freeimpala_amd._abi import FiError, check, lib
    from freeimpala_amd.learner import pack_atari_plane_records
    A = 6
    src = draw(T, B, A, mode)
    want = stacked_of(src)
    S = 7 * (T + 1) + 21 + spare
    raw = np.stack([np.frombuffer(e, np.uint8) for e in pack_atari_plane_records(*src, entry_size=S)]).copy()
    assert raw.shape == (B, S * 1024) and raw.nbytes < 100e6 and want[0].nbytes < 100e6
    rec = raw[:, :(T + 1) * REC].reshape(B, T + 1, REC)
    rec[:, T, PLANE:7144] = 0xEE                      # record T: its plane and episode_start only
    rec[:, :, 7140:7144] = 0xDD                       # flags
    rec[:, :, 7148:] = 0xDD                           # reserved
    rec[:, :T, PLANE + 4 * A:7128] = 0xCC             # mu slots past A
    raw[:, (T + 1) * REC + 3 * PLANE:(T + 1) * REC + HIST] = 0xBB  # history padding
    raw[:, (T + 1) * REC + HIST:] = 0xFF              # entry padding
    dev = hip.DeviceBuffer.from_array(raw)
    G = 64  # guard bytes on both sides of every output
    shapes = [((T + 1) * B * FRAME, np.uint8), (T * B * A, np.float32), (T * B, np.int32),
              (T * B, np.float32), (T * B, np.float32)]
    bufs = []
    for n, dt in shapes:
        nb = n * np.dtype(dt).itemsize
        b = hip.DeviceBuffer(nb + 2 * G)
        b.upload(np.full(nb + 2 * G, 0xA5, np.uint8))
        bufs.append((b, nb))
    ptr = [b.ptr + G for b, _ in bufs]
    check(lib().fi_ingest_atari_planes(dev.ptr, T, B, A, S * 1024, *ptr, None), "fi_ingest_atari_planes")
    hip.synchronize()
    for (b, nb), (n, dt), w, nm in zip(bufs, shapes, want, ("frames", "mu", "actions", "rewards", "discounts")):
        got = b.download(np.uint8, (nb + 2 * G,))
        assert (got[:G] == 0xA5).all() and (got[G + nb:] == 0xA5).all(), nm + ": guard overwritten"
        np.testing.assert_array_equal(got[G:G + nb].view(dt).reshape(w.shape), w, err_msg=nm)
    # what the launcher must refuse before any kernel runs
    need = (T + 1) * REC + HIST
    assert need == 1024 * (7 * T + 28)
    with pytest.raises(FiError, match=str(need)):
        check(lib().fi_ingest_atari_planes(dev.ptr, T, B, A, need - 16, *ptr, None), "ingest")
    with pytest.raises(FiError, match="multiple of 16"):
        check(lib().fi_ingest_atari_planes(dev.ptr, T, B, A, S * 1024 + 8, *ptr, None), "ingest")
    with pytest.raises(FiError, match="18"):
        check(lib().fi_ingest_atari_planes(dev.ptr, T, B, 19, S * 1024, *ptr, None), "ingest")
    with pytest.raises(FiError, match="null"):
        check(lib().fi_ingest_atari_planes(dev.ptr, T, B, A, S * 1024, None, *ptr[1:], None), "ingest")
    with pytest.raises(FiError, match="aligned"):
        check(lib().fi_ingest_atari_planes(dev.ptr + 4, T, B, A, S * 1024, *ptr, None), "ingest")
    with pytest.raises(FiError, match="bad shape"):
        check(lib().fi_ingest_atari_planes(dev.ptr, 0, B, A, S * 1024, *ptr, None), "ingest")
    hip.synchronize()
    for (b, nb), nm in zip(bufs, ("frames", "mu", "actions", "rewards", "discounts")):  # nothing ran
        got = b.download(np.uint8, (nb + 2 * G,))
        assert (got[:G] == 0xA5).all() and (got[G + nb:] == 0xA5).all(), nm + ": guard overwritten by a refused call"
    for b, _ in bufs + [(dev, 0)]:
        b.free()


LOSS_KEYS = ("pg_loss", "baseline_loss", "entropy_loss", "total_loss", "grad_norm", "version")
_batches = {}
_stacked_runs = {}


def batch_of(T, B):
    """One plane batch per shape and its stacked form, shared and read-only."""
    if (T, B) not in _batches:
        src = draw(T, B, 18, "random")
        stk = stacked_of(src)
        for v in src + stk:
            v.setflags(write=False)
        _batches[(T, B)] = (src, stk)
    return _batches[(T, B)]


def stacked_run(T, B, opt, steps):
    """Handle X: a stacked-records handle stepped on pack_atari_records(stack_planes(...)),
    once per configuration."""
    from freeimpala_amd.learner import pack_atari_records
    key = (T, B, opt)
    if key not in _stacked_runs:
        A = 18
        X = mk(T, B, A, optimizer=opt, seed=5)
        entries = pack_atari_records(*batch_of(T, B)[1])
        stats = [X.step(entries) for _ in range(steps)]
        out = dict(stats=stats, batch=resident(X, T, B, A), grads=X.tensor("grads"), logits=X.tensor("logits"),
                   values=X.tensor("values"), params=X.get_params())
        X.close()
        for v in out["batch"] + (out["grads"], out["logits"], out["values"], out["params"]):
            v.setflags(write=False)
        _stacked_runs[key] = out
    return _stacked_runs[key]


def feed(Y, entries, how):
    if how == "step":
        return Y.step(entries)
    if how == "async":
        Y.step_async(entries)
        return Y.wait()
    buf = Y.acquire_staging()
    assert buf.shape == (Y.B, Y.entry_bytes)
    for b, e in enumerate(entries):
        buf[b] = np.frombuffer(e, np.uint8)[:Y.entry_bytes]
    if how == "staged":
        return Y.step_staged()
    Y.step_staged_async()
    return Y.wait()


@pytest.mark.parametrize("how", ["step", "async", "staged", "staged_async"])
@pytest.mark.parametrize("opt,steps", [("sgd", 1), ("adam", 2)])
@pytest.mark.parametrize("T,B", [(2, 7), (3, 32)])
def test_planes_fed_step_equals_stacked_fed_step(T, B, opt, steps, how):
    from freeimpala_amd.learner import pack_atari_plane_records
    A = 18
    ref = stacked_run(T, B, opt, steps)
    src, stk = batch_of(T, B)
    Y = mk(T, B, A, optimizer=opt, seed=5, records="planes")
    assert Y.record_bytes == 7168 and Y.entry_bytes == 1024 * (7 * T + 28)
    # one spare element per entry on the step / async paths (only the first entry_bytes are read)
    entries = pack_atari_plane_records(*src, entry_size=7 * (T + 1) + 21 + (how in ("step", "async")))
    for k in range(steps):
        st = feed(Y, entries, how)
        for key in LOSS_KEYS:
            assert st[key] == ref["stats"][k][key], (k, key, st[key], ref["stats"][k][key])
    for got, want, mine in zip(resident(Y, T, B, A), ref["batch"], stk):
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, mine)
    for nm in ("grads", "logits", "values"):
        np.testing.assert_array_equal(Y.tensor(nm), ref[nm], err_msg=nm)
    np.testing.assert_array_equal(Y.get_params(), ref["params"])
    Y.close()


def test_async_steps_double_buffer():
    """Three different batches through step_async back to back, then one wait: the parameters
    equal three serial steps' bit for bit (a staging slot reused before its ingest had run, or a
    frames tensor rewritten under a running step, would change them)."""
    from freeimpala_amd.learner import pack_atari_plane_records
    T, B, A = 2, 7, 18
    batches = [pack_atari_plane_records(*rand_planes(T, B, A, seed=100 + k)) for k in range(3)]
    S = mk(T, B, A, optimizer="adam", seed=9, records="planes")
    serial = [S.step(e) for e in batches]
    Y = mk(T, B, A, optimizer="adam", seed=9, records="planes")
    for e in batches:
        Y.step_async(e)
    last = Y.wait()
    np.testing.assert_array_equal(Y.get_params(), S.get_params())
    np.testing.assert_array_equal(Y.tensor("grads"), S.tensor("grads"))
    for key in LOSS_KEYS:
        assert last[key] == serial[-1][key], key
    assert last["version"] == 3
    S.close()
    Y.close()


def test_format_selection():
    from freeimpala_amd import _abi
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import DeviceLearner, pack_atari_plane_records, pack_atari_records
    T, B = 2, 4
    M = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=6, obs_dim=8, hidden=16)
    for fmt in (_abi.FI_RECORDS_STACKED, _abi.FI_RECORDS_PLANES):
        with pytest.raises(FiError, match="rc=-1"):
            M.set_record_format(fmt)
    assert M.record_bytes == 1024 and M.entry_bytes == (T + 1) * 1024
    M.close()
    with pytest.raises(FiError, match="rc=-1"):
        DeviceLearner("mlp", seq_len=T, batch=B, num_actions=6, obs_dim=8, hidden=16, records="planes")
    with pytest.raises(ValueError):
        mk(T, B, records="plane")
    # the plane header holds mu[18]. fi_learner_set_record_format checks A <= 18 itself, but no
    # Atari handle with more actions exists to show it: the Atari net's own create refuses
    # A > 18 first (the standalone ingest's refusal of A = 19 is tested above)
    with pytest.raises(FiError, match=r"rc=-1: .*18"):
        mk(T, B, A=19, records="planes")
    Y = mk(T, B)
    assert Y.record_bytes == 28672  # the default is stacked
    with pytest.raises(FiError, match="rc=-1"):
        Y.set_record_format(2)
    Y.set_record_format(_abi.FI_RECORDS_PLANES)
    assert Y.record_bytes == 7168 and Y.entry_bytes == 1024 * (7 * T + 28)
    Y.set_record_format(_abi.FI_RECORDS_STACKED)
    assert Y.record_bytes == 28672 and Y.entry_bytes == (T + 1) * 28672
    Y.set_record_format(_abi.FI_RECORDS_PLANES)
    Y.step_resident()  # no host batch yet: the format is still open
    Y.set_record_format(_abi.FI_RECORDS_PLANES)
    Y.step(pack_atari_plane_records(*rand_planes(T, B, 18, seed=1)))
    for fmt in (_abi.FI_RECORDS_STACKED, _abi.FI_RECORDS_PLANES):
        with pytest.raises(FiError, match="rc=-4"):
            Y.set_record_format(fmt)
    assert Y.record_bytes == 7168
    Y.close()
    # and the other way round: a stacked handle that has taken a host batch stays stacked
    X = mk(T, B)
    src = rand_planes(T, B, 18, seed=1)
    X.step(pack_atari_records(*stacked_of(src)))
    with pytest.raises(FiError, match="rc=-4"):
        X.set_record_format(_abi.FI_RECORDS_PLANES)
    assert X.record_bytes == 28672
    X.close()


def test_entry_bytes_too_small_is_refused():
    from freeimpala_amd._abi import FiError
    T, B = 2, 4
    Y = mk(T, B, records="planes")
    need = 1024 * (7 * T + 28)
    short = [b"\0" * (need - 1024)] * B
    p0 = Y.get_params()
    with pytest.raises(FiError, match=rf"rc=-1: .*{need}"):
        Y.step(short)
    with pytest.raises(FiError, match=rf"rc=-1: .*{need}"):
        Y.step_async(short)
    np.testing.assert_array_equal(Y.get_params(), p0)
    assert Y.get_blob()[1] == 0
    Y.step([b"\0" * need] * B)  # the minimum is accepted
    Y.close()


def test_out_of_range_actions_reject_the_batch():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import pack_atari_plane_records
    T, B, A = 2, 7, 18
    good = rand_planes(T, B, A, seed=21)
    bad = [x.copy() for x in good]
    bad[4][0, 3] = A
    bad[4][1, 5] = -1
    Y = mk(T, B, A, optimizer="adam", seed=4, records="planes")
    twin = mk(T, B, A, optimizer="adam", seed=4, records="planes")
    p0, v0 = Y.get_params(), Y.get_blob()[1]
    with pytest.raises(FiError, match=r"rc=-1: .*2 action\(s\) outside \[0, 18\)"):
        Y.step(pack_atari_plane_records(*bad))
    np.testing.assert_array_equal(Y.get_params(), p0)
    assert Y.get_blob()[1] == v0 == 0
    # the stored actions are clamped, the rest of the batch is ingested as sent
    act = Y.tensor("actions", np.int32, (T, B))
    assert act[0, 3] == A - 1 and act[1, 5] == 0
    np.testing.assert_array_equal(Y.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4)), stacked_of(bad)[0])
    st = Y.step(pack_atari_plane_records(*good))
    ref = twin.step(pack_atari_plane_records(*good))
    assert st["version"] == ref["version"] == 1 and st["total_loss"] == ref["total_loss"]
    np.testing.assert_array_equal(Y.get_params(), twin.get_params())
    assert np.abs(Y.get_params() - p0).max() > 0
    Y.close()
    twin.close()
