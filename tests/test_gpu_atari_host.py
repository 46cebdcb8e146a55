"""The Atari policy fed from host entries (28-element records): the ingest
kernel alone, and fi_learner_step / _step_async / _acquire_staging + _step_staged on an Atari
handle. The ingest is a copy, so everything here is bit-exact: a host-fed step must equal the
resident step on the same tensors, and the resident step is pinned to the oracle by
tests/test_gpu_atari.py (whose checker is reused on an ingested batch).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REC, FRAME = 28672, 84 * 84 * 4
INGEST_MAX_GRID = 2048  # workgroups of ingest_frames_kernel (csrc/misc.hip): one frame each per pass


def mk(T, B, A=18, **kw):
    from freeimpala_amd.learner import DeviceLearner
    kw.setdefault("optimizer", "sgd")
    kw.setdefault("lr", 1e-3)
    kw.setdefault("max_grad_norm", 0.0)
    return DeviceLearner("atari", seq_len=T, batch=B, num_actions=A, **kw)


def rand_batch(T, B, A, seed):
    rs = np.random.RandomState(seed)
    frames = rs.randint(0, 256, (T + 1, B, 84, 84, 4)).astype(np.uint8)
    mu = rs.randn(T, B, A).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.randint(-1, 2, (T, B)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.1)).astype(np.float32)
    return frames, mu, act, rew, disc


def resident(L, T, B, A):
    return (L.tensor("frames", np.uint8, (T + 1, B, 84, 84, 4)), L.tensor("mu", shape=(T, B, A)),
            L.tensor("actions", np.int32, (T, B)), L.tensor("rewards", shape=(T, B)),
            L.tensor("discounts", shape=(T, B)))


# (3, 520): 2,080 frames on the 2,048 workgroups of the frame copy, so its grid-stride loop wraps
@pytest.mark.parametrize("spare", [0, 5])
@pytest.mark.parametrize("T,B", [(1, 1), (2, 7), (3, 32), (3, 520)])
def test_standalone_ingest_is_bit_exact(T, B, spare):
    """fi_ingest_atari_records on uploaded entries: frames, mu, actions, rewards and discounts
    come out as packed, bit for bit. Every byte the kernel must not use is poisoned first -- the
    header of record T, the reserved tail and flags of every record, mu's unused slots, the
    entry padding (0xFF) -- and the outputs sit between guard words that must survive."""
    from freeimpala_amd import hip
    from freeimpala_amd._abi import check, lib
    from freeimpala_amd.learner import pack_atari_records
    A = 6
    if B == 520:
        assert (T + 1) * B > INGEST_MAX_GRID
    src = rand_batch(T, B, A, seed=T * 1000 + B)
    S = 28 * (T + 1) + spare
    raw = np.stack([np.frombuffer(e, np.uint8) for e in pack_atari_records(*src, entry_size=S)]).copy()
    assert raw.shape == (B, S * 1024) and raw.nbytes < 300e6
    rec = raw[:, :(T + 1) * REC].reshape(B, T + 1, REC)
    rec[:, T, FRAME:] = 0xEE                    # record T carries the bootstrap frame only
    rec[:, :, FRAME + 268:] = 0xDD              # flags + reserved
    rec[:, :T, FRAME + 4 * A:FRAME + 256] = 0xCC  # mu slots past A
    raw[:, (T + 1) * REC:] = 0xFF               # entry padding
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
    check(lib().fi_ingest_atari_records(dev.ptr, T, B, A, S * 1024, *ptr, None), "fi_ingest_atari_records")
    hip.synchronize()
    for (b, nb), (n, dt), want, nm in zip(bufs, shapes, src, ("frames", "mu", "actions", "rewards", "discounts")):
        got = b.download(np.uint8, (nb + 2 * G,))
        assert (got[:G] == 0xA5).all() and (got[G + nb:] == 0xA5).all(), nm + ": guard overwritten"
        np.testing.assert_array_equal(got[G:G + nb].view(dt).reshape(want.shape), want, err_msg=nm)
    # what the launcher must refuse before any kernel runs
    from freeimpala_amd._abi import FiError
    with pytest.raises(FiError, match=str((T + 1) * REC)):
        check(lib().fi_ingest_atari_records(dev.ptr, T, B, A, (T + 1) * REC - 16, *ptr, None), "ingest")
    with pytest.raises(FiError, match="multiple of 16"):
        check(lib().fi_ingest_atari_records(dev.ptr, T, B, A, S * 1024 + 8, *ptr, None), "ingest")
    for b, _ in bufs + [(dev, 0)]:
        b.free()


LOSS_KEYS = ("pg_loss", "baseline_loss", "entropy_loss", "total_loss", "grad_norm", "version")
_resident_runs = {}


def resident_run(T, B, opt, steps):
    """Learner X of test 2, once per configuration: synth, read the batch back, step_resident."""
    key = (T, B, opt)
    if key not in _resident_runs:
        A = 18
        X = mk(T, B, A, optimizer=opt, seed=5)
        X.synth(seed=T * 31 + B)
        batch = resident(X, T, B, A)
        stats = [X.step_resident() for _ in range(steps)]
        out = dict(batch=batch, stats=stats, grads=X.tensor("grads"), logits=X.tensor("logits"),
                   values=X.tensor("values"), params=X.get_params())
        X.close()
        for v in out["batch"] + (out["grads"], out["logits"], out["values"], out["params"]):
            v.setflags(write=False)
        _resident_runs[key] = out
    return _resident_runs[key]


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
    return Y.step_staged()


@pytest.mark.parametrize("how", ["step", "async", "staged"])
@pytest.mark.parametrize("opt,steps", [("sgd", 1), ("adam", 2)])
@pytest.mark.parametrize("T,B", [(2, 7), (3, 32)])
def test_host_fed_step_equals_resident_step(T, B, opt, steps, how):
    from freeimpala_amd.learner import pack_atari_records
    A = 18
    ref = resident_run(T, B, opt, steps)
    Y = mk(T, B, A, optimizer=opt, seed=5)
    assert Y.record_bytes == REC and Y.entry_bytes == (T + 1) * REC
    # one spare element per entry on the step / async paths (only the first entry_bytes are read)
    entries = pack_atari_records(*ref["batch"], entry_size=28 * (T + 1) + (how != "staged"))
    for k in range(steps):
        st = feed(Y, entries, how)
        for key in LOSS_KEYS:
            assert st[key] == ref["stats"][k][key], (k, key, st[key], ref["stats"][k][key])
    for got, want in zip(resident(Y, T, B, A), ref["batch"]):
        np.testing.assert_array_equal(got, want)
    for nm in ("grads", "logits", "values"):
        np.testing.assert_array_equal(Y.tensor(nm), ref[nm], err_msg=nm)
    np.testing.assert_array_equal(Y.get_params(), ref["params"])
    Y.close()


def test_ingested_batch_through_the_oracle_chain(orc, monkeypatch):
    """An ingested batch, then forward, V-trace, backward and update against the oracle at the
    bars of tests/test_gpu_atari.py (its checker steps the batch the host step left resident)."""
    from test_gpu_atari import _check_step_against_oracle
    from freeimpala_amd.learner import pack_atari_records
    monkeypatch.setenv("FI_KEEP_DA1", "1")
    monkeypatch.setenv("FI_A1_NHWC", "1")
    T, B, A = 2, 7, 18
    src = rand_batch(T, B, A, seed=11)
    Y = mk(T, B, A)
    Y.step(pack_atari_records(*src))
    for got, want in zip(resident(Y, T, B, A), src):
        np.testing.assert_array_equal(got, want)
    _check_step_against_oracle(orc, Y, T, B, A)
    Y.close()


def test_async_steps_double_buffer():
    """Three different batches through step_async back to back, then one wait: the parameters
    equal three serial steps' bit for bit (a staging slot reused before its ingest had run, or a
    frames tensor rewritten under a running step, would change them)."""
    from freeimpala_amd.learner import pack_atari_records
    T, B, A = 2, 7, 18
    batches = [pack_atari_records(*rand_batch(T, B, A, seed=100 + k)) for k in range(3)]
    S = mk(T, B, A, optimizer="adam", seed=9)
    serial = [S.step(e) for e in batches]
    Y = mk(T, B, A, optimizer="adam", seed=9)
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


def test_out_of_range_actions_reject_the_batch():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import pack_atari_records
    T, B, A = 2, 7, 18
    good = rand_batch(T, B, A, seed=21)
    bad = [x.copy() for x in good]
    bad[2][0, 3] = A
    bad[2][1, 5] = -1
    Y = mk(T, B, A, optimizer="adam", seed=4)
    twin = mk(T, B, A, optimizer="adam", seed=4)
    p0, v0 = Y.get_params(), Y.get_blob()[1]
    with pytest.raises(FiError, match=r"rc=-1: .*2 action\(s\) outside \[0, 18\)"):
        Y.step(pack_atari_records(*bad))
    np.testing.assert_array_equal(Y.get_params(), p0)
    assert Y.get_blob()[1] == v0 == 0
    # the stored actions are clamped, the rest of the batch is ingested as sent
    act = Y.tensor("actions", np.int32, (T, B))
    assert act[0, 3] == A - 1 and act[1, 5] == 0
    st = Y.step(pack_atari_records(*good))
    ref = twin.step(pack_atari_records(*good))
    assert st["version"] == ref["version"] == 1 and st["total_loss"] == ref["total_loss"]
    np.testing.assert_array_equal(Y.get_params(), twin.get_params())
    assert np.abs(Y.get_params() - p0).max() > 0
    Y.close()
    twin.close()


def test_entry_bytes_too_small_is_refused():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.learner import DeviceLearner, pack_records
    T, B = 2, 4
    Y = mk(T, B)
    short = [b"\0" * (REC * (T + 1) - 1024)] * B
    p0 = Y.get_params()
    with pytest.raises(FiError, match=rf"rc=-1: .*{REC * (T + 1)}"):
        Y.step(short)
    with pytest.raises(FiError, match=rf"rc=-1: .*{REC * (T + 1)}"):
        Y.step_async(short)
    np.testing.assert_array_equal(Y.get_params(), p0)
    Y.step([b"\0" * (REC * (T + 1))] * B)  # the minimum is accepted
    Y.close()
    # an MLP handle keeps its 1 KiB records
    M = DeviceLearner("mlp", seq_len=T, batch=B, num_actions=6, obs_dim=8, hidden=16)
    assert M.record_bytes == 1024 and M.entry_bytes == (T + 1) * 1024
    rs = np.random.RandomState(0)
    M.step(pack_records(rs.randn(T + 1, B, 8).astype(np.float32), rs.randn(T, B, 6).astype(np.float32),
                        rs.randint(0, 6, (T, B)).astype(np.int32), rs.randn(T, B).astype(np.float32),
                        np.full((T, B), 0.99, np.float32)))
    M.close()
