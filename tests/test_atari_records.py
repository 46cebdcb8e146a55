"""The Atari host record (28 ELEMENTs = 28,672 B per step: 84x84x4 u8 frame, then the MLP
record's header shape) on the CPU side: the Python packer / unpacker, the constants and exports
of the C ABI, the command line's entry-size arithmetic, and the MLP actor's byte stream, which
the Atari writer must leave as it was.
"""
import hashlib
import os
import re

import numpy as np
import pytest

from test_dropin import _make, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC, FRAME = 28672, 84 * 84 * 4


def _batch(T, B, A, seed=0):
    rs = np.random.RandomState(seed)
    frames = rs.randint(0, 256, (T + 1, B, 84, 84, 4)).astype(np.uint8)
    mu = rs.randn(T, B, A).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.randn(T, B).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.1)).astype(np.float32)
    return frames, mu, act, rew, disc


@pytest.mark.parametrize("T,B,A", [(1, 1, 4), (2, 7, 18)])
@pytest.mark.parametrize("spare", [0, 5])
def test_pack_unpack_round_trip(T, B, A, spare):
    from freeimpala_amd.learner import pack_atari_records, unpack_atari_records
    src = _batch(T, B, A, seed=T * 10 + B)
    S = 28 * (T + 1) + spare
    entries = pack_atari_records(*src, entry_size=S if spare else None)
    assert len(entries) == B and all(len(e) == S * 1024 for e in entries)
    for how in (entries, b"".join(entries), np.frombuffer(b"".join(entries), np.uint8)):
        got = unpack_atari_records(how, T, B, A)
        for g, s in zip(got, src):
            assert g.dtype == s.dtype and g.shape == s.shape
            np.testing.assert_array_equal(g, s)
    # everything outside the fields is zero: the header of record T, the reserved tail, the spare
    e = np.frombuffer(entries[-1], np.uint8).copy()
    rec = e[:(T + 1) * REC].reshape(T + 1, REC)
    assert not rec[T, FRAME:].any() and not rec[:, FRAME + 268:].any() and not e[(T + 1) * REC:].any()
    assert not rec[:T, FRAME + 4 * A:FRAME + 256].any()
    with pytest.raises(ValueError):
        pack_atari_records(*src, entry_size=28 * (T + 1) - 1)


def test_field_offsets_by_poking_known_bytes():
    """The table of DESIGN.md section 3: frame [0, 28224), mu at 28224, action 28480, reward
    28484, discount 28488, flags 28492, record stride 28672; entry b of the batch is column b."""
    from freeimpala_amd.learner import pack_atari_records, unpack_atari_records
    T, B, A = 2, 3, 6
    frames, mu, act, rew, disc = (np.zeros_like(x) for x in _batch(T, B, A))
    frames[1, 2, 0, 0, 0] = 0xA1           # first byte of the frame of record 1
    frames[1, 2, 83, 83, 3] = 0xA2         # its last byte
    frames[2, 2, 0, 0, 1] = 0xA3           # the bootstrap frame (record T)
    frames[0, 2, 0, 1, 0] = 0xA4           # NHWC: pixel (0, 1) channel 0 is byte 4
    mu[1, 2, 0], mu[1, 2, A - 1] = 1.5, -2.5
    act[1, 2], rew[1, 2], disc[1, 2] = 5, 0.25, 0.75
    entries = pack_atari_records(frames, mu, act, rew, disc)
    assert not np.frombuffer(entries[0], np.uint8).any() and not np.frombuffer(entries[1], np.uint8).any()
    e = np.frombuffer(entries[2], np.uint8)
    assert e.size == 28 * 1024 * (T + 1)
    r = e[REC:2 * REC]
    assert r[0] == 0xA1 and r[FRAME - 1] == 0xA2 and e[2 * REC + 1] == 0xA3 and e[4] == 0xA4
    assert r[28224:28228].view(np.float32)[0] == 1.5
    assert r[28224 + 4 * (A - 1):28224 + 4 * A].view(np.float32)[0] == -2.5
    assert r[28480:28484].view(np.int32)[0] == 5
    assert r[28484:28488].view(np.float32)[0] == 0.25
    assert r[28488:28492].view(np.float32)[0] == 0.75
    assert np.count_nonzero(e) == 4 + np.count_nonzero(r[28224:28496])
    # the unpacker reads the same offsets: poke the raw bytes, read the fields
    raw = [bytearray(x) for x in entries]
    raw[0][0 * REC + 28480:0 * REC + 28484] = np.int32(3).tobytes()
    raw[0][1 * REC + 28488:1 * REC + 28492] = np.float32(0.5).tobytes()
    raw[0][2 * REC + 28480:2 * REC + 28484] = np.int32(9).tobytes()   # header of record T: ignored
    raw[0][0 * REC + 28492:0 * REC + 28496] = np.uint32(77).tobytes()  # flags: not a learner input
    f2, m2, a2, r2, d2 = unpack_atari_records(raw, T, B, A)
    assert a2[0, 0] == 3 and d2[1, 0] == 0.5 and a2.sum() == 3 + 5 and not m2[:, 0].any()


def test_header_constants_signatures_and_exports():
    from freeimpala_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "fi_learner.h")).read()
    assert re.search(r"#define\s+FI_ATARI_RECORD_ELEMENTS\s+28\b", hdr)
    assert re.search(r"#define\s+FI_ATARI_RECORD_BYTES\s+28672\b", hdr)
    assert _abi.ATARI_RECORD_ELEMENTS == 28 and _abi.ATARI_RECORD_BYTES == REC == 28 * _abi.RECORD_BYTES
    assert (_abi.ATARI_REC_MU, _abi.ATARI_REC_ACT, _abi.ATARI_REC_REW, _abi.ATARI_REC_DISC,
            _abi.ATARI_REC_FLAGS) == (28224, 28480, 28484, 28488, 28492)
    # the header keeps the MLP record's relative offsets
    for a, m in ((_abi.ATARI_REC_ACT, _abi.REC_ACT), (_abi.ATARI_REC_REW, _abi.REC_REW),
                 (_abi.ATARI_REC_DISC, _abi.REC_DISC), (_abi.ATARI_REC_FLAGS, _abi.REC_FLAGS)):
        assert a - _abi.ATARI_REC_MU == m - _abi.REC_MU
    lib = _abi.lib()
    for name, nargs in (("fi_learner_record_bytes", 1), ("fi_ingest_atari_records", 11)):
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][0]) == nargs
        assert hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert lib.fi_learner_record_bytes(None) == 0


ATARI = ["--learner-arch", "atari", "--players", "1", "--seq-length", "2", "--batch-size", "4",
         "--buffer-capacity", "8", "--agents", "2", "--iterations", "8", "--agent-time", "0"]


def test_cli_entry_size_counts_28_elements_per_atari_record():
    r = run(ATARI + ["--entry-size", "83", "--game-steps", "3"])
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--entry-size must be >= 84" in r.stderr
    # 3 game steps of 28 elements do not fit 2 records' worth either
    r = run(ATARI[:4] + ["--seq-length", "1"] + ATARI[6:] + ["--entry-size", "83", "--game-steps", "3"])
    assert r.returncode == 1 and "84 elements" in r.stderr, r.stdout + r.stderr
    # the MLP arithmetic is as before: one element per record
    r = run(["--learner-arch", "mlp"] + ATARI[2:] + ["--entry-size", "2", "--game-steps", "2"])
    assert r.returncode == 1 and "seq_length + 1 = 3" in r.stderr, r.stdout + r.stderr


def test_cli_atari_writer_on_the_sim_learner(tmp_path):
    """The synthetic actors' Atari records without a GPU (--learner sim consumes the same
    SharedBuffer entries): step s of the game at (s / P) * 28 * 1024 of player s % P's entry."""
    import json
    from freeimpala_amd.learner import unpack_atari_records
    dump = tmp_path / "dump"
    r = run(["--learner", "sim", "--learner-time", "0"] + ATARI + [
        "--entry-size", "85", "--game-steps", "3", "--seed", "7", "--checkpoint-freq", "0", "--log-level", "warn",
        "--checkpoint-location", str(tmp_path / "ck"), "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["learner_iterations"] == [4]
    seen = set()
    for k in range(4):
        b = np.fromfile(dump / f"batch_0_{k}.bin", np.uint8)
        assert b.size == 4 * 85 * 1024
        frames, mu, act, rew, disc = unpack_atari_records(b, 2, 4, 18)
        assert ((act >= 0) & (act < 18)).all() and np.isin(rew, (-1, 0, 1)).all()
        assert np.isin(disc, (np.float32(0), np.float32(0.99))).all()
        assert 0.5 < mu.std() < 1.5 and 100 < frames.mean() < 155 and frames.min() < 8 and frames.max() > 247
        e = b.reshape(4, 85 * 1024)
        assert not e[:, 3 * REC:].any()                                # the spare element
        assert not e[:, :3 * REC].reshape(4, 3, REC)[:, :, 28496:].any()  # reserved
        seen.update(hashlib.sha256(x.tobytes()).hexdigest() for x in e)
    assert len(seen) == 16  # 2 actors x 8 games, every entry different


def test_cli_atari_passes_parsing_then_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("expects no GPU")
    r = run(ATARI + ["--entry-size", "84", "--game-steps", "3"])
    assert r.returncode == 2, r.stdout + r.stderr
    assert "fi_learner_create" in r.stderr and "device" in r.stderr


def test_mlp_writer_byte_stream_unchanged(tmp_path):
    """The synthetic MLP actor draws exactly what it drew before the Atari record existed: one
    actor (a deterministic write order), two players (the s % P interleave), --learner sim (no
    GPU); the first batch each player's learner reads hashes to the value recorded from the
    writer as it was before (tests/golden/mlp_sim_writer_batch.sha256)."""
    dump = tmp_path / "dump"
    r = run(["--learner", "sim", "--players", "2", "--iterations", "4", "--buffer-capacity", "8",
             "--batch-size", "4", "--agents", "1", "--learner-time", "0", "--agent-time", "0", "--seed", "7",
             "--seq-length", "5", "--entry-size", "12", "--game-steps", "12", "--checkpoint-freq", "0",
             "--log-level", "warn", "--checkpoint-location", str(tmp_path / "ck"), "--dump-dir", str(dump)])
    assert r.returncode == 0, r.stdout + r.stderr
    want = dict(reversed(ln.split()) for ln in
                open(os.path.join(ROOT, "tests", "golden", "mlp_sim_writer_batch.sha256")).read().splitlines())
    assert sorted(want) == ["batch_0_0.bin", "batch_1_0.bin"]
    for name, sha in want.items():
        blob = (dump / name).read_bytes()
        assert len(blob) == 4 * 12 * 1024
        assert hashlib.sha256(blob).hexdigest() == sha, name
