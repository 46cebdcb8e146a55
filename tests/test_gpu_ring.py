"""The device entry ring (include/fi_ring.h): the two kernels alone against the host rule, a learner
that steps from a ring against one that is fed the same entries from the host -- FIFO, mixed with
replayed entries across a wrap, behind an overwriting push, and with recording actors that run two
unrolls ahead of the learner -- the refusals, the older paths behind a ring step, and the C++
check program.

Every comparison is exact: the batch rule is integer arithmetic and the ingest a byte shuffle."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC, HIST = 7168, 21504
FLAGS, MLP_FLAGS = 7140, 780
G = 64  # guard bytes on both sides of every output
T, B = 2, 5
D_, H_ = 7, 32
ATARI_E = (T + 1) * REC + HIST  # 43008
MLP_E = (T + 1) * 1024


class Guarded:
    """Device outputs between 0xA5 guards."""

    def __init__(self, shapes):
        from freeimpala_amd import hip
        self.shapes, self.bufs = shapes, []
        for n, dt in shapes:
            nb = n * np.dtype(dt).itemsize
            b = hip.DeviceBuffer(nb + 2 * G)
            b.upload(np.full(nb + 2 * G, 0xA5, np.uint8))
            self.bufs.append((b, nb))
        self.ptr = [b.ptr + G for b, _ in self.bufs]

    def read(self, names):
        out = {}
        for (b, nb), (n, dt), nm in zip(self.bufs, self.shapes, names):
            got = b.download(np.uint8, (nb + 2 * G,))
            assert (got[:G] == 0xA5).all() and (got[G + nb:] == 0xA5).all(), nm + ": guard overwritten"
            out[nm] = got[G:G + nb].view(dt).copy()
        return out

    def free(self):
        for b, _ in self.bufs:
            b.free()


def spaced(rows, stride):
    """(n, E) entries as one device buffer, `stride` apart, 0xFF between and behind them."""
    from freeimpala_amd import hip
    n, E = rows.shape
    host = np.full(n * stride, 0xFF, np.uint8)
    for i in range(n):
        host[i * stride:i * stride + E] = rows[i]
    return hip.DeviceBuffer.from_array(host)


# ------------------------------------------------------------------ 1. the copy kernel alone
@pytest.mark.parametrize("E", [16, 48, ATARI_E])
def test_copy_kernel_fills_its_slots_and_nothing_else(E):
    from freeimpala_amd import hip, ring
    C = 7
    rs = np.random.RandomState(E % 1000)
    for first, n in ((0, 4), (5, 4), (12, 4), (3, 1), (0, 7), (12, 7)):  # from 5 and 12 the run wraps inside the launch
        rows = rs.randint(0, 256, (n, E)).astype(np.uint8)
        src = spaced(rows, E + 48)
        dst = Guarded([(C * E, np.uint8)])
        ring.copy_entries(dst.ptr[0], E, C, first, src.ptr, E + 48, n)
        hip.synchronize()
        got = dst.read(("ring",))["ring"].reshape(C, E)
        want = np.full((C, E), 0xA5, np.uint8)
        for i in range(n):
            want[(first + i) % C] = rows[i]
        np.testing.assert_array_equal(got, want, err_msg=f"first_entry {first}, n {n}")
        src.free()
        dst.free()


# ------------------------------------------------------------------ 2. the columns kernel alone
def columns_case(orc, Bc, C, n_fresh, head, tail, seed, draw, E=ATARI_E):
    from freeimpala_amd import hip, ring
    lo = max(0, head - C)
    want = ring.ring_batch_entries(orc.philox4, seed, draw, Bc, n_fresh, head, tail, C)
    base = 0x7F0000001000  # never read: the kernel only computes addresses
    out = Guarded([(Bc, np.uint64), (Bc, np.uint64), (2, np.uint64)])
    ring.fill_columns(out.ptr[0], out.ptr[1], out.ptr[2], base, E, C, Bc, n_fresh, tail, lo, tail - lo, seed, draw)
    hip.synchronize()
    got = out.read(("cols", "entries", "versions"))
    out.free()
    np.testing.assert_array_equal(got["entries"], np.array(want, np.uint64))
    np.testing.assert_array_equal(got["cols"], np.array([base + (e % C) * E for e in want], np.uint64))
    np.testing.assert_array_equal(got["versions"].view(np.uint32), np.array([0xFFFFFFFF, 0, 0, 0], np.uint32))
    return want


def test_columns_kernel_equals_the_host_rule(orc):
    from freeimpala_amd.ring import ring_batch_entries
    C, head, tail = 8, 14, 9  # lo = 6: the replayable entries 6, 7, 8 lie in the slots 6, 7, 0
    assert [e % C for e in range(head - C, tail)] == [6, 7, 0]
    # a seed whose batch at n_fresh = 3 replays one entry twice, picked with the oracle's philox4
    seed = next(s for s in range(1, 200)
                if len(set(ring_batch_entries(orc.philox4, s, 2, B, 3, head, tail, C)[3:])) == 1)
    for n_fresh in (0, 3, 5):
        e = columns_case(orc, B, C, n_fresh, head, tail, seed, 2)
        assert e[:n_fresh] == list(range(tail, tail + n_fresh)) and all(6 <= x < 9 for x in e[n_fresh:])
        if n_fresh < B:
            assert len(set(e[n_fresh:])) < B - n_fresh, "a duplicated entry"
    # more than one workgroup, the last one's lanes 44 .. 255 idle
    e = columns_case(orc, 300, 512, 100, 700, 400, seed, 3)
    assert len(e) == 300 and len(set(e[100:])) > 100 and all(188 <= x < 400 for x in e[100:])
    # a window far above 2^32, capacity 2^31 - 1
    columns_case(orc, B, 2 ** 31 - 1, 2, 2 ** 40 + 2 ** 31 + 5, 2 ** 40 + 2 ** 31, 11, 2 ** 63, E=16)


# ------------------------------------------------------------------ entries
def flag_words(first, n):
    """Distinct per entry and record, some above 2^31; record T: all ones."""
    w = np.array([[(0xF0000000 if (first + b) % 2 == 0 else 7) + 1000 * (first + b) + t for t in range(T + 1)]
                  for b in range(n)], np.uint32)
    w[:, T] = 0xFFFFFFFF
    return w


def make_entries(arch, n, A, seed, first=0, bad_action=False):
    """n packed entries (n, E) uint8 whose flags words are flag_words(first, n). Atari: start flags
    at t = 0, mid-unroll and twice in a row, as test_gpu_gather.py chooses them."""
    from freeimpala_amd.learner import pack_atari_plane_records, pack_records
    rs = np.random.RandomState(seed)
    mu = rs.standard_normal((T, n, A)).astype(np.float32)
    act = rs.randint(0, A, (T, n)).astype(np.int32)
    if bad_action:
        act[1, 3] = A + 3  # out of range: counted, stored clamped, the batch rejected
    rew = rs.standard_normal((T, n)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, n) > 0.3)).astype(np.float32)
    if arch == "atari":
        planes = rs.randint(0, 256, (T + 1, n, 84, 84)).astype(np.uint8)
        history = rs.randint(0, 256, (3, n, 84, 84)).astype(np.uint8)
        start = np.zeros((T + 1, n), bool)
        for b in range(n):
            k = (first + b) % 5
            start[:, b] = [(1, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 0), (1, 1, 0)][k]
        rows = pack_atari_plane_records(planes, history, start, mu, act, rew, disc)
        rec, off = REC, FLAGS
    else:
        obs = rs.standard_normal((T + 1, n, D_)).astype(np.float32)
        rows = pack_records(obs, mu, act, rew, disc)
        rec, off = 1024, MLP_FLAGS
    raw = np.stack([np.frombuffer(e, np.uint8) for e in rows]).copy()
    words = flag_words(first, n)
    for t in range(T + 1):
        raw[:, t * rec + off:t * rec + off + 4] = words[:, t:t + 1].copy().view(np.uint8)
    return raw, words


def versions_of(words, chosen):
    w = words[list(chosen)][:, :T].astype(np.uint64)
    return dict(min=int(w.min()), max=int(w.max()), mean=int(w.sum()) / w.size, count=int(w.size))


def make_learner(arch, A, optimizer="adam", lr=1e-3, batch=B, **over):
    from freeimpala_amd.learner import DeviceLearner
    kw = dict(seq_len=T, batch=batch, num_actions=A, optimizer=optimizer, lr=lr)
    if arch == "atari":
        kw["records"] = "planes"
    else:
        kw.update(obs_dim=D_, hidden=H_)
    kw.update(over)
    return DeviceLearner(arch, **kw)


def learner_pair(arch, A, **kw):
    """Two learners of the same seed and parameters: one for the ring, one fed from the host."""
    R, Hh = make_learner(arch, A, **kw), make_learner(arch, A, **kw)
    Hh.set_params(R.get_params())
    return R, Hh


INGESTED = {"atari": (("frames", np.uint8),), "mlp": (("obs", np.float32),)}
COMMON = (("mu", np.float32), ("actions", np.int32), ("rewards", np.float32), ("discounts", np.float32),
          ("logits", np.float32), ("vs", np.float32))


def snapshot(L, stats=None):
    d = {nm: L.tensor(nm, dt) for nm, dt in INGESTED[L.arch] + COMMON}
    d["params"] = L.get_params()
    if stats is not None:
        d["stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    return d


def same(x, y, what):
    assert x.keys() == y.keys()
    for nm in x:
        if nm == "stats":
            assert x[nm] == y[nm], (what, x[nm], y[nm])
        else:
            np.testing.assert_array_equal(x[nm], y[nm], err_msg=f"{what}: {nm}")


# ------------------------------------------------------------------ 3. FIFO = the host-fed learner
@pytest.mark.parametrize("arch,A", [("atari", 18), ("atari", 2), ("mlp", 3)])
def test_fifo_step_equals_the_host_fed_learner(arch, A):
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.ring import EntryRing
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    assert E == (ATARI_E if arch == "atari" else MLP_E)
    p0 = R.get_params()
    for bad in (True, False):  # the issue's batch, with its out-of-range action; then the same batch without
        raw, words = make_entries(arch, B, A, seed=A, bad_action=bad)
        ring = EntryRing(E, 8, seed=3)
        a, b = spaced(raw[:2], E + 48), spaced(raw[2:], E + 1024)  # two pushes, 2 + 3, two strides
        ring.push(a.ptr, E + 48, 2)
        ring.push(b.ptr, E + 1024, 3)
        assert ring.info() == dict(capacity=8, entry_bytes=E, head=5, tail=0, draw=0, seed=3)
        np.testing.assert_array_equal(ring.read_slots(0, 5), raw)
        assert not ring.read_slots(5, 3).any(), "the slots behind are still zero"
        rows = [r for r in raw]
        if bad:
            # both learners reject the batch (one action outside [0, A)); everything ingested is equal,
            # the parameters stay, and the entries stay unread
            with pytest.raises(FiError, match=r"rc=-1: .*1 action\(s\) outside"):
                R.step_ring(ring)
            with pytest.raises(FiError, match=r"rc=-1: .*1 action\(s\) outside"):
                Hh.step(rows)
            same(snapshot(R), snapshot(Hh), "rejected batch")
            np.testing.assert_array_equal(R.get_params(), p0)
            assert ring.info()["tail"] == 0 and ring.info()["draw"] == 0
        else:
            got, want = snapshot(R, R.step_ring(ring)), snapshot(Hh, Hh.step(rows))
            same(got, want, "FIFO step")
            assert got["stats"]["version"] == 1 and (got["params"] != p0).any()
            assert ring.info() == dict(capacity=8, entry_bytes=E, head=5, tail=5, draw=1, seed=3)
            assert ring.last_entries(B) == [0, 1, 2, 3, 4]
        assert R.batch_versions == versions_of(words, range(B))
        assert R.staging_bytes == 0 and Hh.staging_bytes > 0
        for h in (a, b):
            h.free()
        ring.close()
    R.close()
    Hh.close()


# ------------------------------------------------------------------ 4. mixed batches across a wrap
@pytest.mark.parametrize("arch,A", [("atari", 18), ("mlp", 3)])
def test_mixed_batches_across_a_wrap(arch, A, orc):
    from freeimpala_amd.ring import EntryRing, ring_batch_entries
    C = 8
    raw, words = make_entries(arch, 13, A, seed=40 + A)
    plan = ((0, 5, 5), (5, 3, 3), (8, 5, 2))  # (first entry pushed, how many, n_fresh of the step behind)

    def batches(seed):
        head = tail = 0
        out = []
        for draw, (_, n, n_fresh) in enumerate(plan):
            head += n
            out.append(ring_batch_entries(orc.philox4, seed, draw, B, n_fresh, head, tail, C))
            tail += n_fresh
        return out

    # a seed whose second or third batch names an entry twice
    seed = next(s for s in range(1, 200) if any(len(set(b)) < B for b in batches(s)[1:]))
    want = batches(seed)
    assert want[0] == [0, 1, 2, 3, 4]
    assert want[1][:3] == [5, 6, 7] and all(0 <= e < 5 for e in want[1][3:])
    assert want[2][:2] == [8, 9] and all(5 <= e < 8 for e in want[2][2:])

    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    ring = EntryRing(E, C, seed=seed)
    for k, (first, n, n_fresh) in enumerate(plan):
        src = spaced(raw[first:first + n], E + 48)
        ring.push(src.ptr, E + 48, n)
        before = ring.info()
        assert ring_batch_entries(orc.philox4, seed, before["draw"], B, n_fresh, before["head"], before["tail"], C) == want[k]
        got = snapshot(R, R.step_ring(ring, n_fresh=n_fresh))
        assert ring.last_entries(B) == want[k], k
        same(got, snapshot(Hh, Hh.step([raw[e] for e in want[k]])), f"step {k}")
        assert R.batch_versions == versions_of(words, want[k]), k  # a duplicated entry counts twice
        after = ring.info()
        assert (after["head"], after["tail"], after["draw"]) == (before["head"], before["tail"] + n_fresh, k + 1)
        src.free()
    # entries 8 .. 12 overwrote 0 .. 4; 5, 6, 7 are where they were
    np.testing.assert_array_equal(ring.read_slots(), raw[[8, 9, 10, 11, 12, 5, 6, 7]])
    ring.close()
    R.close()
    Hh.close()


# ------------------------------------------------------------------ 5. ordering against an overwrite
def test_an_overwriting_push_goes_behind_the_ingest():
    from freeimpala_amd.ring import EntryRing
    arch, A = "atari", 18
    old, _ = make_entries(arch, B, A, seed=50)
    new, _ = make_entries(arch, B, A, seed=51, first=5)
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    ring = EntryRing(E, B)  # capacity = batch: the next push takes exactly the slots the step reads
    a, b = spaced(old, E), spaced(new, E + 48)
    ring.push(a.ptr, E, B)
    assert R.step_ring(ring, wait=False) is None
    ring.push(b.ptr, E + 48, B)  # at once: refused as full unless the step counted as taken
    st = R.wait()
    same(snapshot(R, st), snapshot(Hh, Hh.step([r for r in old])), "the old entries")
    np.testing.assert_array_equal(ring.read_slots(), new)
    assert ring.info()["head"] == 10 and ring.info()["tail"] == 5
    for h in (a, b, ring, R, Hh):
        (h.free if hasattr(h, "free") else h.close)()


# ------------------------------------------------------------------ 6. with actors
def act_call(a, arch, rs):
    if arch == "atari":
        out = a.act_planes(rs.randint(0, 256, (a.N, 84, 84)).astype(np.uint8), rs.rand(a.N) < 0.3)
    else:
        out = a.act_obs(rs.standard_normal((a.N, D_)).astype(np.float32))
    a.outcome(rs.randint(-1, 2, a.N).astype(np.float32), (0.99 * (rs.rand(a.N) > 0.2)).astype(np.float32))
    return out


def make_actor(arch, n, A, p0, version, seed):
    from freeimpala_amd.actor import Actor
    a = Actor(arch, n, num_actions=A, seed=seed) if arch == "atari" else \
        Actor(arch, n, num_actions=A, obs_dim=D_, hidden=H_, seed=seed)
    a.set_params(p0, version=version)
    a.begin_rollout(T)
    return a


def test_actors_run_two_unrolls_ahead_of_the_learner(orc):
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.ring import EntryRing, ring_batch_entries
    arch, A = "atari", 18
    R, Hh = learner_pair(arch, A, optimizer="sgd", lr=0.0)  # the learners hold the actors' parameters throughout
    p0 = R.get_params()
    rs = np.random.RandomState(60)
    # without the ring: the call that completes unroll 1 is refused while unroll 0 waits for a learner
    lone = make_actor(arch, 2, A, p0, 0, seed=70)
    for _ in range(2 * T):
        act_call(lone, arch, rs)
    assert lone.rollout_ready()
    with pytest.raises(FiError, match=r"rc=-4: .*released"):
        act_call(lone, arch, rs)
    lone.end_rollout()
    lone.close()
    # with it: two actors, two unrolls each, before any learner step
    actors = [make_actor(arch, 2, A, p0, 0, seed=71), make_actor(arch, 3, A, p0, 5, seed=72)]
    ring = EntryRing(R.entry_bytes, 10, seed=9)
    pushed = []
    for unroll in range(2):
        for a in actors:
            for _ in range(T + 1 if unroll == 0 else T):
                act_call(a, arch, rs)
            assert a.rollout_ready()
            pushed.append(a.read_rollout())
            ring.push_rollout(a)
            assert not a.rollout_ready()
    assert ring.info()["head"] == 10 and ring.info()["tail"] == 0
    np.testing.assert_array_equal(ring.read_slots(), np.concatenate(pushed))
    ver = np.array([0, 0, 5, 5, 5, 0, 0, 5, 5, 5])
    for k, n_fresh in enumerate((5, 3)):
        i = ring.info()
        want = ring_batch_entries(orc.philox4, 9, i["draw"], B, n_fresh, i["head"], i["tail"], 10)
        got = snapshot(R, R.step_ring(ring, n_fresh=n_fresh))
        assert ring.last_entries(B) == want
        same(got, snapshot(Hh, Hh.step([r for r in ring.read_entries(want)])), f"step {k}")
        v = ver[want]
        assert R.batch_versions == dict(min=int(v.min()), max=int(v.max()), mean=int(v.sum()) * T / (T * B), count=T * B)
        # learner and actors hold the same parameters: pi = mu bit for bit
        np.testing.assert_array_equal(got["logits"].reshape(T + 1, B, A)[:T], got["mu"].reshape(T, B, A))
    assert ring.info()["tail"] == 8
    for a in actors:
        a.end_rollout()
        a.close()
    for h in (ring, R, Hh):
        h.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_ring_as_it_was():
    from freeimpala_amd import hip
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, B, A, seed=80)
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    src = spaced(raw, E + 48)
    with pytest.raises(FiError, match=r"rc=-1: .*entry_bytes 24"):
        EntryRing(24, 8)
    with pytest.raises(FiError, match=r"rc=-1: .*entry_bytes 8"):
        EntryRing(8, 8)
    with pytest.raises(FiError, match=r"rc=-1: .*capacity 0"):
        EntryRing(E, 0)
    with pytest.raises(FiError, match=rf"rc=-1: .*capacity {2 ** 31}"):
        EntryRing(E, 2 ** 31)
    ring = EntryRing(E, 8, seed=1)

    def refused(match, call, *args, **kw):
        before = ring.info()
        with pytest.raises(FiError, match=match):
            call(*args, **kw)
        assert ring.info() == before

    refused(r"rc=-4: .*no ring step yet", ring.last_entries, B)
    refused(rf"rc=-4: .*0 entries unread, n_fresh = {B}", R.step_ring, ring)
    refused(r"rc=-1: .*16-byte aligned", ring.push, src.ptr + 8, E + 48, 1)
    refused(r"rc=-1: .*16-byte aligned", ring.push, src.ptr, E + 8, B)
    refused(rf"rc=-1: .*entry_stride {E - 16} < entry_bytes {E}", ring.push, src.ptr, E - 16, B)
    refused(r"rc=-1: .*n = 0 < 1", ring.push, src.ptr, E + 48, 0)
    refused(r"rc=-1: .*the allocation ends", ring.push, src.ptr, E + 48, B + 1)
    host_mem = np.zeros(E + 16, np.uint8)
    refused(r"rc=-1: .*not device memory", ring.push, host_mem.ctypes.data + (-host_mem.ctypes.data) % 16, E, 1)
    ring.push(src.ptr, E + 48, B)
    refused(r"rc=-4: .*full: 5 entries, capacity 8 - 5 unread leaves 3", ring.push, src.ptr, E + 48, B)
    refused(rf"rc=-4: .*nothing to replay: 2 columns of the batch {B}", R.step_ring, ring, n_fresh=3)
    refused(rf"rc=-1: .*n_fresh {B + 1} outside 0 .. batch {B}", R.step_ring, ring, n_fresh=B + 1)
    refused(rf"rc=-1: .*n_fresh -1 outside 0 .. batch {B}", R.step_ring, ring, n_fresh=-1)
    refused(rf"rc=-1: .*n_fresh {B + 1} outside", R.step_ring, ring, n_fresh=B + 1, wait=False)
    refused(r"rc=-1: .*slots 6 .. 9 outside the capacity 8", ring.read_slots, 6, 3)
    # entry sizes: a learner whose entries are longer than the ring's, an actor whose are not the ring's
    longer = make_learner(arch, A, seq_len=T + 1)
    refused(rf"rc=-1: .*entry_bytes {E} < {E + 1024} = fi_learner_entry_bytes", longer.step_ring, ring)
    longer.close()
    actor = make_actor(arch, 2, A, R.get_params(), 0, seed=81)
    rs = np.random.RandomState(82)
    refused(r"rc=-4: .*no completed unroll", ring.push_rollout, actor)
    for _ in range(T + 1):
        act_call(actor, arch, rs)
    wide = EntryRing(E + 16, 8)
    with pytest.raises(FiError, match=rf"rc=-1: .*actor's entry bytes {E} != the ring's entry_bytes {E + 16}"):
        wide.push_rollout(actor)
    assert wide.info()["head"] == 0 and actor.rollout_ready()
    wide.close()
    ring.push_rollout(actor)  # 2 entries: 7 unread of 8
    assert not actor.rollout_ready()
    for _ in range(T):
        act_call(actor, arch, rs)
    refused(r"rc=-4: .*full: 2 entries, capacity 8 - 7 unread leaves 1", ring.push_rollout, actor)
    assert actor.rollout_ready(), "the unroll still waits"
    stacked = make_learner("atari", 18, records="stacked")
    refused(r"rc=-1: .*planes format", stacked.step_ring, ring)
    stacked.close()
    with pytest.raises(FiError, match=r"rc=-4: .*no step from segments"):
        R.batch_versions
    assert R.staging_bytes == 0
    # every refusal left ring and learner as they were: the FIFO step is the host-fed learner's
    same(snapshot(R, R.step_ring(ring)), snapshot(Hh, Hh.step([r for r in raw])), "after the refusals")
    refused(rf"rc=-4: .*2 entries unread, n_fresh = 3", R.step_ring, ring, n_fresh=3)
    ring.push_rollout(actor)  # room again
    assert ring.info() == dict(capacity=8, entry_bytes=E, head=9, tail=5, draw=1, seed=1)
    actor.end_rollout()
    for h in (actor, ring, R, Hh):
        h.close()
    src.free()
    hip.synchronize()


# ------------------------------------------------------------------ 8. the older paths behind a ring step
def test_older_paths_are_unchanged_behind_a_ring_step():
    """One handle takes a ring step, then step_rollouts, then a host step; before each, a fresh
    handle is given its state and takes only that path on the same entries."""
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    X = make_learner(arch, A)
    E = X.entry_bytes
    raw, _ = make_entries(arch, B, A, seed=90)
    src = spaced(raw, E)
    rs_x, rs_y = np.random.RandomState(91), np.random.RandomState(91)
    ax, ay = (make_actor(arch, B, A, X.get_params(), 2, seed=92) for _ in range(2))  # the same unrolls
    for _ in range(T + 1):
        act_call(ax, arch, rs_x)
        act_call(ay, arch, rs_y)

    def fresh():
        Y = make_learner(arch, A)
        Y.load_state(X.save_state())
        return Y

    def ring_step(L):
        ring = EntryRing(E, 8)
        ring.push(src.ptr, E, B)
        st = L.step_ring(ring)
        ring.close()
        return st

    paths = (("ring", ring_step, ring_step), ("rollouts", lambda L: L.step_rollouts([ax]), lambda L: L.step_rollouts([ay])),
             ("host", lambda L: L.step([r for r in raw]), lambda L: L.step([r for r in raw])))
    for k, (nm, on_x, on_y) in enumerate(paths):
        Y = fresh()
        assert X.staging_bytes == 0 and Y.staging_bytes == 0
        got, want = snapshot(X, on_x(X)), snapshot(Y, on_y(Y))
        same(got, want, nm)
        assert got["stats"]["version"] == k + 1
        assert (X.staging_bytes > 0) == (nm == "host")
        Y.close()
    for a in (ax, ay):
        a.end_rollout()
        a.close()
    X.close()
    src.free()


# ------------------------------------------------------------------ 9. the C++ check program
EXE = os.path.join(ROOT, "build", "host_ring_check")


def test_cpp_check_program_steps_fifo_and_mixed():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_ring_check"], check=True)
    runs = [subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stdout + r.stderr
    lines = [[ln for ln in r.stdout.splitlines() if ln.startswith("ring ")] for r in runs]
    assert len(lines[0]) == 2 and lines[0][0].startswith("ring mlp: fifo 0,1,2,3 mixed 4,5,")
    assert lines[0][1].startswith("ring atari: fifo 0,1,2,3 mixed 4,5,")
    assert lines[0] == lines[1], "a second run prints the same entries"
    for ln in lines[0]:
        assert ln.endswith("version 2") and "nan" not in ln
