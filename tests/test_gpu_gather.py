"""A learner batch gathered from several device buffers (include/fi_gather.h): the gathering ingest
kernels alone against the packer's inverse and against the contiguous ingest, a learner that steps
from two recording actors against one that steps from the host copy of their entries, the closed
loop, one actor as one segment against fi_learner_step_rollout, the refusals, and the older paths
behind a step from segments.

Every comparison is exact. The closed loop alone also checks vs / pg_adv against the oracle's
V-trace on the device's own logits, within 1e-5 of the largest magnitude (the bound of
test_closed_loop_on_the_device in test_gpu_rollout.py)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE, FRAME = 84 * 84, 84 * 84 * 4
REC, HIST = 7168, 21504
FLAGS, MLP_FLAGS = 7140, 780
G = 64  # guard bytes on both sides of every output


def entry_bytes(T):
    return (T + 1) * REC + HIST


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


def scatter(raw, E):
    """B = 5 entries (5, E) into three device buffers with the strides E, E + 48 and E + 1024 -- two,
    two and one entry, 0xFF between and behind them -- and the column table: columns 0..4 alternate
    between the buffers, and within a buffer the later slot comes first, so the table is in no
    address order. Returns (buffers, table of addresses)."""
    from freeimpala_amd import hip
    assert raw.shape == (5, E)
    strides = (E, E + 48, E + 1024)
    where = [(1, 1), (0, 1), (2, 0), (1, 0), (0, 0)]  # column -> (buffer, slot)
    slots = (2, 2, 1)
    host = [np.full(n * s, 0xFF, np.uint8) for n, s in zip(slots, strides)]
    for c, (k, i) in enumerate(where):
        host[k][i * strides[k]:i * strides[k] + E] = raw[c]
    bufs = [hip.DeviceBuffer.from_array(h) for h in host]
    cols = np.array([bufs[k].ptr + i * strides[k] for k, i in where], np.uint64)
    assert (np.diff(cols.astype(np.int64)) < 0).any() and (cols % 16 == 0).all()
    return bufs, cols


def flag_words(T, B):
    """Distinct per record, some above 2^31 so that their sum passes 2^32; record T: all ones."""
    w = np.array([[(0xF0000000 if b % 2 == 0 else 7) + 1000 * b + t for t in range(T + 1)] for b in range(B)],
                 np.uint32)
    w[:, T] = 0xFFFFFFFF
    return w


def check_versions(v, words, T):
    w = words[:, :T].astype(np.uint64)
    assert int(w.sum()) > 2 ** 32
    got = v.view(np.uint32)
    assert (int(got[0]), int(got[1]), int(v.view(np.uint64)[1])) == (int(w.min()), int(w.max()), int(w.sum()))


# ------------------------------------------------------------------ 1. the kernels alone, Atari
@pytest.mark.parametrize("A", [2, 18])
def test_gathering_planes_ingest_is_bit_exact(A):
    from freeimpala_amd import gather, hip
    from freeimpala_amd._abi import check, lib
    from freeimpala_amd.learner import pack_atari_plane_records, stack_planes, unpack_atari_plane_records
    T, B = 2, 5
    E = entry_bytes(T)
    rs = np.random.RandomState(A)
    planes = rs.randint(0, 256, (T + 1, B, 84, 84)).astype(np.uint8)
    history = rs.randint(0, 256, (3, B, 84, 84)).astype(np.uint8)
    start = np.zeros((T + 1, B), bool)
    start[0, 0] = True                 # a start at t = 0
    start[1, 1] = True                 # one mid-unroll, behind a frame from the history block
    start[1, 2] = start[2, 2] = True   # two in a row; column 3 never starts
    start[0, 4] = start[1, 4] = True
    mu = rs.standard_normal((T, B, A)).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    act[1, 3] = A + 3                  # out of range: counted, stored clamped
    rew = rs.standard_normal((T, B)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.3)).astype(np.float32)
    raw = np.stack([np.frombuffer(e, np.uint8)
                    for e in pack_atari_plane_records(planes, history, start, mu, act, rew, disc)]).copy()
    words = flag_words(T, B)
    for t in range(T + 1):
        raw[:, t * REC + FLAGS:t * REC + FLAGS + 4] = words[:, t:t + 1].copy().view(np.uint8)
    u = unpack_atari_plane_records(raw, T, B, A)
    want = dict(frames=stack_planes(*u[:3]).ravel(), mu=u[3].ravel(), act=np.clip(u[4], 0, A - 1).ravel(),
                rew=u[5].ravel(), disc=u[6].ravel())
    names = ("frames", "mu", "act", "rew", "disc", "bad", "versions")
    shapes = [((T + 1) * B * FRAME, np.uint8), (T * B * A, np.float32), (T * B, np.int32), (T * B, np.float32),
              (T * B, np.float32), (1, np.int32), (2, np.uint64)]
    bufs, cols = scatter(raw, E)
    dcols = hip.DeviceBuffer.from_array(cols)
    out = Guarded(shapes)
    hip.upload_ptr(out.ptr[5], np.zeros(1, np.int32))
    gather.ingest_atari_planes_gather(dcols.ptr, T, B, A, *out.ptr)
    hip.synchronize()
    got = out.read(names)
    for nm in ("frames", "mu", "act", "rew", "disc"):
        np.testing.assert_array_equal(got[nm], want[nm], err_msg=nm)
    assert got["bad"][0] == 1
    check_versions(got["versions"], words, T)

    # the contiguous ingest on the same entries in column order
    dev = hip.DeviceBuffer.from_array(raw)
    ref = Guarded(shapes[:5])
    check(lib().fi_ingest_atari_planes(dev.ptr, T, B, A, E, *ref.ptr, None), "fi_ingest_atari_planes")
    hip.synchronize()
    r = ref.read(names[:5])
    for nm in names[:5]:
        np.testing.assert_array_equal(got[nm], r[nm], err_msg=nm + " against the contiguous ingest")
    # without the optional blocks nothing else changes
    gather.ingest_atari_planes_gather(dcols.ptr, T, B, A, *out.ptr[:5])
    hip.synchronize()
    again = out.read(names)
    for nm in names:
        np.testing.assert_array_equal(again[nm], got[nm], err_msg=nm)
    for b in bufs + [dcols, dev]:
        b.free()
    out.free()
    ref.free()


# ------------------------------------------------------------------ 2. the kernels alone, MLP
@pytest.mark.parametrize("D,A", [(3, 2), (128, 64)])
def test_gathering_records_ingest_is_bit_exact(D, A):
    from freeimpala_amd import gather, hip
    from freeimpala_amd._abi import check, lib
    from freeimpala_amd.learner import pack_records
    T, B = 2, 5
    E = (T + 1) * 1024
    rs = np.random.RandomState(D)
    obs = rs.standard_normal((T + 1, B, D)).astype(np.float32)
    mu = rs.standard_normal((T, B, A)).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    act[0, 2] = -1
    rew = rs.standard_normal((T, B)).astype(np.float32)
    disc = (0.99 * (rs.rand(T, B) > 0.3)).astype(np.float32)
    raw = np.stack([np.frombuffer(e, np.uint8) for e in pack_records(obs, mu, act, rew, disc)]).copy()
    words = flag_words(T, B)
    for t in range(T + 1):
        raw[:, t * 1024 + MLP_FLAGS:t * 1024 + MLP_FLAGS + 4] = words[:, t:t + 1].copy().view(np.uint8)
    want = dict(obs=obs.ravel(), mu=mu.ravel(), act=np.clip(act, 0, A - 1).ravel(), rew=rew.ravel(), disc=disc.ravel())
    names = ("obs", "mu", "act", "rew", "disc", "bad", "versions")
    shapes = [((T + 1) * B * D, np.float32), (T * B * A, np.float32), (T * B, np.int32), (T * B, np.float32),
              (T * B, np.float32), (1, np.int32), (2, np.uint64)]
    bufs, cols = scatter(raw, E)
    dcols = hip.DeviceBuffer.from_array(cols)
    out = Guarded(shapes)
    hip.upload_ptr(out.ptr[5], np.zeros(1, np.int32))
    gather.ingest_records_gather(dcols.ptr, T, B, A, D, *out.ptr)
    hip.synchronize()
    got = out.read(names)
    for nm in names[:5]:
        np.testing.assert_array_equal(got[nm], want[nm], err_msg=nm)
    assert got["bad"][0] == 1
    check_versions(got["versions"], words, T)
    dev = hip.DeviceBuffer.from_array(raw)
    ref = Guarded(shapes[:5])
    check(lib().fi_ingest_records(dev.ptr, T, B, A, D, E, *ref.ptr, None), "fi_ingest_records")
    hip.synchronize()
    r = ref.read(names[:5])
    for nm in names[:5]:
        np.testing.assert_array_equal(got[nm], r[nm], err_msg=nm + " against the contiguous ingest")
    for b in bufs + [dcols, dev]:
        b.free()
    out.free()
    ref.free()


# ------------------------------------------------------------------ the shared two-actor runs
A_, T_, SIZES, CALLS, D_, H_ = 6, 3, (1, 3), 10, 5, 32
B_ = sum(SIZES)
VERSIONS = (0, 5)
_runs = {}

TENSORS = {"atari": (("frames", np.uint8),), "mlp": (("obs", np.float32),)}
COMMON = (("logits", np.float32), ("mu", np.float32), ("vs", np.float32), ("values", np.float32),
          ("pg_adv", np.float32), ("actions", np.int32), ("rewards", np.float32), ("discounts", np.float32))


def snapshot(L, stats):
    d = {nm: L.tensor(nm, dt) for nm, dt in TENSORS[L.arch] + COMMON}
    d["params"] = L.get_params()
    d["stats"] = {k: v for k, v in stats.items() if k != "step_ms"}
    return d


def make_learner(arch, optimizer="adam", lr=1e-3, **over):
    from freeimpala_amd.learner import DeviceLearner
    kw = dict(seq_len=T_, batch=B_, num_actions=A_, optimizer=optimizer, lr=lr)
    if arch == "atari":
        kw["records"] = "planes"
    else:
        kw.update(obs_dim=D_, hidden=H_)
    kw.update(over)
    return DeviceLearner(arch, **kw)


def make_actors(arch, p0):
    from freeimpala_amd.actor import Actor
    actors = []
    for k, (n, v) in enumerate(zip(SIZES, VERSIONS)):
        a = Actor(arch, n, num_actions=A_, seed=21 + k) if arch == "atari" else \
            Actor(arch, n, num_actions=A_, obs_dim=D_, hidden=H_, seed=21 + k)
        a.set_params(p0, version=v)
        a.begin_rollout(T_)
        actors.append(a)
    return actors


def inputs(arch):
    """What the environments of both actors return over 10 calls, as one (CALLS, 4, ...) run whose
    columns are the batch's: column 0 is the N = 1 actor's, columns 1..3 the N = 3 actor's."""
    rs = np.random.RandomState(77)
    if arch == "atari":
        x = rs.randint(0, 256, (CALLS, B_, 84, 84)).astype(np.uint8)
        start = np.zeros((CALLS, B_), bool)
        start[0] = True
        start[1, 0] = start[3, 1] = start[4, 3] = start[5, 3] = True  # column 2 never again
    else:
        x = rs.standard_normal((CALLS, B_, D_)).astype(np.float32)
        start = None
    rew = rs.randint(-1, 2, (CALLS, B_)).astype(np.float32)
    disc = (0.99 * (rs.rand(CALLS, B_) > 0.2)).astype(np.float32)
    return x, start, rew, disc


def act_call(a, arch, x, start, rew, disc, j, lo, hi):
    out = a.act_planes(x[j, lo:hi], start[j, lo:hi]) if arch == "atari" else a.act_obs(x[j, lo:hi])
    a.outcome(rew[j, lo:hi], disc[j, lo:hi])
    return out


def two_actor_run(arch):
    """10 act calls of two recording actors (N = 1 with version 0, N = 3 with version 5; T = 3: three
    unrolls, each actor's first buffer used twice). After each completing call: both unrolls read
    back, then three learners from the same parameters -- `still` (lr = 0) through
    step_segments_dev on the acquired buffers, `dev` (Adam) through step_rollouts, `host` (Adam)
    through step() on the concatenated host copies. Everything the tests compare, computed once."""
    if arch in _runs:
        return _runs[arch]
    dev, host, still = make_learner(arch), make_learner(arch), make_learner(arch, "sgd", 0.0)
    p0 = dev.get_params()
    host.set_params(p0)
    still.set_params(p0)
    actors = make_actors(arch, p0)
    x, start, rew, disc = inputs(arch)
    bounds = [(0, SIZES[0]), (SIZES[0], B_)]
    outs, entries, snaps, versions, ready_after = [], [], dict(dev=[], host=[], still=[]), [], []
    for j in range(CALLS):
        outs.append([act_call(a, arch, x, start, rew, disc, j, lo, hi) for a, (lo, hi) in zip(actors, bounds)])
        if not all(a.rollout_ready() for a in actors):
            assert not any(a.rollout_ready() for a in actors)
            continue
        e = [a.read_rollout() for a in actors]
        entries.append(e)
        segs = [a.acquire_rollout() for a in actors]
        segs = [(ptr, stride, a.N, ev) for a, (ptr, stride, ev) in zip(actors, segs)]
        snaps["still"].append(snapshot(still, still.step_segments_dev(segs)))
        assert all(a.rollout_ready() for a in actors)  # step_segments_dev does not release
        snaps["dev"].append(snapshot(dev, dev.step_rollouts(actors)))
        versions.append(dev.batch_versions)
        ready_after.append([a.rollout_ready() for a in actors])
        snaps["host"].append(snapshot(host, host.step([row for part in e for row in part])))
    _runs[arch] = dict(p0=p0, x=x, start=start, rew=rew, disc=disc, outs=outs, entries=entries, snaps=snaps,
                       versions=versions, ready_after=ready_after, bounds=bounds,
                       staging=dict(dev=dev.staging_bytes, host=host.staging_bytes, still=still.staging_bytes))
    for a in actors:
        a.end_rollout()
    for h in actors + [dev, host, still]:
        h.close()
    return _runs[arch]


def flags_of(entries, arch):
    rec, off = (REC, FLAGS) if arch == "atari" else (1024, MLP_FLAGS)
    e = np.asarray(entries)
    return np.stack([e[:, t * rec + off:t * rec + off + 4].copy().view(np.uint32)[:, 0] for t in range(T_ + 1)], 1)


# ------------------------------------------------------------------ 3. two actors = the host copy
@pytest.mark.parametrize("arch", ["atari", "mlp"])
def test_step_from_two_actors_equals_step_from_their_host_copy(arch):
    from freeimpala_amd.learner import pack_atari_plane_records, pack_records
    from freeimpala_amd.rollout import split_unrolls
    r = two_actor_run(arch)
    dev, host = r["snaps"]["dev"], r["snaps"]["host"]
    assert len(dev) == len(host) == 3
    first = "frames" if arch == "atari" else "obs"
    for k, (d, h) in enumerate(zip(dev, host)):
        for nm in (first, "logits", "mu", "vs", "params"):
            np.testing.assert_array_equal(d[nm], h[nm], err_msg=f"unroll {k}: {nm}")
        assert d["stats"] == h["stats"], (k, d["stats"], h["stats"])
        assert d["stats"]["version"] == k + 1
    assert (dev[0]["params"] != r["p0"]).any(), "Adam at lr > 0 moves the parameters"
    assert r["staging"]["dev"] == 0 and r["staging"]["still"] == 0 and r["staging"]["host"] > 0
    for v in r["versions"]:
        assert v == dict(min=0, max=5, mean=15 / 4, count=12)
    assert r["ready_after"] == [[False, False]] * 3
    # the recorded entries themselves, the third unroll (each actor's first buffer again) included
    for i, (lo, hi) in enumerate(r["bounds"]):
        mu = np.stack([o[i]["logits"] for o in r["outs"]])
        act = np.stack([o[i]["actions"] for o in r["outs"]])
        if arch == "atari":
            unrolls = split_unrolls(r["x"][:, lo:hi], r["start"][:, lo:hi], mu, act, r["rew"][:, lo:hi],
                                    r["disc"][:, lo:hi], T_)
            want = [np.stack([np.frombuffer(e, np.uint8) for e in pack_atari_plane_records(*u)]) for u in unrolls]
        else:
            want = [np.stack([np.frombuffer(e, np.uint8) for e in
                              pack_records(r["x"][s:s + T_ + 1, lo:hi], mu[s:s + T_], act[s:s + T_],
                                           r["rew"][s:s + T_, lo:hi], r["disc"][s:s + T_, lo:hi])])
                    for s in range(0, CALLS - 1, T_)]
        rec, off = (REC, FLAGS) if arch == "atari" else (1024, MLP_FLAGS)
        for k in range(3):
            got = r["entries"][k][i].copy()
            w = flags_of(got, arch)
            assert (w[:, :T_] == VERSIONS[i]).all() and (w[:, T_] == 0).all()
            for t in range(T_):
                got[:, t * rec + off:t * rec + off + 4] = 0
            np.testing.assert_array_equal(got, want[k], err_msg=f"actor {i}, unroll {k}")


# ------------------------------------------------------------------ 4. closed loop
def test_closed_loop_over_two_actors(orc):
    """The learner that holds the actors' parameters (lr = 0) recomputes, in actor k's columns, that
    actor's logits and values bit for bit, so pi = mu exactly, in every unroll; vs and pg_adv are the
    oracle's at those logits within 1e-5."""
    r = two_actor_run("atari")
    for k, s in enumerate(r["snaps"]["still"][:2]):
        lo = k * T_
        logits = s["logits"].reshape(T_ + 1, B_, A_)
        values = s["values"].reshape(T_ + 1, B_)
        mu = s["mu"].reshape(T_, B_, A_)
        for i, (c0, c1) in enumerate(r["bounds"]):
            for t in range(T_ + 1):
                o = r["outs"][lo + t][i]
                np.testing.assert_array_equal(logits[t, c0:c1], o["logits"], err_msg=f"actor {i}, call {lo + t}")
                np.testing.assert_array_equal(values[t, c0:c1], o["values"], err_msg=f"actor {i}, call {lo + t}")
        np.testing.assert_array_equal(mu, logits[:T_])
        act = s["actions"].reshape(T_, B_)
        np.testing.assert_array_equal(act, np.stack([np.concatenate([o["actions"] for o in r["outs"][lo + t]])
                                                     for t in range(T_)]))
        np.testing.assert_array_equal(s["rewards"].reshape(T_, B_), r["rew"][lo:lo + T_])
        np.testing.assert_array_equal(s["discounts"].reshape(T_, B_), r["disc"][lo:lo + T_])
        vt = orc.vtrace_loss(logits[:T_], mu, act, r["rew"][lo:lo + T_], r["disc"][lo:lo + T_], values)
        for nm in ("vs", "pg_adv"):
            got = s[nm].reshape(T_, B_)
            err = np.abs(got - vt[nm]).max() / max(1.0, np.abs(vt[nm]).max())
            print(f"closed loop over two actors, unroll {k}: {nm} err {err:.2e}")
            assert err <= 1e-5, (k, nm, err)


# ------------------------------------------------------------------ 5. and 7. one actor, one segment
def one_actor_run():
    """Three identical recording actors (N = B = 3, T = 2, the same seed and inputs: the same
    unrolls) and five Adam learners from the same parameters, over two unrolls:
      roll   step_rollout(a)                          multi  step_rollouts([b])
      async  step_rollouts_async([c]), wait()
      mixed  unroll 0 through step_segments_dev, unroll 1 through step_entries_dev
      plain  step_entries_dev only (mixed and plain read a's buffer before roll releases it)"""
    if "one" in _runs:
        return _runs["one"]
    from freeimpala_amd.actor import Actor
    from freeimpala_amd.learner import DeviceLearner
    N, T, calls = 3, 2, 5
    names = ("roll", "multi", "async", "mixed", "plain")
    L = {nm: DeviceLearner("atari", seq_len=T, batch=N, num_actions=A_, records="planes", optimizer="adam", lr=1e-3)
         for nm in names}
    p0 = L["roll"].get_params()
    for nm in names[1:]:
        L[nm].set_params(p0)
    actors = [Actor("atari", N, num_actions=A_, seed=31) for _ in range(3)]
    for a in actors:
        a.set_params(p0, version=2)
        a.begin_rollout(T)
    rs = np.random.RandomState(91)
    planes = rs.randint(0, 256, (calls, N, 84, 84)).astype(np.uint8)
    start = rs.rand(calls, N) < 0.3
    start[0] = True
    rew = rs.randint(-1, 2, (calls, N)).astype(np.float32)
    disc = (0.99 * (rs.rand(calls, N) > 0.2)).astype(np.float32)
    snaps = {nm: [] for nm in names}
    for j in range(calls):
        for a in actors:
            a.act_planes(planes[j], start[j])
            a.outcome(rew[j], disc[j])
        a, b, c = actors
        if not a.rollout_ready():
            continue
        k = len(snaps["roll"])
        ptr, stride, ev = a.acquire_rollout()
        st = L["mixed"].step_segments_dev([(ptr, stride, N, ev)]) if k == 0 else L["mixed"].step_entries_dev(ptr, stride, ev)
        snaps["mixed"].append(snapshot(L["mixed"], st))
        snaps["plain"].append(snapshot(L["plain"], L["plain"].step_entries_dev(ptr, stride, ev)))
        snaps["roll"].append(snapshot(L["roll"], L["roll"].step_rollout(a)))
        snaps["multi"].append(snapshot(L["multi"], L["multi"].step_rollouts([b])))
        L["async"].step_rollouts_async([c])
        assert not c.rollout_ready()  # released once the step is enqueued
        snaps["async"].append(snapshot(L["async"], L["async"].wait()))
    _runs["one"] = dict(snaps=snaps, versions=L["multi"].batch_versions, count=T * N)
    for a in actors:
        a.end_rollout()
    for h in actors + list(L.values()):
        h.close()
    return _runs["one"]


def same(x, y, what):
    for k, (d, h) in enumerate(zip(x, y)):
        for nm in d:
            if nm == "stats":
                assert d[nm] == h[nm], (what, k, d[nm], h[nm])
            else:
                np.testing.assert_array_equal(d[nm], h[nm], err_msg=f"{what}, unroll {k}: {nm}")


def test_one_actor_as_one_segment_equals_step_rollout():
    r = one_actor_run()
    s = r["snaps"]
    assert len(s["roll"]) == 2
    same(s["multi"], s["roll"], "step_rollouts([a]) against step_rollout(a)")
    same(s["async"], s["multi"], "step_rollouts_async + wait against step_rollouts")
    assert r["versions"] == dict(min=2, max=2, mean=2.0, count=r["count"])


# ------------------------------------------------------------------ 7. the older paths behind a step from segments
def test_step_entries_dev_is_unchanged_behind_a_step_from_segments():
    r = one_actor_run()
    s = r["snaps"]
    same(s["mixed"], s["plain"], "step_segments_dev then step_entries_dev against step_entries_dev alone")
    assert (s["plain"][1]["params"] != s["plain"][0]["params"]).any()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handles_usable():
    from freeimpala_amd._abi import FiError
    r = two_actor_run("atari")
    x, start, rew, disc = r["x"], r["start"], r["rew"], r["disc"]
    L = make_learner("atari")
    L.set_params(r["p0"])
    a1, a3 = make_actors("atari", r["p0"])
    with pytest.raises(FiError, match=r"rc=-4: .*no step from segments"):
        L.batch_versions
    for j in range(T_ + 1):
        act_call(a1, "atari", x, start, rew, disc, j, *r["bounds"][0])
    for j in range(T_):
        act_call(a3, "atari", x, start, rew, disc, j, *r["bounds"][1])
    assert a1.rollout_ready() and not a3.rollout_ready()
    with pytest.raises(FiError, match=r"rc=-4: .*actor 1 has no completed unroll"):
        L.step_rollouts([a1, a3])
    assert a1.rollout_ready()  # nothing was acquired or released
    act_call(a3, "atari", x, start, rew, disc, T_, *r["bounds"][1])
    assert a3.rollout_ready()
    with pytest.raises(FiError, match=rf"rc=-1: .*sum to 3 != the learner's batch {B_}"):
        L.step_rollouts([a3])
    with pytest.raises(FiError, match=r"rc=-1: .*actor 1 is actor 0 again"):
        L.step_rollouts([a3, a3])
    with pytest.raises(FiError, match=r"rc=-1: .*0 actors"):
        L.step_rollouts([])

    (p1, stride, e1), (p3, _, e3) = a1.acquire_rollout(), a3.acquire_rollout()
    good = [(p1, stride, 1, e1), (p3, stride, 3, e3)]
    with pytest.raises(FiError, match=r"rc=-1: .*65 segments"):
        L.step_segments_dev([(p1, stride, 1, e1)] * 65)
    with pytest.raises(FiError, match=r"rc=-1: .*segment 1: num_entries 0 < 1"):
        L.step_segments_dev([good[0], (p3, stride, 0, e3)])
    with pytest.raises(FiError, match=rf"rc=-1: .*the segments hold 3 entries, the learner's batch is {B_}"):
        L.step_segments_dev([good[1]])
    with pytest.raises(FiError, match=r"rc=-1: .*pass the learner's batch"):
        L.step_segments_dev([good[1], good[1]])
    with pytest.raises(FiError, match=r"rc=-1: .*segment 1: .*16-byte aligned"):
        L.step_segments_dev([good[0], (p3, stride + 8, 3, e3)])
    with pytest.raises(FiError, match=r"rc=-1: .*segment 0: .*16-byte aligned"):
        L.step_segments_dev([(p1 + 4, stride, 1, e1), good[1]])
    with pytest.raises(FiError, match=rf"rc=-1: .*segment 1: entry_stride {stride - 16} < {stride}"):
        L.step_segments_dev([good[0], (p3, stride - 16, 3, e3)])
    host_mem = np.zeros(stride + 16, np.uint8)
    with pytest.raises(FiError, match=r"rc=-1: .*segment 0: .*not device memory"):
        L.step_segments_dev([(host_mem.ctypes.data + (-host_mem.ctypes.data) % 16, stride, 1, None), good[1]])
    with pytest.raises(FiError, match=r"rc=-1: .*segment 0: the allocation ends"):  # one entry too short
        L.step_segments_dev([(p3, stride, 4, e3)])
    long = make_learner("atari", seq_len=T_ + 1)
    with pytest.raises(FiError, match=rf"rc=-1: .*actor 0's rollout seq_len {T_} != the learner's {T_ + 1}"):
        long.step_rollouts([a1, a3])
    long.close()
    wide = make_learner("atari", num_actions=A_ + 1)
    with pytest.raises(FiError, match=rf"rc=-1: .*actor 0's num_actions {A_} != the learner's {A_ + 1}"):
        wide.step_rollouts([a1, a3])
    wide.close()
    stacked = make_learner("atari", records="stacked")
    with pytest.raises(FiError, match=r"rc=-1: .*planes format"):
        stacked.step_rollouts([a1, a3])
    with pytest.raises(FiError, match=r"rc=-1: .*planes format"):
        stacked.step_segments_dev(good)
    stacked.close()
    with pytest.raises(FiError, match=r"rc=-4: .*no step from segments"):
        L.batch_versions
    assert a1.rollout_ready() and a3.rollout_ready() and L.staging_bytes == 0

    # every refusal left the unrolls waiting and the learner as it was: the step gives test 3's result
    got = snapshot(L, L.step_rollouts([a1, a3]))
    same([got], [r["snaps"]["dev"][0]], "after the refusals")
    assert L.batch_versions == dict(min=0, max=5, mean=15 / 4, count=12)
    assert not a1.rollout_ready() and not a3.rollout_ready()
    for a in (a1, a3):
        a.end_rollout()
        a.close()
    L.close()


# ------------------------------------------------------------------ 8. C++ wrapper
EXE = os.path.join(ROOT, "build", "host_rollouts_check")


def test_cpp_wrapper_steps_from_two_actors():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_rollouts_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("rollouts ")]
    assert len(lines) == 2 and lines[0].startswith("rollouts mlp:") and lines[1].startswith("rollouts atari:")
    for ln in lines:
        assert ln.endswith("version 1") and "nan" not in ln
