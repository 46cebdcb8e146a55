"""Prioritised replay for the device entry ring (include/fi_prio.h): the three standalone kernels
against the host rule (freeimpala_amd/prio.py), a learner that takes prioritised steps from a ring
against one fed the same entries from the host, the refresh of the table, the refusals, and the
older paths behind a prioritised step.

The draw is integer arithmetic and compared exactly. A priority computed from vs and values is
compared with the fp64 rule on the same fp32 inputs within 1 + q (T + 6) 2^-24: every term is
non-negative (no cancellation), there are T + 6 fp32 roundings (one per |.|, T sum steps, the
divide, two products, one add) and rint adds one quantum."""
import numpy as np
import pytest

from test_gpu_ring import (B, T, Guarded, act_call, learner_pair, make_actor, make_entries, make_learner, same, snapshot,
                           spaced)

pytestmark = pytest.mark.gpu

Q_MAX = 2 ** 31 - 1
ETA = 0.9


def bar(q_ref, t):
    return 1 + q_ref * (t + 6) * 2.0 ** -24


# ------------------------------------------------------------------ 1. priorities from vs and values
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (100, 70)])
def test_from_td_equals_the_fp64_rule(shape):
    from freeimpala_amd import hip, prio
    Tc, Bc = shape
    rs = np.random.RandomState(Tc * 1000 + Bc)
    scale = (10.0 ** rs.uniform(-6, 2, Bc)).astype(np.float32)  # columns of very different magnitude
    values = (rs.standard_normal((Tc + 1, Bc)) * scale).astype(np.float32)
    vs = (values[:Tc] + rs.standard_normal((Tc, Bc)) * scale).astype(np.float32)
    special = {}
    if Bc >= 5:
        vs[:, 0] = values[:Tc, 0]  # every difference 0 -> the floor of 1
        vs[Tc // 2, 1] = np.nan
        vs[Tc - 1, 2] = np.inf
        vs[:, 3] = values[:Tc, 3] + np.float32(1e6)  # at every step: the mean passes 32768 as the maximum does
        special = {0: 1, 1: Q_MAX, 2: Q_MAX, 3: Q_MAX}
    dv, dval = hip.DeviceBuffer.from_array(vs), hip.DeviceBuffer.from_array(values)
    for eta in (0.0, 0.9, 1.0):
        out = Guarded([(Bc, np.uint32)])
        prio.from_td(dv.ptr, dval.ptr, Tc, Bc, eta, out.ptr[0])
        hip.synchronize()
        got = out.read(("q",))["q"].astype(np.int64)
        out.free()
        want = prio.td_priorities(vs, values, eta)
        for b, q in special.items():
            assert want[b] == q and got[b] == q, (eta, b, got[b], want[b])
        err = np.abs(got - want)
        worst = int(np.argmax(err - bar(want, Tc)))
        print(f"T {Tc} B {Bc} eta {eta}: worst column {worst}: dev {got[worst]} ref {want[worst]} bar {bar(want[worst], Tc):.2f}")
        assert (err <= bar(want, Tc)).all(), (eta, worst, got[worst], want[worst])
        assert (got >= 1).all() and (got <= Q_MAX).all()
    dv.free()
    dval.free()


# ------------------------------------------------------------------ 2. the draw alone
def draw_case(orc, Bc, C, n_fresh, head, tail, seed, draw, table, E=1024):
    """table: (C,) uint32 by slot. The device's cols / entries / versions against prio_batch_entries."""
    from freeimpala_amd import hip, prio
    lo = max(0, head - C)
    n_valid = tail - lo
    window = table[(lo + np.arange(n_valid)) % C]
    want = prio.prio_batch_entries(orc.philox4, seed, draw, Bc, n_fresh, head, tail, C, window)
    base = 0x7F0000001000  # never read: the kernel only computes addresses
    dt, ws = hip.DeviceBuffer.from_array(table), hip.DeviceBuffer(prio.CHUNK_WS_BYTES)
    out = Guarded([(Bc, np.uint64), (Bc, np.uint64), (2, np.uint64)])
    prio.fill_columns(out.ptr[0], out.ptr[1], out.ptr[2], base, E, C, Bc, n_fresh, tail, lo, n_valid, dt.ptr, ws.ptr,
                      seed, draw)
    hip.synchronize()
    got = out.read(("cols", "entries", "versions"))
    np.testing.assert_array_equal(dt.download(np.uint32, (C,)), table, err_msg="the draw writes no priority")
    for h in (out, dt, ws):
        h.free()
    np.testing.assert_array_equal(got["entries"], np.array(want, np.uint64))
    np.testing.assert_array_equal(got["cols"], np.array([base + (e % C) * E for e in want], np.uint64))
    np.testing.assert_array_equal(got["versions"].view(np.uint32), np.array([0xFFFFFFFF, 0, 0, 0], np.uint32))
    assert want[:n_fresh] == list(range(tail, tail + n_fresh)) and all(lo <= e < tail for e in want[n_fresh:])
    return want


def table_with(C, lo, q_window, rest=0xDEADBEEF):
    """(C,) uint32: q_window at the slots of the entries lo .., a value no draw may use elsewhere."""
    t = np.full(C, rest, np.uint32)
    t[(lo + np.arange(len(q_window))) % C] = q_window
    return t


def test_draw_across_a_wrap_and_with_one_entry(orc):
    from freeimpala_amd.prio import prio_batch_entries
    C, head, tail = 8, 14, 9  # lo = 6: the window is the slots 6, 7, 0
    q = [1, 7, 2]
    # a seed whose batch at n_fresh = 3 replays one entry twice
    seed = next(s for s in range(1, 200) if len(set(prio_batch_entries(orc.philox4, s, 2, B, 3, head, tail, C, q)[3:])) == 1)
    for n_fresh in (0, 3, 5):
        draw_case(orc, B, C, n_fresh, head, tail, seed, 2, table_with(C, 6, q))
    # (1, 1, 1): the three values of r give the three entries
    seen = set()
    for draw in range(6):
        seen.update(draw_case(orc, B, C, 0, head, tail, 3, draw, table_with(C, 6, [1, 1, 1])))
    assert seen == {6, 7, 8}
    for qv in (1, Q_MAX):  # n_valid = 1
        assert draw_case(orc, B, C, 2, 4, 1, 5, 0, table_with(C, 0, [qv])) == [1, 2, 0, 0, 0]


@pytest.mark.parametrize("n_valid", [1023, 1024, 1027, 2049])
def test_draw_around_the_chunk_size(orc, n_valid):
    C = 4096
    rs = np.random.RandomState(n_valid)
    lo = C - 1000  # the window wraps
    q = rs.randint(1, 2 ** 16 + 1, n_valid).astype(np.uint32)
    e = draw_case(orc, 64, C, 3, lo + C, lo + n_valid, 21, 4, table_with(C, lo, q))
    assert len(set(e)) > 40
    # every weight in the window's last entry: the last position of the last chunk is reached
    q = np.ones(n_valid, np.uint32)
    q[-1] = Q_MAX
    e = draw_case(orc, 64, C, 0, lo + C, lo + n_valid, 22, 0, table_with(C, lo, q))
    assert e.count(lo + n_valid - 1) >= 60


def test_draw_with_more_chunks_than_lanes(orc):
    C, n_valid = 2 ** 17, 65 * 1024 + 5
    lo = C + 70000  # slots 70000 .. 2^17 - 1, then 0 .. 5492
    assert (lo + n_valid) % C < lo % C
    rs = np.random.RandomState(65)
    q = rs.randint(1, 2 ** 16 + 1, n_valid).astype(np.uint32)
    e = draw_case(orc, 64, C, 2, lo + C, lo + n_valid, 31, 7, table_with(C, lo, q))
    assert max(e[2:]) - lo >= 64 * 1024 or len(set(x - lo >> 10 for x in e[2:])) > 20
    # the weight in the 66th chunk, which lane 4 holds as its second sum
    q = np.ones(n_valid, np.uint32)
    q[65 * 1024 + 2] = 2 ** 30
    e = draw_case(orc, 64, C, 0, lo + C, lo + n_valid, 32, 0, table_with(C, lo, q))
    assert e.count(lo + 65 * 1024 + 2) >= 60


def test_draw_from_a_full_ring_of_q_max(orc):
    C = 2 ** 20
    head = tail = C + 12345  # the whole ring is replayable and the window wraps
    e = draw_case(orc, 64, C, 0, head, tail, 41, 1, np.full(C, Q_MAX, np.uint32), E=16)
    assert len(set(x - 12345 >> 10 for x in e)) > 50, "the draws spread over the chunks"


def test_draw_of_256_columns_and_a_heavy_entry_in_the_last_chunk(orc):
    C, n_valid = 4096, 3000
    rs = np.random.RandomState(256)
    q = rs.randint(1, 2 ** 16 + 1, n_valid).astype(np.uint32)
    e = draw_case(orc, 256, C, 100, 500 + C, 500 + n_valid, 51, 9, table_with(C, 500, q))
    assert len(set(e[100:])) > 100
    n_valid = 5000
    q = np.ones(n_valid, np.uint32)
    q[4990] = 2 ** 20  # in the last chunk, which holds 904 positions
    e = draw_case(orc, 64, 8192, 0, 5000, 5000, 52, 0, table_with(8192, 0, q))
    assert e.count(4990) >= 32, "2^20 of the total 2^20 + 4999"


# ------------------------------------------------------------------ 3. the refresh alone
def test_scatter_takes_the_maximum_over_duplicates():
    from freeimpala_amd import hip, prio

    def case(C, entries, q):
        rs = np.random.RandomState(C)
        before = rs.randint(1, 2 ** 31, C).astype(np.uint32)
        tab = Guarded([(C, np.uint32)])
        hip.upload_ptr(tab.ptr[0], before)
        de = hip.DeviceBuffer.from_array(np.array(entries, np.uint64))
        dq = hip.DeviceBuffer.from_array(np.array(q, np.uint32))
        prio.scatter(tab.ptr[0], C, de.ptr, dq.ptr, len(entries))
        hip.synchronize()
        got = tab.read(("table",))["table"]
        want = before.copy()
        slots = np.array(entries, np.uint64) % np.uint64(C)
        want[slots.astype(np.int64)] = 0
        np.maximum.at(want, slots.astype(np.int64), np.array(q, np.uint32))
        np.testing.assert_array_equal(got, want)
        for h in (tab, de, dq):
            h.free()
        return got, before

    got, before = case(16, [3, 19, 35, 5, 2 ** 40 + 6], [10, 99, 50, 7, Q_MAX])  # 3, 19, 35: slot 3, three times
    assert got[3] == 99 and got[5] == 7 and got[6] == Q_MAX
    untouched = [s for s in range(16) if s not in (3, 5, 6)]
    np.testing.assert_array_equal(got[untouched], before[untouched])
    # more than one workgroup, many duplicates; a smaller value replaces a larger old one
    rs = np.random.RandomState(7)
    got, before = case(64, rs.randint(0, 1000, 300).tolist(), rs.randint(1, 100, 300).tolist())
    assert (got < 100).sum() >= 60 and (before >= 100).all()


# ------------------------------------------------------------------ 4. end to end
def lo_of(i):
    return max(0, i["head"] - i["capacity"])


def prio_step(orc, R, Hh, ring, raw, n_fresh, wait=True, pick_duplicate=False):
    """One prioritised step of R from the ring, checked against the host rule on the window read
    back before it, the host-fed learner Hh, and the fp64 refresh. Returns the chosen entries."""
    from freeimpala_amd.prio import prio_batch_entries, td_priorities
    i = ring.info()
    C, lo = i["capacity"], lo_of(i)
    window = ring.priorities() if i["tail"] > lo else np.zeros(0, np.uint32)
    seed = i["seed"]
    if pick_duplicate:  # a seed for which this batch replays one entry at least twice
        seed = next(s for s in range(1, 400) if len(set(
            prio_batch_entries(orc.philox4, s, i["draw"], B, n_fresh, i["head"], i["tail"], C, window)[n_fresh:])) < B - n_fresh)
        ring.seed(seed, i["draw"])
    want = prio_batch_entries(orc.philox4, seed, i["draw"], B, n_fresh, i["head"], i["tail"], C, window)
    st = R.step_ring(ring, n_fresh=n_fresh, wait=wait, prioritized=True)
    if not wait:
        st = R.wait()
    assert ring.last_entries(B) == want
    same(snapshot(R, st), snapshot(Hh, Hh.step([raw[e] for e in want])), f"prioritised step, n_fresh {n_fresh}")
    after = ring.info()
    assert (after["head"], after["tail"], after["draw"]) == (i["head"], i["tail"] + n_fresh, i["draw"] + 1)
    assert ring.priority_info()["prio_hi"] == i["tail"] + n_fresh
    # the refresh: every named entry holds the maximum over the columns that name it, every other
    # resident one what it held
    q_cols = td_priorities(R.tensor("vs").reshape(T, B), R.tensor("values").reshape(T + 1, B), ETA)
    q_init = ring.priority_info()["q_init"]
    now = ring.priorities().astype(np.int64)
    for e in range(lo, after["tail"]):
        cols = [b for b in range(B) if want[b] == e]
        if cols:
            ref = int(max(q_cols[b] for b in cols))
            print(f"entry {e}: columns {cols}: dev {now[e - lo]} ref {ref} bar {bar(ref, T):.2f}")
            assert abs(int(now[e - lo]) - ref) <= bar(ref, T), (e, cols, now[e - lo], ref)
        else:
            assert now[e - lo] == (window[e - lo] if e < i["tail"] else q_init), e
    return want


@pytest.mark.parametrize("arch,A", [("mlp", 3), ("atari", 18)])
def test_prioritised_steps_equal_the_host_rule_and_the_host_fed_learner(arch, A, orc):
    from freeimpala_amd.prio import prio_batch_entries, quantize_priority
    from freeimpala_amd.ring import EntryRing
    C = 16
    raw, _ = make_entries(arch, 15, A, seed=100 + A)
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    ring = EntryRing(E, C, seed=17)
    ring.enable_priorities(ETA, 1.0)
    q_init = quantize_priority(1.0)
    assert ring.priority_info() == dict(enabled=True, eta=float(np.float32(ETA)), q_init=65536, prio_hi=0, table_bytes=4 * C)
    src = spaced(raw[:10], E + 48)
    ring.push(src.ptr, E + 48, 10)
    assert prio_step(orc, R, Hh, ring, raw, 5) == [0, 1, 2, 3, 4]
    e = prio_step(orc, R, Hh, ring, raw, 2, pick_duplicate=True)
    assert e[:2] == [5, 6] and len(set(e[2:])) < 3
    prio_step(orc, R, Hh, ring, raw, 0)
    assert R.batch_versions["count"] == T * B
    # a uniform step in between leaves the table alone; what it took as fresh reads as q_init
    src2 = spaced(raw[10:], E + 48)
    ring.push(src2.ptr, E + 48, 5)
    before = ring.priorities()
    assert len(before) == 7 and ring.priority_info()["prio_hi"] == 7
    same(snapshot(R, R.step_ring(ring, n_fresh=3)),
         snapshot(Hh, Hh.step([raw[x] for x in ring.last_entries(B)])), "uniform step in between")
    assert ring.last_entries(B)[:3] == [7, 8, 9]
    assert ring.priority_info()["prio_hi"] == 7 and ring.info()["tail"] == 10
    np.testing.assert_array_equal(ring.priorities(), np.concatenate([before, [q_init] * 3]).astype(np.uint32))
    prio_step(orc, R, Hh, ring, raw, 0)  # fills 7, 8, 9: prio_hi = 10 (checked inside)
    # one entry at 2^20 among ones: every replayed column names it
    heavy = 4
    ring.set_priorities(0, [2 ** 20 if x == heavy else 1 for x in range(10)])
    i = ring.info()
    assert prio_batch_entries(orc.philox4, i["seed"], i["draw"], B, 0, i["head"], i["tail"], C, ring.priorities()) == [heavy] * B
    assert prio_step(orc, R, Hh, ring, raw, 0) == [heavy] * B
    q = ring.priorities()
    assert (np.delete(q, heavy) == 1).all() and q[heavy] != 2 ** 20
    for h in (src, src2):
        h.free()
    for h in (ring, R, Hh):
        h.close()


def test_async_steps_leave_the_same_table():
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, 10, A, seed=120)
    tables = []
    for wait in (True, False):
        R = make_learner(arch, A)
        E = R.entry_bytes
        ring = EntryRing(E, 16, seed=5)
        ring.enable_priorities(ETA, 0.25)
        src = spaced(raw, E)
        ring.push(src.ptr, E, 10)
        chosen = []
        for n_fresh in (5, 2, 0, 3):
            st = R.step_ring(ring, n_fresh=n_fresh, wait=wait, prioritized=True)
            assert (st is None) == (not wait)
            if not wait:
                R.wait()
            chosen.append(ring.last_entries(B))
        tables.append((ring.priorities(), chosen, R.get_params(), ring.priority_info()))
        src.free()
        ring.close()
        R.close()
    np.testing.assert_array_equal(tables[0][0], tables[1][0])
    assert tables[0][1] == tables[1][1] and tables[0][3] == tables[1][3]
    np.testing.assert_array_equal(tables[0][2], tables[1][2])
    assert len(set(int(q) for q in tables[0][0])) > 3, "the table holds refreshed values"


@pytest.mark.parametrize("wait", [True, False])
def test_a_step_that_skips_its_update_still_refreshes(wait):
    """A NaN reward in one entry: the step returns FI_ERR_NONFINITE (-7), the batch counts as taken,
    that entry's priority becomes Q_MAX and the finite columns get their value."""
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.prio import td_priorities
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, B, A, seed=125)
    raw[2, 1024 + 772:1024 + 776] = np.array([np.nan], np.float32).view(np.uint8)  # entry 2, record 1: the reward
    R = make_learner(arch, A)
    E = R.entry_bytes
    ring = EntryRing(E, 8, seed=4)
    ring.enable_priorities(ETA, 1.0)
    src = spaced(raw, E)
    ring.push(src.ptr, E, B)
    p0 = R.get_params()
    with pytest.raises(FiError, match=r"rc=-7.*not finite"):
        R.step_ring(ring, prioritized=True, wait=wait)
        R.wait()
    np.testing.assert_array_equal(R.get_params(), p0)
    i = ring.info()
    assert (i["tail"], i["draw"], ring.priority_info()["prio_hi"]) == (B, 1, B) and ring.last_entries(B) == list(range(B))
    vs, values = R.tensor("vs").reshape(T, B), R.tensor("values").reshape(T + 1, B)
    assert np.isnan(vs[:, 2]).any() and np.isfinite(np.delete(vs, 2, axis=1)).all()
    want, got = td_priorities(vs, values, ETA), ring.priorities().astype(np.int64)
    assert want[2] == Q_MAX and got[2] == Q_MAX
    assert (np.abs(got - want) <= bar(want, T)).all() and (np.delete(got, 2) < Q_MAX).all(), (got, want)
    for h in (ring, R):
        h.close()
    src.free()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_ring_and_table_as_they_were():
    from freeimpala_amd._abi import FiError
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    raw, _ = make_entries(arch, 10, A, seed=130)
    R, Hh = learner_pair(arch, A)
    E = R.entry_bytes
    src = spaced(raw, E)
    big = EntryRing(16, 2 ** 20 + 1)
    with pytest.raises(FiError, match=r"rc=-1: .*capacity 1048577 above 2\^20"):
        big.enable_priorities()
    assert big.priority_info()["enabled"] is False
    big.close()
    ring = EntryRing(E, 16, seed=2)
    ring.push(src.ptr, E, 10)

    def refused(match, call, *args, **kw):
        before = ring.info(), ring.priority_info()
        table = ring.priorities() if before[1]["enabled"] and before[0]["tail"] > lo_of(before[0]) else None
        with pytest.raises(FiError, match=match):
            call(*args, **kw)
        assert (ring.info(), ring.priority_info()) == before
        if table is not None:
            np.testing.assert_array_equal(ring.priorities(), table)

    refused(r"rc=-4: .*priorities are not enabled", R.step_ring, ring, prioritized=True)
    refused(r"rc=-4: .*priorities are not enabled", R.step_ring, ring, prioritized=True, wait=False)
    refused(r"rc=-4: .*priorities are not enabled", ring.priorities, 0, 1)
    refused(r"rc=-1: .*eta 1.5\d* outside \[0, 1\]", ring.enable_priorities, 1.5)
    refused(r"rc=-1: .*eta -0.1\d* outside \[0, 1\]", ring.enable_priorities, -0.1)
    refused(r"rc=-1: .*init_priority -1.0\d* is negative or not finite", ring.enable_priorities, 0.9, -1.0)
    refused(r"rc=-1: .*init_priority (inf|nan)", ring.enable_priorities, 0.9, float("inf"))
    ring.enable_priorities(ETA, 1.0)
    refused(r"rc=-4: .*enabled already", ring.enable_priorities, ETA, 1.0)
    # every refusal of step_ring, with its status
    refused(rf"rc=-4: .*nothing to replay: 2 columns of the batch {B}", R.step_ring, ring, n_fresh=3, prioritized=True)
    refused(rf"rc=-1: .*n_fresh {B + 1} outside 0 .. batch {B}", R.step_ring, ring, n_fresh=B + 1, prioritized=True)
    refused(rf"rc=-1: .*n_fresh -1 outside 0 .. batch {B}", R.step_ring, ring, n_fresh=-1, prioritized=True, wait=False)
    refused(r"rc=-1: .*entries 0 .. 1 outside the replayable \[0, 0\)", ring.priorities, 0, 1)
    R.step_ring(ring, prioritized=True)
    six = make_learner(arch, A, batch=6)
    refused(r"rc=-4: .*5 entries unread, n_fresh = 6", six.step_ring, ring, prioritized=True)
    six.close()
    refused(r"rc=-1: .*entries 3 .. 6 outside the replayable \[0, 5\)", ring.priorities, 3, 3)
    refused(r"rc=-1: .*entries 5 .. 6 outside the replayable \[0, 5\)", ring.set_priorities, 5, [7])
    refused(r"rc=-1: .*entries 0 .. 0 outside the replayable", ring.priorities, 0, 0)
    refused(r"rc=-1: .*value 0 at index 1 outside 1 .. 2\^31-1", ring.set_priorities, 0, [5, 0, 5])
    refused(r"rc=-1: .*value 2147483648 at index 0", ring.set_priorities, 4, [2 ** 31])
    refused(r"rc=-1: .*a second learner handle", Hh.step_ring, ring, n_fresh=2, prioritized=True)
    refused(r"rc=-1: .*a second learner handle", Hh.step_ring, ring, n_fresh=2, prioritized=True, wait=False)
    # the uniform step is any learner's; the owner goes on where every refusal left it
    Hh.set_params(R.get_params())
    R.step_ring(ring, n_fresh=2, prioritized=True)
    assert ring.info()["tail"] == 7 and ring.info()["draw"] == 2 and ring.priority_info()["prio_hi"] == 7
    for h in (ring, R, Hh):
        h.close()
    src.free()


# ------------------------------------------------------------------ 6. the older paths behind a prioritised step
def test_older_paths_are_unchanged_behind_a_prioritised_step():
    """One handle takes prioritised ring steps, then a uniform ring step, step_rollouts and the
    resident step; before each, a fresh handle is given its state and takes only that path."""
    from freeimpala_amd.ring import EntryRing
    arch, A = "mlp", 3
    X = make_learner(arch, A)
    E = X.entry_bytes
    raw, _ = make_entries(arch, 10, A, seed=140)
    src = spaced(raw, E)
    ring = EntryRing(E, 16, seed=3)
    ring.enable_priorities(ETA, 1.0)
    ring.push(src.ptr, E, 10)
    X.step_ring(ring, prioritized=True)
    X.step_ring(ring, n_fresh=2, prioritized=True)
    rs_x, rs_y = np.random.RandomState(141), np.random.RandomState(141)
    ax, ay = (make_actor(arch, B, A, X.get_params(), 2, seed=142) for _ in range(2))  # the same unrolls
    for _ in range(T + 1):
        act_call(ax, arch, rs_x)
        act_call(ay, arch, rs_y)

    def fresh():
        Y = make_learner(arch, A)
        Y.load_state(X.save_state())
        return Y

    # the uniform step on the same ring (X) against a ring of its own that holds the same three entries
    Y = fresh()
    got = snapshot(X, X.step_ring(ring, n_fresh=3))
    chosen = ring.last_entries(B)
    assert chosen[:3] == [7, 8, 9]
    same(got, snapshot(Y, Y.step([raw[e] for e in chosen])), "uniform ring step")
    Y.close()
    Y = fresh()
    same(snapshot(X, X.step_rollouts([ax])), snapshot(Y, Y.step_rollouts([ay])), "rollouts")
    same(snapshot(X, X.step_resident()), snapshot(Y, Y.step_resident()), "resident")
    assert X.staging_bytes == 0
    Y.close()
    for a in (ax, ay):
        a.end_rollout()
        a.close()
    ring.close()
    X.close()
    src.free()
