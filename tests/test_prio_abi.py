"""CPU-side checks of prioritised replay's ABI (include/fi_prio.h): the in-tree libfi_learner.so exports
every function the header declares, freeimpala_amd.prio binds exactly that set, none of it is in the
six older headers or their tables, fi_prio_state has one layout in C and in ctypes, and the host form
of the rule -- quantize_priority, td_priorities, prio_batch_entries -- with the oracle's philox4."""
import bisect
import ctypes
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h")
FUNCTIONS = ("fi_prio_enable", "fi_prio_info", "fi_prio_read", "fi_prio_set", "fi_learner_step_ring_prioritized",
             "fi_learner_step_ring_prioritized_async", "fi_prio_from_td", "fi_prio_scatter", "fi_prio_fill_columns")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_prio_header_symbol():
    from freeimpala_amd import _abi, actor, farmer, gather, prio, ring, rollout
    lib = prio.lib()
    names = header_functions("fi_prio.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(prio.SIGNATURES), set(names) ^ set(prio.SIGNATURES)
    # a header of its own: the older headers' sets (pinned by their own tests) do not grow
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, farmer.SIGNATURES, actor.SIGNATURES, rollout.SIGNATURES, gather.SIGNATURES,
                  ring.SIGNATURES):
        assert not set(names) & set(table)
    assert len(ring.SIGNATURES) == 14 and lib.fi_abi_version() == 1


def test_prio_state_layout_matches_c(tmp_path):
    from freeimpala_amd import prio
    fields = [f for f, _ in prio.PrioState._fields_]
    assert fields == ["enabled", "eta", "q_init", "reserved", "prio_hi", "table_bytes"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_prio.h"\nint main(){'
           'printf("%zu", sizeof(fi_prio_state));' +
           "".join(f'printf(" %zu", offsetof(fi_prio_state, {f}));' for f in fields) +
           'printf(" %u %d", FI_PRIO_Q_MAX, FI_PRIO_MAX_CAPACITY);}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert got[:-2] == [ctypes.sizeof(prio.PrioState)] + [getattr(prio.PrioState, f).offset for f in fields]
    assert got[:-2] == [32, 0, 4, 8, 12, 16, 24]
    assert got[-2:] == [prio.Q_MAX, prio.MAX_CAPACITY] == [2 ** 31 - 1, 2 ** 20]
    assert prio.PrioState(1, 0.5, 65536, 0, 9, 64).as_dict() == dict(enabled=True, eta=0.5, q_init=65536, prio_hi=9,
                                                                    table_bytes=64)


def test_quantize_priority():
    from freeimpala_amd.prio import Q_MAX, quantize_priority
    assert quantize_priority(0.0) == 1
    assert quantize_priority(0.5) == 32768
    assert quantize_priority(1.0) == 65536
    for p in (32768.0, 1e6, float("nan"), float("inf")):
        assert quantize_priority(p) == Q_MAX == 2 ** 31 - 1, p
    assert quantize_priority(32768.0 - 2.0 ** -16) == 2 ** 31 - 1  # the largest value below the threshold
    assert quantize_priority(32768.0 - 2.0 ** -15) == 2 ** 31 - 2
    # ties to even, as rintf: k + 1/2 quanta go to the even neighbour
    assert quantize_priority(2.5 / 65536) == 2 and quantize_priority(3.5 / 65536) == 4
    assert quantize_priority(0.5 / 65536) == 1 and quantize_priority(1.5 / 65536) == 2  # 0 -> the floor of 1
    np.testing.assert_array_equal(quantize_priority(np.array([0.0, 0.5, np.nan, 40000.0])), [1, 32768, Q_MAX, Q_MAX])


def test_td_priorities_is_eta_max_plus_mean():
    from freeimpala_amd.prio import Q_MAX, td_priorities
    vs = np.array([[1.0, 0.0, 2.0, np.nan], [0.0, 0.0, 5.0, 1.0]], np.float32)
    values = np.array([[0.5, 0.0, 1.0, 0.0], [0.25, 0.0, 1.0, 0.0], [9.0, 9.0, 9.0, 9.0]], np.float32)  # T + 1 rows
    # d = (0.5, 0.25), (0, 0), (1, 4), (nan, 1)
    assert list(td_priorities(vs, values, 1.0)) == [32768, 1, 4 * 65536, Q_MAX]
    assert list(td_priorities(vs, values, 0.0)) == [int(0.375 * 65536), 1, int(2.5 * 65536), Q_MAX]
    assert list(td_priorities(vs, values, 0.5)) == [int(0.4375 * 65536), 1, int(3.25 * 65536), Q_MAX]


def brute(q, r):
    run = 0
    for j, v in enumerate(q):
        run += int(v)
        if run > r:
            return j
    raise AssertionError("r is not below the total")


def test_draw_takes_the_first_entry_whose_sum_exceeds_r(orc):
    """Window (1, 1, 1): r = 0, 1, 2 give the entries lo, lo + 1, lo + 2 -- with >= in place of >
    every one of them would move down by one."""
    from freeimpala_amd.prio import prio_batch_entries
    head, tail, C = 14, 9, 8  # lo = 6
    seen = {}
    for draw in range(40):
        e = prio_batch_entries(orc.philox4, 3, draw, 5, 0, head, tail, C, [1, 1, 1])
        for c, x in enumerate(e):
            w = orc.philox4(3, draw * 5 + c, 8)
            r = (((int(w[0]) << 32) | int(w[1])) * 3) >> 64
            assert x == 6 + r, (draw, c)
            seen[r] = x
    assert seen == {0: 6, 1: 7, 2: 8}


def test_sums_stay_exact_with_one_q_max_among_ones(orc):
    from freeimpala_amd.prio import Q_MAX, prio_batch_entries
    n = 2 ** 20
    q = np.ones(n, np.uint32)
    at = 777_777
    q[at] = Q_MAX
    cum = list(itertools.accumulate(int(v) for v in q))  # Python ints
    total = cum[-1]
    assert total == Q_MAX + n - 1
    head, tail = 5 * n + 3, 5 * n + 3  # lo = 4 n + 3: the window is the whole ring and wraps
    got = prio_batch_entries(orc.philox4, 11, 2, 64, 0, head, tail, n, q)
    want = []
    for c in range(64):
        w = orc.philox4(11, 2 * 64 + c, 8)
        r = (((int(w[0]) << 32) | int(w[1])) * total) >> 64
        want.append(head - n + bisect.bisect_right(cum, r))
    assert got == want
    assert brute(q[:at + 2], at - 1) == at - 1 and brute(q[:at + 2], at) == at and brute(q[:at + 2], at + Q_MAX - 1) == at
    # the heavy entry holds all but 2^20 - 1 of the total 2^31 + 2^20 - 2: nearly every column names it
    assert got.count(head - n + at) >= 60


def test_one_replayable_entry_is_always_drawn(orc):
    from freeimpala_amd.prio import Q_MAX, prio_batch_entries
    for qv in (1, 12345, Q_MAX):
        for draw in (0, 1, 2 ** 40):
            assert prio_batch_entries(orc.philox4, 5, draw, 4, 1, 10, 1, 16, [qv]) == [1, 0, 0, 0]
    with pytest.raises(ValueError, match="nothing to replay"):
        prio_batch_entries(orc.philox4, 0, 0, 4, 3, 5, 0, 8, [])
    with pytest.raises(ValueError, match="unread"):
        prio_batch_entries(orc.philox4, 0, 0, 4, 4, 8, 5, 8, [1] * 5)
    with pytest.raises(ValueError, match="outside 1"):
        prio_batch_entries(orc.philox4, 0, 0, 4, 0, 8, 5, 8, [1, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="2\\^20"):
        prio_batch_entries(orc.philox4, 0, 0, 4, 0, 8, 5, 2 ** 20 + 1, [1] * 5)


def test_draw_is_a_function_of_seed_draw_column_and_window(orc):
    from freeimpala_amd import prio
    assert prio.ST_PRIO == 8
    B, head, tail, C = 6, 21, 14, 16  # lo = 5, n_valid = 9
    q = [3, 1, 4, 1, 5, 9, 2, 6, 5]
    for seed, draw in ((9, 0), (9, 3), (2 ** 64 - 1, 2 ** 64 - 1)):
        want = []
        for c in range(B):
            w = orc.philox4(seed, (draw * B + c) % 2 ** 64, 8)
            want.append(5 + brute(q, ((((int(w[0]) << 32) | int(w[1])) * sum(q)) >> 64)))
        for n_fresh in range(B + 1):
            got = prio.prio_batch_entries(orc.philox4, seed, draw, B, n_fresh, head, tail, C, q)
            assert got[:n_fresh] == list(range(tail, tail + n_fresh)) and got[n_fresh:] == want[n_fresh:]
        moved = prio.prio_batch_entries(orc.philox4, seed, draw, B, 0, head + 100, tail + 100, C, q)
        assert [m - 100 for m in moved] == want
    a = prio.prio_batch_entries(orc.philox4, 9, 0, B, 0, head, tail, C, q)
    assert a != prio.prio_batch_entries(orc.philox4, 9, 1, B, 0, head, tail, C, q)
    assert a != prio.prio_batch_entries(orc.philox4, 10, 0, B, 0, head, tail, C, q)
    assert a != prio.prio_batch_entries(orc.philox4, 9, 0, B, 0, head, tail, C, q[::-1])


def test_frequencies_follow_the_priorities(orc):
    """Window (1, 2, 5), seed 0, draws 0 .. 3999 of B = 5 columns: 20,000 draws; every entry's count
    within 5 sigma of its binomial expectation (2,500 / 5,000 / 12,500)."""
    from freeimpala_amd.prio import prio_batch_entries
    q, n = (1, 2, 5), 20000
    counts = [0, 0, 0]
    for draw in range(4000):
        for e in prio_batch_entries(orc.philox4, 0, draw, 5, 0, 3, 3, 8, q):
            counts[e] += 1
    assert sum(counts) == n
    for k, c in enumerate(counts):
        p = q[k] / 8
        assert abs(c - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (k, counts)
