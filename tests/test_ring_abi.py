"""CPU-side checks of the device entry ring's ABI (include/fi_ring.h): the in-tree libfi_learner.so
exports every function the header declares, freeimpala_amd.ring binds exactly that set, none of it
is in the five older headers or their tables, fi_ring_state has one layout in C and in ctypes, and
ring_batch_entries -- the host form of the batch rule -- with the oracle's philox4."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_ring_header_symbol():
    from freeimpala_amd import _abi, actor, farmer, gather, ring, rollout
    lib = ring.lib()
    names = header_functions("fi_ring.h")
    for must in ("fi_ring_create", "fi_ring_destroy", "fi_ring_info", "fi_ring_seed", "fi_ring_push",
                 "fi_ring_pushed_event", "fi_ring_stream", "fi_ring_push_rollout", "fi_ring_read_slots",
                 "fi_ring_last_entries", "fi_learner_step_ring", "fi_learner_step_ring_async", "fi_ring_copy_entries",
                 "fi_ring_fill_columns"):
        assert must in names, must
    assert len(names) == 14
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(ring.SIGNATURES), set(names) ^ set(ring.SIGNATURES)
    # a header of its own: the older headers' sets (pinned by their own tests) do not grow
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, farmer.SIGNATURES, actor.SIGNATURES, rollout.SIGNATURES, gather.SIGNATURES):
        assert not set(names) & set(table)


def test_ring_state_layout_matches_c(tmp_path):
    from freeimpala_amd import ring
    fields = [f for f, _ in ring.RingState._fields_]
    assert fields == ["capacity", "entry_bytes", "head", "tail", "draw", "seed"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_ring.h"\nint main(){'
           'printf("%zu", sizeof(fi_ring_state));' +
           "".join(f'printf(" %zu", offsetof(fi_ring_state, {f}));' for f in fields) + "}")
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert got == [ctypes.sizeof(ring.RingState)] + [getattr(ring.RingState, f).offset for f in fields]
    assert got == [48, 0, 8, 16, 24, 32, 40]
    assert ring.RingState(8, 16, 13, 7, 2, 5).as_dict() == dict(capacity=8, entry_bytes=16, head=13, tail=7, draw=2, seed=5)


def test_fifo_batch_is_the_next_b_entries(orc):
    from freeimpala_amd.ring import ring_batch_entries
    calls = []

    def no_draw(*a):
        calls.append(a)
        raise AssertionError("a FIFO batch draws nothing")

    for head, tail, C in ((5, 0, 8), (13, 8, 8), (2 ** 40 + 9, 2 ** 40, 16)):
        assert ring_batch_entries(no_draw, 3, 7, 5, 5, head, tail, C) == list(range(tail, tail + 5))
    assert not calls


def test_replayed_entries_are_resident_and_read(orc):
    """Every replayed index lies in [lo, tail), whatever the seed and the draw; with one replayable
    entry every replayed column names it; the draws cover the range."""
    from freeimpala_amd.ring import ring_batch_entries
    B = 5
    for head, tail, C in ((8, 5, 8), (13, 8, 8), (13, 6, 8), (2 ** 33 + 20, 2 ** 33 + 10, 64), (3, 1, 8)):
        lo = max(0, head - C)
        seen = set()
        for seed in (0, 1, 2 ** 63 + 11):
            for draw in (0, 1, 2 ** 40):
                for n_fresh in (0, 2):
                    e = ring_batch_entries(orc.philox4, seed, draw, B, n_fresh, head, tail, C)
                    assert len(e) == B and e[:n_fresh] == list(range(tail, tail + n_fresh))
                    assert all(lo <= x < tail for x in e[n_fresh:]), (head, tail, C, e)
                    seen.update(e[n_fresh:])
        assert seen == set(range(lo, tail)) or tail - lo > 40, (head, tail, C, sorted(seen))
    with pytest.raises(ValueError, match="unread"):
        ring_batch_entries(orc.philox4, 0, 0, B, 4, 8, 5, 8)
    with pytest.raises(ValueError, match="nothing to replay"):
        ring_batch_entries(orc.philox4, 0, 0, B, 4, 5, 0, 8)
    with pytest.raises(ValueError, match="outside"):
        ring_batch_entries(orc.philox4, 0, 0, B, 6, 8, 0, 8)


def test_replay_draw_is_a_function_of_seed_draw_and_column(orc):
    """Column c's draw is the first word of philox4(seed, draw * B + c, 7): the fresh columns before
    it, and the ring's counters at equal n_valid, do not enter."""
    from freeimpala_amd import ring
    assert ring.ST_REPLAY == 7
    B, head, tail, C = 6, 21, 14, 16          # lo = 5, n_valid = 9
    lo, n_valid = 5, 9
    for seed, draw in ((9, 0), (9, 3), (2 ** 64 - 1, 2 ** 64 - 1)):
        want = [lo + ((int(orc.philox4(seed, (draw * B + c) % 2 ** 64, 7)[0]) * n_valid) >> 32) for c in range(B)]
        for n_fresh in range(B + 1):
            got = ring.ring_batch_entries(orc.philox4, seed, draw, B, n_fresh, head, tail, C)
            assert got[n_fresh:] == want[n_fresh:], (seed, draw, n_fresh)
        # the same offsets into another window of the same width
        moved = ring.ring_batch_entries(orc.philox4, seed, draw, B, 0, head + 100, tail + 100, C)
        assert [m - 100 for m in moved] == want
    a = ring.ring_batch_entries(orc.philox4, 9, 0, B, 0, head, tail, C)
    b = ring.ring_batch_entries(orc.philox4, 9, 1, B, 0, head, tail, C)
    c = ring.ring_batch_entries(orc.philox4, 10, 0, B, 0, head, tail, C)
    assert a != b and a != c
