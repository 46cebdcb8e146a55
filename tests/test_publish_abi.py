"""CPU-side checks of the device publication's ABI (include/fi_publish.h): the in-tree
libfi_learner.so exports exactly the functions the header declares, freeimpala_amd.publish binds
exactly that set, none of it is in an older header or table, fi_publish_state has one layout in C and
in ctypes, and round_params -- the host form of the rounding rule -- on hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h", "fi_train.h", "fi_breakout.h")
FUNCTIONS = ("fi_publish_params", "fi_publish_read", "fi_publish_get_state", "fi_publish_event",
             "fi_actor_set_params_ptr", "fi_actor_set_params_dev", "fi_actor_read_params", "fi_publish_copy")
FIELDS = ["publications", "tag", "version", "slot", "dtype", "readers"]


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_publish_header():
    from freeimpala_amd import _abi, actor, breakout, env, farmer, gather, prio, publish, ring, rollout, train, weights
    lib = publish.lib()
    names = header_functions("fi_publish.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(publish.SIGNATURES), set(names) ^ set(publish.SIGNATURES)
    # the library's publication symbols are the header's: nothing else named fi_publish_* is exported
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert {s for s in exported if s.startswith("fi_publish_")} == {n for n in names if n.startswith("fi_publish_")}
    assert set(names) <= exported
    # a header of its own: no older header and no older table gains a function
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for mod in (_abi, farmer, actor, rollout, gather, ring, prio, weights, env, train, breakout):
        assert not set(names) & set(mod.SIGNATURES), mod.__name__
    assert len(actor.SIGNATURES) == 17 and len(train.SIGNATURES) == 8
    assert lib.fi_abi_version() == 1


def test_publish_state_layout_matches_c(tmp_path):
    from freeimpala_amd import publish
    assert [f for f, _ in publish.PublishState._fields_] == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_publish.h"\nint main(){'
           'printf("%zu", sizeof(fi_publish_state));' +
           "".join(f'printf(" %zu", offsetof(fi_publish_state, {f}));' for f in FIELDS) +
           'printf(" %d %d", FI_PUBLISH_MAX_READERS, FI_MAX_SEGMENTS);}')
    c = tmp_path / "s.c"
    c.write_text('#include "fi_gather.h"\n' + src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert got[:-2] == [ctypes.sizeof(publish.PublishState)] + [getattr(publish.PublishState, f).offset for f in FIELDS]
    assert got[:-2] == [40, 0, 8, 16, 24, 28, 32]
    assert got[-2] == got[-1] == publish.FI_PUBLISH_MAX_READERS == 64
    st = publish.PublishState(4, 7, 6, 1, 1, (ctypes.c_uint32 * 2)(2, 0))
    assert st.as_dict() == dict(publications=4, tag=7, version=6, slot=1, dtype="bf16", readers=[2, 0])


def _bits(words):
    return np.array(words, np.uint32).view(np.float32)


def test_round_params_by_hand():
    from freeimpala_amd.publish import round_params
    cases = [
        (0x3f808000, 0x3f800000),  # a tie, the kept half even: down
        (0x3f818000, 0x3f820000),  # a tie, the kept half odd: up
        (0x3f808001, 0x3f810000),  # just above the tie
        (0x3f807fff, 0x3f800000),  # just below it
        (0x7f7fffff, 0x7f800000),  # the largest finite fp32 rounds to +Inf
        (0xff7fffff, 0xff800000),
        (0x7f800000, 0x7f800000),  # +-Inf
        (0xff800000, 0xff800000),
        (0x80000000, 0x80000000),  # -0.0
        (0x00000000, 0x00000000),
        (0x00000001, 0x00000000),  # the smallest denormal: to zero
        (0x00018000, 0x00020000),  # a denormal on a tie, odd: up, still a denormal
        (0x807fffff, 0x80800000),  # the largest denormal rounds to the smallest normal, sign kept
        (0x7f800001, 0x7fc00000),  # a signalling NaN with its payload in the lower half: quiet, not Inf
        (0xff800001, 0xffc00000),  # and its sign is kept
        (0x7fa00000, 0x7fa00000),  # a signalling NaN whose payload survives: untouched
        (0xffc12345, 0xffc10000),  # a quiet NaN: bit 6 is set already
        (0x3f800000, 0x3f800000),  # 1.0
    ]
    x = _bits([a for a, _ in cases])
    got = round_params(x, "bf16")
    assert got.dtype == np.float32 and got.shape == x.shape and got is not x
    assert [hex(v) for v in got.view(np.uint32)] == [hex(b) for _, b in cases]
    assert np.isnan(got[13]) and np.isnan(got[14]) and np.signbit(got[14]) and np.isposinf(got[4])
    # fp32 mode: the input's bits, NaN payloads included, as a copy
    same = round_params(x, "fp32")
    assert same is not x and not np.shares_memory(same, x)
    np.testing.assert_array_equal(same.view(np.uint32), x.view(np.uint32))
    # idempotent, shape kept, and the rule of the blob path: f2bf then u << 16
    np.testing.assert_array_equal(round_params(got, "bf16").view(np.uint32), got.view(np.uint32))
    assert round_params(np.zeros((3, 5), np.float32), 1).shape == (3, 5)
    rs = np.random.RandomState(5)
    r = rs.standard_normal(4099).astype(np.float32)
    u = r.view(np.uint32).astype(np.uint64)
    want = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    np.testing.assert_array_equal(round_params(r, "bf16").view(np.uint32), want)
    with pytest.raises(ValueError):
        round_params(x, "fp16")
