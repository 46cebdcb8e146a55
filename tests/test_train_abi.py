"""CPU-side checks of the training recipe's ABI (include/fi_train.h): the in-tree libfi_learner.so
exports every function the header declares, freeimpala_amd.train binds exactly that set, none of it
is in the nine older headers or their tables, fi_train_state has one layout in C and in ctypes, and the
host forms of the three rules -- rmsprop_reference against torch.optim.RMSprop in fp64, lr_at and
clip_rewards on hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_weights.h", "fi_env.h")
FUNCTIONS = ("fi_train_set_rmsprop", "fi_train_set_lr", "fi_train_set_lr_schedule", "fi_train_clear_lr_schedule",
             "fi_train_set_reward_clip", "fi_train_get_state", "fi_train_rmsprop_update", "fi_train_clip_rewards")
FIELDS = ["optimizer", "eps_in_sqrt", "decay", "momentum", "eps", "lr_base", "lr_end", "lr_next", "reward_clip",
          "schedule_on", "lr_steps", "next_update"]


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_train_header_symbol():
    from freeimpala_amd import _abi, actor, env, farmer, gather, prio, ring, rollout, train, weights
    lib = train.lib()
    names = header_functions("fi_train.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(train.SIGNATURES), set(names) ^ set(train.SIGNATURES)
    # a header of its own: the older headers' sets (pinned by their own tests) do not grow
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, farmer.SIGNATURES, actor.SIGNATURES, rollout.SIGNATURES, gather.SIGNATURES,
                  ring.SIGNATURES, prio.SIGNATURES, weights.SIGNATURES, env.SIGNATURES):
        assert not set(names) & set(table)
    assert len(ring.SIGNATURES) == 14 and len(prio.SIGNATURES) == 9 and len(weights.SIGNATURES) == 9
    assert lib.fi_abi_version() == 1


def test_train_state_layout_matches_c(tmp_path):
    from freeimpala_amd import train
    assert [f for f, _ in train.TrainState._fields_] == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_train.h"\nint main(){'
           'printf("%zu", sizeof(fi_train_state));' +
           "".join(f'printf(" %zu", offsetof(fi_train_state, {f}));' for f in FIELDS) +
           'printf(" %d", FI_TRAIN_OPT_RMSPROP);}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert got[:-1] == [ctypes.sizeof(train.TrainState)] + [getattr(train.TrainState, f).offset for f in FIELDS]
    assert got[:-1] == [56] + list(range(0, 40, 4)) + [40, 48]
    assert got[-1] == train.FI_TRAIN_OPT_RMSPROP == 2
    d = train.TrainState(2, 1, 0.5, 0.25, 0.125, 1.0, 0.0, 0.75, 2.0, 1, 8, 3).as_dict()
    assert d == dict(optimizer="rmsprop", eps_in_sqrt=True, decay=0.5, momentum=0.25, eps=0.125, lr_base=1.0, lr_end=0.0,
                     lr_next=0.75, reward_clip=2.0, schedule_on=1, lr_steps=8, next_update=3)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_reference_is_torch_rmsprop_in_fp64(momentum):
    """Four steps of n = 1027 elements, gradients of magnitude 1e-4 .. 10 and mixed sign, against
    torch.optim.RMSprop (eps outside the root) on the CPU in fp64: max |dp| <= 1e-12. Both evaluate
    the same handful of fp64 operations per element on numbers of order 1, so they agree to a few
    2^-53; the bound leaves four decimal digits above that."""
    import torch
    from freeimpala_amd.train import rmsprop_reference
    n, lr, decay, eps = 1027, 4.8e-4, 0.99, 0.01
    rs = np.random.RandomState(1027 + int(momentum * 10))
    p = rs.standard_normal(n)
    tp = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.RMSprop([tp], lr=lr, alpha=decay, eps=eps, momentum=momentum)
    v = np.zeros(n)
    m = np.zeros(n) if momentum else None
    worst = 0.0
    for _ in range(4):
        g = 10.0 ** rs.uniform(-4, 1, n) * rs.choice([-1.0, 1.0], n)
        assert 1e-4 <= np.abs(g).min() and np.abs(g).max() <= 10
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, v, m = rmsprop_reference(p, g, v, m, lr, decay, momentum, eps, False, 1.0)
        assert p.dtype == np.float64 and v.dtype == np.float64
        worst = max(worst, float(np.abs(tp.detach().numpy() - p).max()))
        st = opt.state[tp]
        np.testing.assert_allclose(st["square_avg"].numpy(), v, rtol=1e-14, atol=0)
        if momentum:
            np.testing.assert_allclose(st["momentum_buffer"].numpy(), m, rtol=1e-13, atol=1e-300)
    print(f"momentum {momentum}: max |dp| {worst:.3e}")
    assert worst <= 1e-12
    if not momentum:
        assert m is None, "momentum 0 hands m back untouched"


def test_rmsprop_reference_by_hand():
    from freeimpala_amd.train import rmsprop_reference
    # eps inside the root, with a scale: g' = 4 * 0.5 = 2; v = 0.75 * 5 + 0.25 * 4 = 4.75;
    # d = sqrt(4.75 + 1.5) = 2.5; u = 0.8; m = 0.5 * 0.4 + 0.8 = 1; p = 3 - 0.25 * 1 = 2.75
    p, v, m = rmsprop_reference([3.0], [4.0], [5.0], [0.4], 0.25, 0.75, 0.5, 1.5, True, 0.5)
    assert (p[0], v[0], m[0]) == (2.75, 4.75, 1.0)
    # the same element with eps outside the root: d = sqrt(4.75) + 1.5
    p, v, m = rmsprop_reference([3.0], [4.0], [5.0], [0.4], 0.25, 0.75, 0.5, 1.5, False, 0.5)
    d = np.sqrt(4.75) + 1.5
    assert v[0] == 4.75 and m[0] == 0.2 + 2.0 / d and p[0] == 3.0 - 0.25 * (0.2 + 2.0 / d)
    # momentum 0: p = 3 - 0.25 * 0.8, m handed back as it came
    sentinel = np.array([123.0])
    p, v, m = rmsprop_reference([3.0], [4.0], [5.0], sentinel, 0.25, 0.75, 0.0, 1.5, True, 0.5)
    assert p[0] == 3.0 - 0.25 * 0.8 and m is sentinel
    # a zero gradient from v = 0: v stays 0, d = eps, p does not move
    p, v, _ = rmsprop_reference([1.0], [0.0], [0.0], None, 0.1, 0.9, 0.0, 0.01)
    assert (p[0], v[0]) == (1.0, 0.0)


def test_lr_at():
    from freeimpala_amd.train import lr_at
    b, e = np.float32(4.8e-4), np.float32(1e-5)
    assert lr_at(1, 4.8e-4, 1e-5, 2000) == float(b), "update 1 runs at lr_base"
    assert lr_at(2001, 4.8e-4, 1e-5, 2000) == float(e) and lr_at(10 ** 9, 4.8e-4, 1e-5, 2000) == float(e)
    assert lr_at(2000, 4.8e-4, 1e-5, 2000) != float(e), "update n_steps is one step short of lr_end"
    # the midpoint: update n/2 + 1 has taken n/2 of the n steps
    assert lr_at(1001, 4.8e-4, 1e-5, 2000) == float(np.float32(float(b) + (float(e) - float(b)) * 1000.0 / 2000.0))
    assert lr_at(3, 1.0, 0.5, 4) == 0.75 and lr_at(2, 1.0, 0.0, 2) == 0.5
    # lr_end = 0, and a rising line
    assert lr_at(1, 0.25, 0.0, 2) == 0.25 and lr_at(3, 0.25, 0.0, 2) == 0.0 and lr_at(4, 0.25, 0.0, 2) == 0.0
    assert lr_at(2, 0.0, 1.0, 4) == 0.25
    # n_steps = 1: update 1 at lr_base, everything behind it at lr_end
    assert lr_at(1, 0.5, 0.125, 1) == 0.5 and lr_at(2, 0.5, 0.125, 1) == 0.125
    # every value is an fp32 number, monotone between the two ends
    line = [lr_at(s, 4.8e-4, 0.0, 7) for s in range(1, 10)]
    assert all(x == float(np.float32(x)) for x in line) and all(x > y for x, y in zip(line[:7], line[1:8])) and line[7:] == [0.0, 0.0]
    with pytest.raises(ValueError):
        lr_at(0, 1.0, 0.0, 5)
    with pytest.raises(ValueError):
        lr_at(1, 1.0, 0.0, 0)


def test_clip_rewards():
    from freeimpala_amd.train import clip_rewards
    c = np.float32(0.7)
    r = np.array([np.nan, np.inf, -np.inf, c, -c, -0.0, 0.3, 2 * c], np.float32)
    out = clip_rewards(r, 0.7)
    assert out.dtype == np.float32 and out is not r
    assert np.isnan(out[0]), "a NaN stays a NaN"
    np.testing.assert_array_equal(out[1:], np.array([c, -c, c, -c, -0.0, 0.3, c], np.float32))
    assert np.signbit(out[5]) and out[5] == 0, "-0.0 keeps its sign"
    assert out[0:1].view(np.uint32)[0] == r[0:1].view(np.uint32)[0], "the NaN's own bits"
    np.testing.assert_array_equal(clip_rewards(out, 0.7).view(np.uint32), out.view(np.uint32), err_msg="idempotent")
    np.testing.assert_array_equal(clip_rewards(np.float32([[1.5, -0.25], [-3.0, 0.0]]), 1.0), np.float32([[1.0, -0.25], [-1.0, 0.0]]))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            clip_rewards(r, bad)
