"""CPU-side checks of the column weights' ABI (include/fi_weights.h): the in-tree libfi_learner.so
exports every function the header declares, freeimpala_amd.weights binds exactly that set, none of it
is in the eight older headers or their tables, fi_prio_exponents_state has one layout in C and in
ctypes, and the host form of the rule -- is_weights and td_priorities_alpha -- on hand-computed cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h", "fi_gather.h", "fi_ring.h", "fi_prio.h",
                 "fi_env.h")
FUNCTIONS = ("fi_learner_set_column_weights", "fi_learner_clear_column_weights", "fi_learner_column_weights",
             "fi_prio_set_exponents", "fi_prio_exponents", "fi_prio_last_weights", "fi_weights_scale_columns",
             "fi_prio_from_td_alpha", "fi_prio_is_weights")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_weights_header_symbol():
    from freeimpala_amd import _abi, actor, env, farmer, gather, prio, ring, rollout, weights
    lib = weights.lib()
    names = header_functions("fi_weights.h")
    assert names == sorted(FUNCTIONS)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(weights.SIGNATURES), set(names) ^ set(weights.SIGNATURES)
    # a header of its own: the older headers' sets (pinned by their own tests) do not grow
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, farmer.SIGNATURES, actor.SIGNATURES, rollout.SIGNATURES, gather.SIGNATURES,
                  ring.SIGNATURES, prio.SIGNATURES, env.SIGNATURES):
        assert not set(names) & set(table)
    assert len(ring.SIGNATURES) == 14 and len(prio.SIGNATURES) == 9 and lib.fi_abi_version() == 1
    assert [f for f, _ in prio.PrioState._fields_] == ["enabled", "eta", "q_init", "reserved", "prio_hi", "table_bytes"]


def test_exponents_state_layout_matches_c(tmp_path):
    from freeimpala_amd import weights
    fields = [f for f, _ in weights.ExponentsState._fields_]
    assert fields == ["alpha", "beta", "weights_valid", "reserved"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_weights.h"\nint main(){'
           'printf("%zu", sizeof(fi_prio_exponents_state));' +
           "".join(f'printf(" %zu", offsetof(fi_prio_exponents_state, {f}));' for f in fields) +
           'printf(" %zu", sizeof(fi_prio_state));}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    assert got[:-1] == [ctypes.sizeof(weights.ExponentsState)] + [getattr(weights.ExponentsState, f).offset for f in fields]
    assert got[:-1] == [16, 0, 4, 8, 12]
    assert got[-1] == 32, "fi_prio_state is what it was"
    assert weights.ExponentsState(0.5, 0.25, 1, 0).as_dict() == dict(alpha=0.5, beta=0.25, weights_valid=True)


def test_is_weights_by_hand():
    """Window q = (1, 1, 2), n_valid = 3, Q = 4, beta = 1, one fresh column and three replayed ones
    that name the entries 0, 1, 2: ratio = (3/4, 3/4, 3/2), u = (1, 4/3, 4/3, 2/3), w = u / (4/3)."""
    from freeimpala_amd.weights import is_weights
    window = np.array([1, 1, 2])
    q_cols = np.concatenate([[12345], window[[0, 1, 2]]])  # the fresh column's value is not read
    w = is_weights(q_cols, 1, 3, int(window.sum()), 1.0)
    assert w.dtype == np.float64
    np.testing.assert_array_equal(w, [0.75, 1.0, 1.0, 0.5])
    # beta = 1/2: u = (1, (3/4)^-1/2, ., (3/2)^-1/2)
    w = is_weights(q_cols, 1, 3, 4, 0.5)
    m = 0.75 ** -0.5
    np.testing.assert_allclose(w, [1 / m, 1.0, 1.0, 1.5 ** -0.5 / m], rtol=1e-15)
    # every replayed entry above the mean priority: the fresh columns hold the maximum
    w = is_weights([7, 7, 2, 2], 2, 3, 4, 1.0)
    np.testing.assert_array_equal(w, [1.0, 1.0, 2 / 3, 2 / 3])
    assert w.max() == 1.0


def test_is_weights_neutral_cases():
    from freeimpala_amd.prio import Q_MAX
    from freeimpala_amd.weights import is_weights
    q = np.array([3, 1, Q_MAX, 65536, 9])
    np.testing.assert_array_equal(is_weights(q, 2, 1000, int(q.sum()) + 5000, 0.0), np.ones(5))  # beta = 0
    np.testing.assert_array_equal(is_weights(q, 5, 0, 0, 0.7), np.ones(5))  # n_fresh = B: no window is needed
    np.testing.assert_array_equal(is_weights([5], 0, 1, 5, 1.0), [1.0])  # one entry: ratio = 1
    np.testing.assert_array_equal(is_weights([4, 4, 4], 0, 8, 32, 0.4), np.ones(3))  # a uniform table
    # the largest totals the rule allows: 2^20 entries of Q_MAX, exact in fp64 up to the one rounding
    w = is_weights([Q_MAX, 1], 0, 2 ** 20, (2 ** 20 - 1) * Q_MAX + 1, 1.0)
    assert w[1] == 1.0 and 0 < w[0] < 1e-9
    with pytest.raises(ValueError, match="beta"):
        is_weights(q, 2, 10, 100, 1.5)
    with pytest.raises(ValueError, match="n_fresh"):
        is_weights(q, 6, 10, 100, 0.5)
    with pytest.raises(ValueError, match=">= 1"):
        is_weights([1, 0], 0, 2, 1, 0.5)


def test_td_priorities_alpha():
    from freeimpala_amd.prio import Q_MAX, td_priorities
    from freeimpala_amd.weights import td_priorities_alpha
    vs = np.array([[1.0, 0.0, 2.0, np.nan, np.inf], [0.0, 0.0, 5.0, 1.0, 0.0]], np.float32)
    values = np.array([[0.5, 0.0, 1.0, 0.0, 0.0], [0.25, 0.0, 1.0, 0.0, 0.0], [9.0] * 5], np.float32)  # T + 1 rows
    # d = (0.5, 0.25), (0, 0), (1, 4), (nan, 1), (inf, 0)
    for eta in (0.0, 0.5, 0.9, 1.0):
        np.testing.assert_array_equal(td_priorities_alpha(vs, values, eta, 1.0), td_priorities(vs, values, eta))
        # alpha = 0: p^0 = 1 for every finite column, p = 0 included; a NaN column stays Q_MAX
        assert list(td_priorities_alpha(vs, values, eta, 0.0))[:4] == [65536, 65536, 65536, Q_MAX]
    # the Inf column: p = Inf for 0 < eta < 1 and Inf^0 = 1; with eta = 0 or 1 one term is 0 * Inf = NaN
    assert td_priorities_alpha(vs, values, 0.5, 0.0)[4] == 65536 and td_priorities_alpha(vs, values, 0.5, 0.6)[4] == Q_MAX
    assert td_priorities_alpha(vs, values, 1.0, 0.0)[4] == Q_MAX and td_priorities_alpha(vs, values, 0.0, 0.0)[4] == Q_MAX
    # eta = 1: p = (0.5, 0, 4, nan, 0 * inf = nan); alpha = 1/2: sqrt
    assert list(td_priorities_alpha(vs, values, 1.0, 0.5)) == [int(np.rint(0.5 ** 0.5 * 65536)), 1, 2 * 65536, Q_MAX, Q_MAX]
    # above the table's range before the exponent, inside it behind: 40000^0.5 = 200
    big = np.array([[40000.0]], np.float32)
    assert td_priorities(big, np.zeros((2, 1), np.float32), 1.0)[0] == Q_MAX
    assert td_priorities_alpha(big, np.zeros((2, 1), np.float32), 1.0, 0.5)[0] == 200 * 65536
    with pytest.raises(ValueError, match="alpha"):
        td_priorities_alpha(vs, values, 0.9, 1.25)
