"""FarmerLstm's acting branch (include/fi_farmer_act.h) without a device: the exports and the ctypes table, the
configuration's layout against the C compiler, pick_reference on hand-written cases, and the inputs of the GPU cases
(tests/test_gpu_farmer_act.py): act_reference alone says how wide their intervals are."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import atari_ref as R
from test_abi import header_functions
from test_gpu_farmer_act import CASES, case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["max_states", "max_rows", "seq_len", "device", "seed"]


def test_exports_table_and_layout_match_c(tmp_path):
    from freeimpala_amd import _abi, farmer_act
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.lib()._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    names = set(header_functions("fi_farmer_act.h"))
    assert names == set(farmer_act.SIGNATURES) == {s for s in exported if s.startswith("fi_farmer_actor_")}
    assert len(names) == 12
    farmer_act.lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_farmer_act.h"\nint main(){'
           'printf("%zu", sizeof(fi_farmer_actor_config));' +
           "".join(f'printf(" %zu", offsetof(fi_farmer_actor_config, {f}));' for f in FIELDS) + "return 0;}")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()]
    Cfg = farmer_act.FarmerActorConfig
    assert [f for f, _ in Cfg._fields_] == FIELDS
    assert got == [ctypes.sizeof(Cfg)] + [getattr(Cfg, f).offset for f in FIELDS] == [24, 0, 4, 8, 12, 16]
    cfg = Cfg()
    farmer_act.lib().fi_farmer_actor_config_init(ctypes.byref(cfg))
    assert (cfg.max_states, cfg.max_rows, cfg.seq_len, cfg.device, cfg.seed) == (256, 4096, 10, 0, 0)


def test_pick_reference_on_hand_written_cases():
    from freeimpala_amd.env import philox4
    from freeimpala_amd.farmer_act import ST_FARMER_ACT, pick_reference
    #        a tie: lowest row | empty | a NaN and an inf beside the best | only non-finite rows
    values = np.float32([1, 5, 5, 2, np.nan, 7, np.inf, 3, np.nan, -np.inf])
    offsets = [0, 4, 4, 8, 10]
    ref = pick_reference(values, offsets, 0.0, seed=1, draw=0)
    np.testing.assert_array_equal(ref["actions"], [1, -1, 1, -1])
    np.testing.assert_array_equal(ref["best_value"], np.float32([5, -np.inf, 7, -np.inf]))
    assert not ref["explored"].any() and ref["nonfinite"] == 4
    # eps = 1: every decision point takes row (w1 n) >> 32 of its own Philox words, unless that row is not finite
    seed, draw, S = 77, 3, 4
    ref = pick_reference(values, offsets, 1.0, seed, draw)
    w = philox4(seed, np.arange(draw * S, draw * S + S, dtype=np.uint64), ST_FARMER_ACT)
    assert ST_FARMER_ACT == 11 and w.shape == (4, 4)
    j0, j2 = (int(w[0, 1]) * 4) >> 32, (int(w[2, 1]) * 4) >> 32
    assert ref["actions"][0] == j0 and ref["explored"][0] == 1
    assert (ref["actions"][2], ref["explored"][2]) == ((j2, 1) if j2 in (1, 3) else (1, 0))
    assert ref["actions"][1] == ref["actions"][3] == -1 and not ref["explored"][[1, 3]].any()
    # the threshold itself: a decision point explores exactly when w0 2^-32 < eps
    u = float(w[0, 0]) * 2.0 ** -32
    eps = np.float32([np.nextafter(np.float32(u), np.float32(2)), 0, 0, 0])
    assert pick_reference(values, offsets, eps, seed, draw)["explored"][0] == (u < float(eps[0]))
    assert pick_reference(values, offsets, np.float32([np.nextafter(np.float32(u), np.float32(-1)), 0, 0, 0]), seed,
                          draw)["explored"][0] == 0


@pytest.mark.parametrize("T,sizes", CASES, ids=[f"T{T}_S{len(s)}_N{sum(s)}" for T, s in CASES])
def test_gpu_case_inputs_keep_the_intervals_narrow(T, sizes):
    """A condition on the inputs: at most atari_ref.CAP of each stored tensor's (K + c) u S intervals hold more than
    four bf16 values. A case that exceeds it gets other inputs, not another cap."""
    from freeimpala_amd.farmer_act import act_reference
    p, z, x, offsets = case_inputs(T, sizes)
    ref = act_reference(z, x, offsets, p)
    assert ref["c"].shape == (sum(sizes), 612) and np.isfinite(ref["values"]).all()
    wide = {f"a{l + 1}": R.bf16_interval_stats(*ref["pre"][l], 624 if l == 0 else 512, 1, relu=True)[2] for l in range(5)}
    wide["values"] = R.bf16_interval_stats(*ref["values_terms"], 512, 1)[2]
    assert max(wide.values()) <= R.CAP, wide
    assert min(a.mean() for a in ref["a"]) > 0.1  # the activations stay O(1) through the five layers
