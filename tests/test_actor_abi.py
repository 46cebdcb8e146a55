"""CPU-side checks of the acting ABI (include/fi_actor.h): the in-tree libfi_learner.so exports
every function the header declares, freeimpala_amd.actor binds exactly that set, and
fi_actor_config has one layout in C and in ctypes."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_actor_header_symbol():
    from freeimpala_amd import _abi, actor
    lib = actor.lib()
    names = header_functions("fi_actor.h")
    for must in ("fi_actor_create", "fi_actor_set_params", "fi_actor_act_obs", "fi_actor_act_frames",
                 "fi_actor_act_planes", "fi_actor_read_stacks", "fi_push_planes", "fi_sample_actions"):
        assert must in names, must
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(actor.SIGNATURES), set(names) ^ set(actor.SIGNATURES)
    # a header of its own: fi_learner.h's set (pinned by test_abi.py) does not grow
    assert not set(names) & set(_abi.SIGNATURES)
    assert not set(names) & set(header_functions("fi_learner.h"))


def test_actor_config_layout_matches_c(tmp_path):
    from freeimpala_amd import actor
    fields = [f for f, _ in actor.ActorConfig._fields_]
    assert fields == ["struct_size", "arch", "num_envs", "num_actions", "obs_dim", "hidden", "device", "mode",
                      "seed"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_actor.h"\nint main(){printf("%zu", '
           'sizeof(fi_actor_config));' +
           "".join(f'printf(" %zu", offsetof(fi_actor_config, {f}));' for f in fields) +
           'printf(" %d %d", (int)FI_ACT_SAMPLE, (int)FI_ACT_GREEDY);}')
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    exp = ([ctypes.sizeof(actor.ActorConfig)] + [getattr(actor.ActorConfig, f).offset for f in fields] +
           [actor.FI_ACT_SAMPLE, actor.FI_ACT_GREEDY])
    assert got == exp
    assert got[0] == 40


def test_config_init_sets_the_struct_size_and_defaults():
    """fi_actor_config_init runs without a device."""
    from freeimpala_amd import actor
    cfg = actor.ActorConfig()
    actor.lib().fi_actor_config_init(ctypes.byref(cfg))
    assert cfg.struct_size == ctypes.sizeof(actor.ActorConfig)
    assert (cfg.num_envs, cfg.num_actions, cfg.obs_dim, cfg.hidden, cfg.mode) == (1, 18, 128, 256, 0)
