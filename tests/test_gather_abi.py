"""CPU-side checks of the gathering ABI (include/fi_gather.h): the in-tree libfi_learner.so exports
every function the header declares, freeimpala_amd.gather binds exactly that set, none of it is in
the four older headers or their tables, and fi_entry_segment / fi_batch_versions have one layout in
C and in ctypes."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("fi_learner.h", "fi_farmer.h", "fi_actor.h", "fi_rollout.h")


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_gather_header_symbol():
    from freeimpala_amd import _abi, actor, farmer, gather, rollout
    lib = gather.lib()
    names = header_functions("fi_gather.h")
    for must in ("fi_learner_step_segments_dev", "fi_learner_step_segments_dev_async", "fi_learner_batch_versions",
                 "fi_learner_step_rollouts", "fi_learner_step_rollouts_async", "fi_ingest_atari_planes_gather",
                 "fi_ingest_records_gather"):
        assert must in names, must
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(gather.SIGNATURES), set(names) ^ set(gather.SIGNATURES)
    # a header of its own: the older headers' sets (pinned by their own tests) do not grow
    for other in OTHER_HEADERS:
        assert not set(names) & set(header_functions(other)), other
    for table in (_abi.SIGNATURES, farmer.SIGNATURES, actor.SIGNATURES, rollout.SIGNATURES):
        assert not set(names) & set(table)


def test_segment_and_versions_layouts_match_c(tmp_path):
    from freeimpala_amd import gather
    seg = [f for f, _ in gather.EntrySegment._fields_]
    ver = [f for f, _ in gather.BatchVersions._fields_]
    assert seg == ["entries_dev", "entry_stride", "num_entries", "ready_event"]
    assert ver == ["min_version", "max_version", "sum_versions", "count"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "fi_gather.h"\nint main(){'
           'printf("%zu %zu %d", sizeof(fi_entry_segment), sizeof(fi_batch_versions), (int)FI_MAX_SEGMENTS);' +
           "".join(f'printf(" %zu", offsetof(fi_entry_segment, {f}));' for f in seg) +
           "".join(f'printf(" %zu", offsetof(fi_batch_versions, {f}));' for f in ver) + "}")
    c = tmp_path / "s.c"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout
    got = [int(v) for v in out.split()]
    exp = ([ctypes.sizeof(gather.EntrySegment), ctypes.sizeof(gather.BatchVersions), gather.FI_MAX_SEGMENTS] +
           [getattr(gather.EntrySegment, f).offset for f in seg] +
           [getattr(gather.BatchVersions, f).offset for f in ver])
    assert got == exp
    assert got[:3] == [32, 24, 64]


def test_batch_versions_as_dict():
    from freeimpala_amd import gather
    bv = gather.BatchVersions(0, 5, 45, 12)
    assert bv.as_dict() == dict(min=0, max=5, mean=15 / 4, count=12)
