"""The internal host helpers (freeimpala_amd/csrc/host_util.h) through their own check program,
tests/cpp/host_util_check.cpp: the checks of a caller's device pointers, the device allocations,
the exception boundary of a C entry point and the tail of a step that took its batch.

CPU: every refusal that is made before HIP is asked, a host pointer, guarded() and the step tail;
without a device also a refused allocation that leaves HIP's last error cleared. It passes with a GPU
as well. GPU: the span checks against one 4,096-byte allocation, dev_alloc and dev_grow; no kernel
is launched.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "host_util_check")


def _run(mode):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", ROOT, "build/host_util_check"], check=True)
    r = subprocess.run(["timeout", "-k", "10", "60", EXE, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"OK {mode}" in r.stdout


def test_host_util_cpu_mode():
    _run("cpu")


@pytest.mark.gpu
def test_host_util_against_one_allocation():
    _run("gpu")
