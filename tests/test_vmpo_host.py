"""CPU-side checks of the V-MPO objective (include/fi_vmpo.h): the library exports the header's functions and
freeimpala_amd.vmpo binds exactly that set; the two structures' sizes and offsets; every refusal of the stand-alone
entry points comes before a device call (there is no device here); and the references against the definitions they
must satisfy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # an aligned non-null address that a refused call never follows


def test_library_exports_the_header():
    from freeimpala_amd import vmpo
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fi_vmpo.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(fi_vmpo_[a-z0-9_]+)\s*\(", src))
    assert names == set(vmpo.SIGNATURES) and len(names) == 10
    assert not [n for n in names if not hasattr(vmpo.lib(), n)]


def test_struct_sizes_and_offsets():
    from freeimpala_amd import vmpo
    assert C.sizeof(vmpo.VmpoParams) == 32 and C.sizeof(vmpo.VmpoState) == vmpo.STATE_BYTES == 88
    assert {k: getattr(vmpo.VmpoState, k).offset for k in vmpo.OFFSETS} == vmpo.OFFSETS
    assert [getattr(vmpo.VmpoParams, k).offset for k, _ in vmpo.VmpoParams._fields_] == [0, 4, 8, 12, 16, 20, 24]
    header = open(os.path.join(ROOT, "include", "fi_vmpo.h")).read()
    assert f"FI_VMPO_SELECT_WS_BYTES {vmpo.SELECT_WS_BYTES}u" in header


def test_workspace_bytes_and_blocks():
    from freeimpala_amd import vmpo
    assert [vmpo.workspace_bytes(*s) for s in ((5, 24, 1), (5, 24, 65), (0, 24, 18))] == [0, 0, 0]
    assert [vmpo.select_blocks(n) for n in (0, 1, 1024, 1025, 4097, 70001, 262144, 2 ** 31 - 1, 2 ** 31)] == \
        [0, 1, 1, 1, 4, 69, 256, 256, 0]


BAD_PARAMS = [dict(top_fraction=0.0), dict(top_fraction=1.5), dict(top_fraction=float("nan")), dict(eps_eta=0.0),
              dict(eps_eta=float("inf")), dict(eta_min=0.0), dict(eta_init=1e-9), dict(lr_eta=-1.0), dict(adapt=2)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_parameters_are_refused_before_a_device_call(bad):
    from freeimpala_amd import _abi, vmpo
    from freeimpala_amd._abi import FiError
    prm = vmpo.params()
    for k, v in bad.items():
        setattr(prm, k, v)
    hp = _abi.VtraceHparams()
    calls = [lambda: vmpo.select_dev(100, FAKE, prm, FAKE, FAKE, vmpo.SELECT_WS_BYTES),
             lambda: vmpo.vmpo_loss_dev(5, 20, 3, FAKE, FAKE, FAKE, FAKE, FAKE, hp, prm, FAKE, FAKE, FAKE, None, FAKE, 1 << 20),
             lambda: vmpo.eta_step_dev(FAKE, prm),
             lambda: _abi.check(vmpo.lib().fi_vmpo_enable(FAKE, C.byref(prm)), "fi_vmpo_enable")]
    for call in calls:
        with pytest.raises(FiError, match=r"rc=-1: .*" + next(iter(bad))):
            call()


def test_bad_arguments_are_refused_before_a_device_call():
    from freeimpala_amd import _abi, vmpo
    from freeimpala_amd._abi import FiError
    prm, hp, W = vmpo.params(), _abi.VtraceHparams(), vmpo.SELECT_WS_BYTES
    ws = vmpo.workspace_bytes(5, 20, 3)
    loss = lambda **kw: vmpo.vmpo_loss_dev(**{**dict(T=5, B=20, A=3, pi=FAKE, act=FAKE, adv=FAKE, vs=FAKE, val=FAKE, hp=hp,  # noqa: E731
                                                     prm=prm, state=FAKE, dlogits=FAKE, dvalue=FAKE, losses=None, ws=FAKE,
                                                     ws_bytes=ws), **kw})
    for why, call in (("n = 0", lambda: vmpo.select_dev(0, FAKE, prm, FAKE, FAKE, W)),
                      ("n = 2147483648", lambda: vmpo.select_dev(2 ** 31, FAKE, prm, FAKE, FAKE, W)),
                      ("16-byte", lambda: vmpo.select_dev(100, FAKE + 4, prm, FAKE, FAKE, W)),
                      ("ws_bytes", lambda: vmpo.select_dev(100, FAKE, prm, FAKE, FAKE, W - 8)),
                      ("null", lambda: vmpo.select_dev(100, None, prm, FAKE, FAKE, W)),
                      ("null params", lambda: vmpo.select_dev(100, FAKE, None, FAKE, FAKE, W)),
                      ("A = 1", lambda: loss(A=1)), ("A = 65", lambda: loss(A=65)), ("T = 0", lambda: loss(T=0)),
                      ("16-byte", lambda: loss(pi=FAKE + 4)), ("ws_bytes", lambda: loss(ws_bytes=ws - 8)),
                      ("null", lambda: loss(state=None)), ("null state", lambda: vmpo.eta_step_dev(None, prm)),
                      ("4-byte", lambda: vmpo.eta_step_dev(FAKE, prm, skip=FAKE + 2))):
        with pytest.raises(FiError, match=r"rc=-1\b") as e:
            call()
        assert why.split(" = ")[0] in str(e.value), (why, str(e.value))


def case(T=6, B=9, A=5, seed=1):
    rs = np.random.RandomState(seed)
    return dict(pi=rs.standard_normal((T, B, A)).astype(np.float32), act=rs.randint(0, A, (T, B)).astype(np.int32),
                adv=rs.standard_normal((T, B)).astype(np.float32), vs=rs.standard_normal((T, B)).astype(np.float32),
                val=rs.standard_normal((T + 1, B)).astype(np.float32), hp=dict(baseline_cost=0.5, entropy_cost=0.0))


def test_a_huge_eta_over_the_whole_batch_is_plain_maximum_likelihood():
    """f = 1 and eta = 1e30: n psi is 1 on every row, so the policy gradient is that of -sum log pi(a): pi - onehot."""
    from freeimpala_amd import vmpo
    c = case()
    ref = vmpo.vmpo_reference(**c, eta=1e30, top_fraction=1.0)
    n = c["adv"].size
    assert ref["selected"] == n and np.abs(n * ref["psi"] - 1.0).max() <= 1e-12
    z = c["pi"].astype(np.float64)
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    onehot = np.eye(p.shape[-1])[c["act"]]
    assert np.abs(ref["dlogits"] - (p - onehot)).max() <= 1e-12


@pytest.mark.parametrize("f", [0.5, 1.0, 0.3, 0.01])
@pytest.mark.parametrize("kind", ["normal", "ties", "zeros"])
def test_select_reference_agrees_with_partition_on_the_keys(kind, f):
    from freeimpala_amd import vmpo
    rs = np.random.RandomState(7)
    a = rs.standard_normal(1001).astype(np.float32)
    if kind == "ties":
        a = np.round(a * 2) / 2
    if kind == "zeros":
        a[::3], a[1::3] = 0.0, -0.0
    s = vmpo.select_reference(a, f)
    ky, n = vmpo.keys(a), a.size
    assert s["key_tau"] == int(np.partition(ky, n - s["k"])[n - s["k"]]) and s["k"] == max(1, int(np.float32(f) * np.float64(n)))
    assert s["selected"] == int((a >= s["threshold"]).sum()) >= s["k"] and s["adv_max"] == a.max()
    assert (np.argsort(ky, kind="stable") == np.argsort(a + np.float32(0), kind="stable")).all(), "the keys keep the order"
