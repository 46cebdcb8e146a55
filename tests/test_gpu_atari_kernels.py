"""Every Atari kernel on its own against fp64, element by element, at the small shapes where each
path variant runs.

One resident step per case; then each kernel is recomputed in fp64 (tests/atari_ref.py) from the
tensors the step left behind -- the GPU's own stored inputs of that kernel -- so nothing separates
the stored output from the reference but the kernel's fp32 accumulation:

  * every bf16 and fp32 output, every element: the kernel accumulates a length-K reduction in fp32,
    so |acc32 - r| <= e = (K + c) u S with S the sum of the terms' absolute values, u = 2^-23 (which
    also covers a truncating adder) and c the epilogue's operations; rounding is monotone, so a
    stored bf16 output g satisfies rne_bf16(r - e) <= g <= rne_bf16(r + e) and an fp32 output
    |g - r| <= e. The bound is derived, not measured; no other tolerance is used.
  * every weight gradient in full at rel L2 1e-5 / scaled max 1e-4 (the bars of
    test_atari_full_size_gradient_vs_fp64), whole and per output channel.

The parameters (atari_ref.structured_params) keep the sums from cancelling, so an interval holds
one or two bf16 values for nearly every element (asserted: at most 5 % hold more than four); the
n21 and n128 production cases overwrite frame 0, frame N - 1 and both ends of every persistent
workgroup's walk with all-zero, all-255, single-impulse and sprite frames.

Recorded without asserting (FI_TEST_REPORT_DIR, and printed): per tensor the share of elements
with g != rne_bf16(r) and the largest distance in bf16 ulps."""
import numpy as np
import pytest

import atari_ref as R
from test_gpu_atari import _report, a1_planar_to_nhwc, mk

pytestmark = pytest.mark.gpu

# tensor -> (reduction length K, epilogue operations c): conv1 scales and adds its bias, the other
# forward layers add a bias, the data gradients only mask and round; dh sums the A + 1 outputs
KC = {"a1": (256, 2), "a2": (512, 1), "a3": (576, 1), "h": (3136, 1), "logits": (512, 1), "values": (512, 1),
      "da3": (512, 0), "da2": (576, 0), "da1": (256, 0)}


def _first(bad, shape):
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), shape))


def check_bf16(out, nm, bits, rS, K, c, relu=False):
    """Stored bf16 tensor (bit patterns) inside the interval of its reference, every element."""
    r, S = rS
    bits = np.asarray(bits, np.uint16).reshape(r.shape)
    lo_b, hi_b, wide = R.bf16_interval_stats(r, S, K, c, relu)
    g, lo, hi = R.bf16_bits_to_f64(bits), R.bf16_bits_to_f64(lo_b), R.bf16_bits_to_f64(hi_b)
    bad = ~((lo <= g) & (g <= hi))
    want = R.bf16_bits(np.maximum(r, 0) if relu else r)
    dist = np.abs(R.bf16_ord(bits) - R.bf16_ord(want))
    out["stats"][nm] = dict(share_not_rne=float((dist != 0).mean()), max_ulp=int(dist.max()), wide=wide)
    if wide > R.CAP:
        out["fails"].append(f"{nm}: {wide:.3f} of the intervals hold more than four bf16 values (inputs)")
    if bad.any():
        i = _first(bad, r.shape)
        out["fails"].append(f"{nm}: {int(bad.sum())} of {bad.size} outside the interval, first at (frame, ...) = {i}: "
                            f"g = {g[i]!r}, r = {r[i]!r}, e = {(K + c) * R.U32 * S[i]!r}")


def check_f32(out, nm, g, rS, K, c):
    r, S = rS
    g = np.asarray(g, np.float32).reshape(r.shape).astype(np.float64)
    _, _, e = R.interval(r, S, K, c)
    bad = ~(np.abs(g - r) <= e)
    wide = R.bf16_interval_stats(r, S, K, c)[2]
    r32 = r.astype(np.float32)
    ulp = np.abs(g - r32) / np.spacing(np.abs(r32)).astype(np.float64)
    out["stats"][nm] = dict(share_not_rne=float((g != r32).mean()), max_ulp_f32=float(ulp.max()), wide=wide)
    if wide > R.CAP:
        out["fails"].append(f"{nm}: {wide:.3f} of the intervals hold more than four bf16 values (inputs)")
    if bad.any():
        i = _first(bad, r.shape)
        out["fails"].append(f"{nm}: {int(bad.sum())} of {bad.size} outside the interval, first at (frame, ...) = {i}: "
                            f"g = {g[i]!r}, r = {r[i]!r}, e = {e[i]!r}")


def check_wgrad(out, nm, got, rS):
    """A weight gradient (k, co) against fp64 at rel L2 1e-5 / scaled max 1e-4, whole and for
    every output channel's slice on its own."""
    ref = rS[0]
    got = np.asarray(got, np.float64).reshape(ref.shape)
    d = got - ref
    if not np.isfinite(got).all():
        out["fails"].append(f"{nm}: not finite")
        return
    l2 = np.linalg.norm(d) / max(1e-30, np.linalg.norm(ref))
    mx = np.abs(d).max() / max(1e-30, np.abs(ref).max())
    cl2 = np.linalg.norm(d, axis=0) / np.maximum(1e-30, np.linalg.norm(ref, axis=0))
    cmx = np.abs(d).max(0) / np.maximum(1e-30, np.abs(ref).max(0))
    out["stats"][nm] = dict(rel_l2=float(l2), scaled_max=float(mx), worst_channel_rel_l2=float(cl2.max()),
                            worst_channel_scaled_max=float(cmx.max()))
    if l2 > 1e-5 or mx > 1e-4:
        k, co = _first(np.abs(d) == np.abs(d).max(), d.shape)
        out["fails"].append(f"{nm}: rel L2 {l2:.2e} scaled max {mx:.2e}, largest error at (k, co) = ({k}, {co}): "
                            f"g = {got[k, co]!r}, r = {ref[k, co]!r}")
    badc = (cl2 > 1e-5) | (cmx > 1e-4)
    if badc.any():
        co = int(np.argmax(badc))
        k = int(np.argmax(np.abs(d[:, co])))
        out["fails"].append(f"{nm}: {int(badc.sum())} output channels over the bars, first co = {co}: rel L2 "
                            f"{cl2[co]:.2e} scaled max {cmx[co]:.2e}, largest at k = {k}: g = {got[k, co]!r}, "
                            f"r = {ref[k, co]!r}")


@pytest.mark.parametrize("name,T,B,A,env,structured", R.CASES, ids=[c[0] for c in R.CASES])
def test_atari_kernels_elementwise_vs_fp64(name, T, B, A, env, structured, monkeypatch):
    """See the module docstring. Cases: 21 ragged frames on 4 persistent workgroups and 128 frames
    on 3 (42-43 frames each) on the production path with structured frames; 128 frames on 8 with
    the unfused forward and backward and a1 in NHWC; the generic implicit-GEMM path; A = 4; T = 1.
    On the production path da1 is never stored: it comes from a FI_KEEP_DA1 twin, whose a1 and da2
    must equal the learner's bit for bit."""
    for k in R.PATH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N, TB = (T + 1) * B, T * B
    production = not ({"FI_BWD_UNFUSED", "FI_ATARI_GENERIC"} & set(env))
    planar = production and "FI_A1_NHWC" not in env
    L = mk(T=T, B=B, A=A, seed=31)
    Ls = [L]
    if production:
        monkeypatch.setenv("FI_KEEP_DA1", "1")
        Ls.append(mk(T=T, B=B, A=A, seed=31))
        monkeypatch.delenv("FI_KEEP_DA1")
    L.synth(seed=R.case_seed(T, B, A))
    frames, what, p0 = R.case_inputs(L.tensor("frames", np.uint8, (N, 84, 84, 4)), T, B, A, env, structured)
    for X in Ls:
        X.synth(seed=R.case_seed(T, B, A))
        X.set_params(p0)
        if structured:
            X.upload("frames", frames)
    np.testing.assert_array_equal(L.get_params(), p0)
    for X in Ls:
        X.step_resident()
    np.testing.assert_array_equal(L.tensor("frames", np.uint8, (N, 84, 84, 4)), frames)

    def bits(X, nm, sh):
        a = X.tensor(nm, np.uint16, (N, int(np.prod(sh))))
        return (a1_planar_to_nhwc(a) if nm == "a1" and planar else a).reshape((N,) + sh)

    b = {nm: bits(L, nm, sh) for nm, sh in [("a1", (20, 20, 32)), ("a2", (9, 9, 64)), ("a3", (7, 7, 64)), ("h", (512,)),
                                            ("dh", (512,)), ("da3", (7, 7, 64)), ("da2", (9, 9, 64))]}
    src = Ls[-1]
    b["da1"] = src.tensor("da1", np.uint16, (N, 20, 20, 32))
    if production:  # the twin's da1 belongs to the same a1 and da2
        np.testing.assert_array_equal(src.tensor("a1", np.uint16, (N, 12800)), L.tensor("a1", np.uint16, (N, 12800)))
        np.testing.assert_array_equal(bits(src, "da2", (9, 9, 64)), b["da2"])
        np.testing.assert_array_equal(src.tensor("grads"), L.tensor("grads"))
    v = {nm: R.bf16_bits_to_f64(x) for nm, x in b.items()}
    logits = L.tensor("logits", shape=(N, A))
    values = L.tensor("values", shape=(N,))
    dout = np.zeros((N, A + 1))
    dout[:TB, :A] = L.tensor("dlogits", shape=(TB, A))
    dout[:, A] = L.tensor("dvalue", shape=(N,))
    grads = R.split_grads(L.tensor("grads"), A)
    for X in Ls:
        X.close()

    P = R.unpack_params(p0, A)
    out = dict(fails=[], stats={})
    # forward: each layer from the stored output of the layer before it
    check_bf16(out, "a1", b["a1"], R.conv1_fwd(frames, P["c1W"], P["c1b"], relu=False), *KC["a1"], relu=True)
    check_bf16(out, "a2", b["a2"], R.conv2_fwd(v["a1"], P["c2W"], P["c2b"], relu=False), *KC["a2"], relu=True)
    check_bf16(out, "a3", b["a3"], R.conv3_fwd(v["a2"], P["c3W"], P["c3b"], relu=False), *KC["a3"], relu=True)
    check_bf16(out, "h", b["h"], R.fc_fwd(v["a3"].reshape(N, 3136), P["fcW"], P["fcb"], relu=False), *KC["h"],
               relu=True)
    r, S = R.heads_fwd(v["h"], P["hW"], P["hb"])
    check_f32(out, "logits", logits, (r[:, :A], S[:, :A]), *KC["logits"])
    check_f32(out, "values", values, (r[:, A], S[:, A]), *KC["values"])
    # data gradients (rows T B .. belong to the bootstrap frames: exact zeros on both sides)
    check_bf16(out, "dh", b["dh"], R.heads_dgrad(dout, P["hW32"], v["h"]), A + 1, 0)
    # (the generic path masks the stored da3 in place, relu_mask_bf16, before conv3's GEMMs read it)
    m3 = (v["a3"] > 0) if "FI_ATARI_GENERIC" in env else 1.0
    check_bf16(out, "da3", b["da3"], [x.reshape(N, 7, 7, 64) * m3 for x in R.fc_dgrad(v["dh"], P["fcW"])], *KC["da3"])
    check_bf16(out, "da2", b["da2"], R.conv3_dgrad(v["da3"], v["a3"], P["c3W"], v["a2"]), *KC["da2"])
    check_bf16(out, "da1", b["da1"], R.conv2_dgrad(v["da2"], P["c2W"], v["a1"]), *KC["da1"])
    # weight gradients, every channel and tap
    c1w = R.conv1_wgrad(frames, v["da1"])
    check_wgrad(out, "c1W", grads["c1W"], c1w)
    check_wgrad(out, "c2W", grads["c2W"], R.conv2_wgrad(v["a1"], v["da2"]))
    check_wgrad(out, "c3W", grads["c3W"], R.conv3_wgrad(v["a2"], v["da3"], v["a3"]))
    check_wgrad(out, "fcW", grads["fcW"], R.fc_wgrad(v["a3"].reshape(N, 3136), v["dh"]))
    check_wgrad(out, "hW", grads["hW"], R.heads_wgrad(v["h"], dout))
    if structured:
        zero = [f for f, w in what.items() if w == "zero"]
        assert zero and 0 in zero and (N - 1) in what and len(set(what.values()) - {"zero"}) == len(what) - len(zero)
        # a1 of an all-zero frame is bf16(max(b1, 0)) at all 400 positions, bit for bit
        want = R.bf16_bits(np.maximum(P["c1b"], 0))
        for f in zero:
            if not (b["a1"][f] == want).all():
                y, x, c = _first(b["a1"][f] != want, (20, 20, 32))
                out["fails"].append(f"a1 of the all-zero frame {f} is not bf16(max(b1, 0)) at (y, x, c) = ({y}, {x}, {c}): "
                                    f"g = {v['a1'][f, y, x, c]!r}, b1 = {P['c1b'][c]!r}")
        # an all-zero frame adds nothing to the c1W gradient: the reference over the other frames
        # is the same reference (a consistency check of the reference's frame slices)
        keep = np.array([f for f in range(N) if f not in zero])
        np.testing.assert_array_equal(R.conv1_wgrad(frames[keep], v["da1"][keep])[0], c1w[0])
    out["stats"]["frames"] = {str(f): w for f, w in what.items()}
    _report("atari_kernels_" + name, out)
    print(f"\n{name}:")
    for nm, s in out["stats"].items():
        print(f"  {nm}: {s}")
    assert not out["fails"], "\n".join(out["fails"])
