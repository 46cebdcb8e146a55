"""Per-kernel fp64 references of the Atari step, in numpy -- TEST INFRASTRUCTURE.

Every function computes ONE kernel from that kernel's own inputs as the kernel reads them (uint8
frames; stored bf16 tensors widened exactly to fp64; weight images as bf16_round(p0[...]); biases
and the heads' Wh in fp32 where the kernel reads fp32) and returns

    r -- the fp64 result before the output rounding, with the kernel's rounding points and
         nothing else (conv1: relu(conv(frames) * fl32(1/255) + b));
    S -- the fp64 sum of the absolute values of the same terms, |bias| included, computed by the
         same routine on |x| and |w|.

What separates a kernel's stored output from r is then fp32 accumulation alone:
|acc32 - r| <= (K + c) u S for a length-K fp32 reduction with c epilogue operations (interval()).
The forward references take relu=False to return r before the ReLU: the interval test needs the
pre-activation (relu is monotone and 1-Lipschitz, so the interval's ends are relu(r -+ e); from
relu(r) alone an element with r < 0 would get the vacuous interval [-e, e]).

Convolutions are im2col + fp64 matmul, chunked over frames. Weight matrices are the parameter
blob's own layout: conv [ky][kx][ci][co] flattened to (k, co), fc (3136, 512), heads (512, A+1).
"""
import numpy as np

INV255 = np.float64(np.float32(1.0) / np.float32(255.0))  # the fp32 constant the kernels multiply by
U32 = 2.0 ** -23  # fp32 unit roundoff of the accumulation, covering a truncating adder
CHUNK = 32        # frames per im2col chunk

SIZES = lambda A: [8192, 32, 32768, 64, 36864, 64, 3136 * 512, 512, 512 * (A + 1), A + 1]
NAMES = ["c1W", "c1b", "c2W", "c2b", "c3W", "c3b", "fcW", "fcb", "hW", "hb"]


# ------------------------------------------------------------------ number formats
def bf16_bits_to_f64(u16):
    """stored bf16 (uint16 bit patterns) -> float64, exactly."""
    return (np.asarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_bits(x):
    """float64 -> bf16 bit patterns by round-to-nearest-even of the fp32 value of x (the kernels
    round an fp32 accumulator; fp64 -> fp32 -> bf16 is monotone, and for an fp32 accumulator
    acc <= x it gives bf16(acc) <= bf16(fl32(x)), so it is the right end of an interval)."""
    u = np.ascontiguousarray(x, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def rne_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64."""
    return bf16_bits_to_f64(bf16_bits(x))


def bf16_ord(bits):
    """bf16 bit patterns -> integers in the order of the values (-0 and +0 both 0): the
    difference of two is their distance in representable bf16 values."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    return np.where(b < 0x8000, b, 0x8000 - b)


def unpack_params(p0, A):
    """fp32 parameter blob -> dict of fp64 arrays as the kernels read them: cNW / fcW / hW are the
    bf16 weight images (RNE of the fp32 master weights), hW32 the fp32 heads weights the heads'
    backward reads, biases fp32."""
    p0 = np.asarray(p0, np.float32)
    off = np.cumsum([0] + SIZES(A))
    raw = {nm: p0[off[i]:off[i + 1]] for i, nm in enumerate(NAMES)}
    out = {nm: raw[nm].astype(np.float64) for nm in NAMES if nm.endswith("b")}
    for nm, sh in [("c1W", (256, 32)), ("c2W", (512, 64)), ("c3W", (576, 64)), ("fcW", (3136, 512)),
                   ("hW", (512, A + 1))]:
        out[nm] = rne_bf16(raw[nm].astype(np.float64)).reshape(sh)
    out["hW32"] = raw["hW"].astype(np.float64).reshape(512, A + 1)
    return out


def split_grads(g, A):
    off = np.cumsum([0] + SIZES(A))
    return {nm: np.asarray(g[off[i]:off[i + 1]]) for i, nm in enumerate(NAMES)}


# ------------------------------------------------------------------ im2col
def _im2col(x, K, S):
    """(n, H, H, C) -> (n * OH * OH, K * K * C), k = (ky, kx, c) as in the weight blob."""
    n, H, _, C = x.shape
    OH = (H - K) // S + 1
    w = np.lib.stride_tricks.sliding_window_view(x, (K, K), axis=(1, 2))[:, ::S, ::S]  # n,OH,OH,C,K,K
    return np.ascontiguousarray(w.transpose(0, 1, 2, 4, 5, 3)).reshape(n * OH * OH, K * K * C)


def _conv(x, w, K, S):
    n, H = x.shape[0], x.shape[1]
    OH = (H - K) // S + 1
    out = np.empty((n, OH, OH, w.shape[1]))
    for i in range(0, n, CHUNK):
        xs = x[i:i + CHUNK]
        out[i:i + CHUNK] = (_im2col(xs, K, S) @ w).reshape(xs.shape[0], OH, OH, -1)
    return out


def _conv_wgrad(x, dy, K, S):
    """sum over frames and output pixels of im2col(x)^T dy -> (K * K * C, OC)."""
    out = np.zeros((K * K * x.shape[3], dy.shape[3]))
    for i in range(0, x.shape[0], CHUNK):
        out += _im2col(x[i:i + CHUNK], K, S).T @ dy[i:i + CHUNK].reshape(-1, dy.shape[3])
    return out


def _conv_dgrad(dy, w, K, S, IH, C):
    """dx[n][oy S + ky][ox S + kx][c] += sum_o dy[n][oy][ox][o] w[(ky, kx, c)][o]."""
    n, OH, _, OC = dy.shape
    cols = (dy.reshape(-1, OC) @ w.T).reshape(n, OH, OH, K, K, C)
    dx = np.zeros((n, IH, IH, C))
    for ky in range(K):
        for kx in range(K):
            dx[:, ky:ky + S * OH:S, kx:kx + S * OH:S] += cols[:, :, :, ky, kx]
    return dx


def _act(r, relu):
    return np.maximum(r, 0.0) if relu else r


# ------------------------------------------------------------------ forward
def conv1_fwd(frames, w, b, relu=True):
    """a1 before its bf16 rounding: relu(conv8x8/4(frames) * fl32(1/255) + b1). Mirrors
    atari_fr.hip conv1_fwd_fr / conv12_fwd_fr's conv1 epilogue `fmaxf(d * inv255 + bch, 0.f)`
    and atari.hip EpiAct with scale 1/255 (generic path). K = 256, c = 2 (scale, bias add)."""
    x = np.asarray(frames, np.uint8).astype(np.float64)
    return (_act(_conv(x, w, 8, 4) * INV255 + b, relu),
            _conv(x, np.abs(w), 8, 4) * INV255 + np.abs(b))


def conv2_fwd(a1, w, b, relu=True):
    """a2 before rounding: relu(conv4x4/2(a1) + b2), a1 (N, 20, 20, 32) NHWC as stored. Mirrors
    atari_fr.hip conv_fwd_fr<2> / conv12_fwd_fr's conv2 epilogue `fmaxf(acc + bch, 0.f)` and
    atari.hip EpiAct (scale 1). K = 512, c = 1 (bias add)."""
    return _act(_conv(a1, w, 4, 2) + b, relu), _conv(np.abs(a1), np.abs(w), 4, 2) + np.abs(b)


def conv3_fwd(a2, w, b, relu=True):
    """a3 before rounding: relu(conv3x3/1(a2) + b3). Mirrors atari_fr.hip conv_fwd_fr<3>'s
    epilogue `fmaxf(acc + bch, 0.f)` and atari.hip EpiAct. K = 576, c = 1."""
    return _act(_conv(a2, w, 3, 1) + b, relu), _conv(np.abs(a2), np.abs(w), 3, 1) + np.abs(b)


def fc_fwd(a3, w, b, relu=True):
    """h before rounding: relu(a3 . fcW + b), a3 (N, 3136). Mirrors fc_gemm.hip fc_nt_kernel with
    the forward's bias + ReLU epilogue (header: `h = relu(a3 . fcW + b)`). K = 3136, c = 1."""
    return _act(a3 @ w + b, relu), np.abs(a3) @ np.abs(w) + np.abs(b)


def heads_fwd(h, w, b):
    """[logits | value] in fp32: h . bf16(Wh) + bh. Mirrors atari.hip bf16_gemm<128, 32, 4, 1> over
    the bf16 image hT with EpiHeadsOut (`v += bias[n]`). K = 512, c = 1."""
    return h @ w + b, np.abs(h) @ np.abs(w) + np.abs(b)


# ------------------------------------------------------------------ data gradients
def heads_dgrad(dout, w32, h):
    """dh before rounding: (h > 0) * dout . Wh^T with dout = [dlogits | dvalue] and Wh in fp32.
    Mirrors atari.hip heads_dgrad_valu (an fmaf chain over the A + 1 outputs, then
    `hv > 0 ? acc : 0`). K = A + 1, c = 0."""
    m = h > 0
    return (dout @ w32.T) * m, (np.abs(dout) @ np.abs(w32).T) * m


def fc_dgrad(dh, w):
    """da3 before rounding, stored unmasked: dh . fcW^T. Mirrors fc_gemm.hip fc_dgrad_wreg_kernel
    (and fc_nt_kernel's dgrad), whose epilogue only rounds. K = 512, c = 0."""
    return dh @ w.T, np.abs(dh) @ np.abs(w).T


def conv3_dgrad(da3, a3, w, a2):
    """da2 before rounding: (a2 > 0) * dgrad3x3/1((a3 > 0) * da3, W3): the a3 mask is applied to the
    stored, unmasked da3 as it is loaded, the a2 mask in the epilogue. Mirrors atari_fr.hip
    conv3_bwd_fr (`mv > 0 ? v : 0` on load, `m > 0 ? acc : 0` on store) and atari.hip
    relu_mask_bf16 + DgradGather<9, 3, 1, 7, 64> + EpiDgrad (generic). K = 576, c = 0."""
    d = da3 * (a3 > 0)
    m = a2 > 0
    return _conv_dgrad(d, w, 3, 1, 9, 64) * m, _conv_dgrad(np.abs(d), np.abs(w), 3, 1, 9, 64) * m


def conv2_dgrad(da2, w, a1):
    """da1 before rounding: (a1 > 0) * dgrad4x4/2(da2, W2), da2 as stored (already masked by a2).
    Mirrors atari_fr.hip conv2_bwd_fr / conv21_bwd_fr (`m > 0 ? acc : 0`) and atari.hip
    DgradGather<20, 4, 2, 9, 64> + EpiDgrad: a parity class's pixel sums 2 x 2 taps of 64
    channels. K = 256, c = 0."""
    m = a1 > 0
    return _conv_dgrad(da2, w, 4, 2, 20, 32) * m, _conv_dgrad(np.abs(da2), np.abs(w), 4, 2, 20, 32) * m


# ------------------------------------------------------------------ weight gradients
def conv1_wgrad(frames, da1):
    """c1W gradient (256, 32): fl32(1/255) * sum im2col(frames)^T da1. Mirrors atari_fr.hip
    conv1_wgrad_fr / conv21_bwd_fr's conv1 slabs (`v * inv255`) and atari.hip bf16_wgrad with
    scale 1/255."""
    x = np.asarray(frames, np.uint8).astype(np.float64)
    return _conv_wgrad(x, da1, 8, 4) * INV255, _conv_wgrad(x, np.abs(da1), 8, 4) * INV255


def conv2_wgrad(a1, da2):
    """c2W gradient (512, 64): sum im2col(a1)^T da2 (atari_fr.hip conv2_bwd_fr / conv21_bwd_fr,
    atari.hip bf16_wgrad)."""
    return _conv_wgrad(a1, da2, 4, 2), _conv_wgrad(np.abs(a1), np.abs(da2), 4, 2)


def conv3_wgrad(a2, da3, a3):
    """c3W gradient (576, 64): sum im2col(a2)^T ((a3 > 0) * da3) (atari_fr.hip conv3_bwd_fr,
    atari.hip relu_mask_bf16 + bf16_wgrad)."""
    d = da3 * (a3 > 0)
    return _conv_wgrad(a2, d, 3, 1), _conv_wgrad(np.abs(a2), np.abs(d), 3, 1)


def fc_wgrad(a3, dh):
    """fcW gradient (3136, 512): a3^T dh (fc_gemm.hip fc_tn_kernel)."""
    return a3.T @ dh, np.abs(a3).T @ np.abs(dh)


def heads_wgrad(h, dout):
    """hW gradient (512, A + 1): h^T [dlogits | dvalue] in fp32 (atari.hip heads_wgrad_valu)."""
    return h.T @ dout, np.abs(h).T @ np.abs(dout)


# ------------------------------------------------------------------ the interval
def interval(r, S, K, c, relu=False):
    """(lo, hi, e): e = (K + c) u S bounds |acc32 - r| for a length-K fp32 reduction and c epilogue
    operations; the epilogue's ReLU is monotone and 1-Lipschitz, so it is applied to both ends."""
    e = (K + c) * U32 * S
    return _act(r - e, relu), _act(r + e, relu), e


def bf16_interval_stats(r, S, K, c, relu=False):
    """Input-only figures of a tensor's interval test (they depend on r, S and K alone): the bf16
    bit patterns of the interval's ends and the share of elements whose interval holds more than
    four representable bf16 values."""
    lo, hi, _ = interval(r, S, K, c, relu)
    lo_b, hi_b = bf16_bits(lo), bf16_bits(hi)
    wide = (bf16_ord(hi_b) - bf16_ord(lo_b) + 1) > 4
    return lo_b, hi_b, float(wide.mean())


# ------------------------------------------------------------------ inputs of the kernel tests
# (id, T, B, A, environment of the path, structured frames): the cases of
# tests/test_gpu_atari_kernels.py; tests/test_atari_ref.py checks their inputs on the CPU
_UNFUSED = {"FI_FR_GRID": "8", "FI_FWD_UNFUSED": "1", "FI_BWD_UNFUSED": "1", "FI_A1_NHWC": "1"}
CASES = [("n21_grid4", 2, 7, 18, {"FI_FR_GRID": "4"}, True),
         ("n128_grid3", 3, 32, 18, {"FI_FR_GRID": "3"}, True),
         ("n128_grid8_unfused_nhwc", 3, 32, 18, _UNFUSED, False),
         ("n48_generic", 2, 16, 18, {"FI_ATARI_GENERIC": "1"}, False),
         ("n48_grid5_a4", 2, 16, 4, {"FI_FR_GRID": "5"}, False),
         ("n18_t1", 1, 9, 18, {}, False)]
PATH_ENV = ("FI_FR_GRID", "FI_FWD_UNFUSED", "FI_BWD_UNFUSED", "FI_A1_NHWC", "FI_ATARI_GENERIC", "FI_KEEP_DA1",
            "FI_FC_DGRAD_RING")
CAP = 0.05  # share of a tensor's elements whose interval may hold more than four bf16 values


def case_seed(T, B, A):
    return 7000 + 100 * T + B + A


def case_inputs(synth_frames, T, B, A, env, structured):
    """(frames (N, 84, 84, 4), {frame: pattern}, parameters) of a case from its synthetic frames."""
    seed = case_seed(T, B, A)
    frames, what = np.asarray(synth_frames, np.uint8).reshape(-1, 84, 84, 4), {}
    if structured:
        frames, what = structured_frames(frames, T * B, int(env.get("FI_FR_GRID", 256)), seed)
    return frames, what, structured_params(A, seed)


def structured_params(A, seed):
    """Parameters for the per-kernel interval tests. With the Glorot initialisation (weights of
    both signs, zero biases) every output is a sum of up to 3,136 cancelling terms, |r| << S, and
    the derived interval (K + c) u S spans many bf16 values of r: for a third of h's elements the
    test would be vacuous (the figures are in tests/test_atari_ref.py). Here every output
    channel's weights share one sign and their magnitudes vary by +-50 % around a per-layer scale
    that keeps the activations O(1); the activations are >= 0, so a pre-activation is a sum of
    same-sign terms plus a bias of the opposite sign, and a frame's data gradients mostly keep one
    sign through the backward. Of every 8 output channels 5 are positive with a small negative
    bias (on), 1 is negative without a bias (off: exact zeros downstream), and 2 switch from
    pixel to pixel and frame to frame: one negative with a positive bias, one positive with a
    negative bias, the bias near the channel's mean |sum| over two calibration frames of noise."""
    rs = np.random.RandomState(seed)
    parts = []
    x = rs.randint(0, 256, (2, 84, 84, 4)).astype(np.float64) * INV255

    def layer(x, O, conv, spread):
        K = x.shape[-1] if conv is None else conv[0] * conv[0] * x.shape[-1]
        mag = (0.5 + rs.random_sample((K, O))) / (K * x.mean())
        a = x @ mag if conv is None else _conv(x, mag, *conv)
        M = a.reshape(-1, O).mean(0)
        kind = np.arange(O) % 8  # 0-4 on, 5 negative + bias, 6 positive - bias, 7 off
        rs.shuffle(kind)
        sign = np.where((kind < 5) | (kind == 6), 1.0, -1.0)
        f = M * (1.0 + spread * (2.0 * rs.random_sample(O) - 1.0))
        bias = np.where(kind < 5, -0.05, np.where(kind == 5, f, np.where(kind == 6, -f, 0.0)))
        parts.extend([(mag * sign).ravel(), bias])
        return np.maximum(a * sign + bias, 0.0)

    x = layer(x, 32, (8, 4), 0.15)
    x = layer(x, 64, (4, 2), 0.15)
    x = layer(x, 64, (3, 1), 0.15)
    x = layer(x.reshape(2, 3136), 512, None, 0.7)
    # heads: logits / value of both signs (no ReLU behind them), magnitudes within +-10 % per output
    # so that a row's dh keeps one sign over the hidden units
    mag = (0.9 + 0.2 * rs.random_sample((512, A + 1))) / (512 * x.mean()) * (0.3 + 1.5 * rs.random_sample(A + 1))
    sign = np.where(rs.random_sample(A + 1) < 0.5, 1.0, -1.0)
    parts.extend([(mag * sign).ravel(), 0.1 * rs.standard_normal(A + 1)])
    return np.concatenate(parts).astype(np.float32)


def walk_ends(n_fwd, n_bwd, grid):
    """First and last frame of every persistent workgroup's walk: workgroup b of G = min(N, grid)
    walks frames b, b + G, b + 2G, ... (atari_fr.hip: `f = blockIdx.x + it * gridDim.x`), over all
    N frames in the forward and over the first T * B in the backward."""
    G = min(n_fwd, grid)
    out = {0, n_fwd - 1}
    for n in (n_fwd, n_bwd):
        for b in range(min(G, n)):
            out.update((b, b + (n - 1 - b) // G * G))
    return sorted(out)


IMPULSES = [(0, 0), (83, 83), (3, 4), (4, 3), (79, 80)]


def structured_frames(frames, n_bwd, grid, seed):
    """Overwrite frame 0, frame N - 1 and the ends of every workgroup's walk with frames that look
    like Atari: all zero, all 255, a single byte 255 at one of IMPULSES (one per frame and channel,
    another (position, channel) in every frame), and one frame constant 87 outside a 6 x 6 sprite of
    random bytes. Returns (frames, {frame: pattern})."""
    fr = np.array(frames, np.uint8).reshape(-1, 84, 84, 4)
    rs = np.random.RandomState(seed)
    what = {}
    idx = walk_ends(fr.shape[0], n_bwd, grid)
    for j, f in enumerate(idx):
        if j == 0:
            fr[f] = 0
            what[f] = "zero"
        elif j == 1:
            fr[f] = 255
            what[f] = "full"
        elif j == 2:
            fr[f] = 87
            y, x = rs.randint(0, 79, 2)
            fr[f, y:y + 6, x:x + 6] = rs.randint(0, 256, (6, 6, 4))
            what[f] = "sprite"
        elif j % 7 == 3:
            fr[f] = 0
            what[f] = "zero"
        else:
            k = j - 3
            (y, x), c = IMPULSES[k % 5], (k // 5) % 4
            fr[f] = 0
            fr[f, y, x, c] = 255
            what[f] = f"impulse({y},{x},{c})"
    return fr, what
