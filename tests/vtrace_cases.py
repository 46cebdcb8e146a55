"""Shared pieces of the V-trace tests: a plain helper module, not a conftest.

* case builders: one named input regime each, ``build(name, seed, T, B, A)`` ->
  ``(pi, mu, act, rew, disc, val, hp)``;
* ``ref_numpy``: SURVEY.md 8(a) / the header comment of csrc/vtrace.hip in float64 numpy. It shares
  no code with oracle/ (tests/test_vtrace_reference.py proves the two against each other before
  either judges a kernel);
* ``run_vtrace`` / ``compare``: launch one kernel variant through the C ABI and hold its five outputs
  against a reference at the project's bar; ``guard=True`` puts 4 KiB of a sentinel on both sides of
  every output tensor and requires every sentinel word to survive;
* the case lists of tests/test_gpu_vtrace_matrix.py, so that the CPU reference test walks exactly
  the cases the GPU matrix walks.
"""
import ctypes as C

import numpy as np

HP_KEYS = ["rho_bar", "c_bar", "pg_rho_bar", "lambda_", "baseline_cost", "entropy_cost"]
HP_DEFAULT = dict(rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, lambda_=1.0, baseline_cost=0.5,
                  entropy_cost=0.01)
TOL = 1e-5
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
EVEN_A = tuple(range(2, 21, 2))  # the instantiations of the three fast kernels
CUS_MI355X = 256                 # the CPU reference test walks section d's shapes at this count


def f32hp(**hp):
    """Hyper-parameters rounded to fp32 (what the kernels' struct holds), so that the fp64
    references and the kernels are given the same numbers."""
    h = dict(HP_DEFAULT)
    h.update(hp)
    return {k: float(np.float32(v)) for k, v in h.items()}


# ------------------------------------------------------------------------------------------
# the fp64 reference
# ------------------------------------------------------------------------------------------
def _log_softmax(z):
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def ref_numpy(pi, mu, act, rew, disc, val, **hp):
    """V-trace targets, the three IMPALA loss sums and their analytic gradients, float64.
    log_rho = log pi(a) - log mu(a); rho = min(rho_bar, e^log_rho); c = lambda min(c_bar, e^log_rho)
    acc_t = rho_t (r_t + g_t V_{t+1} - V_t) + g_t c_t acc_{t+1}, acc_T = 0; vs_t = V_t + acc_t
    pg_adv_t = min(pg_rho_bar, e^log_rho) (r_t + g_t vs_{t+1} - V_t), vs_T = V_T
    losses = [sum -pg_adv log pi(a), sum acc^2 / 2, sum_t,b sum_i pi_i log pi_i]
    dlogits = -pg_adv (onehot - pi) + ec pi (log pi - sum pi log pi); dvalue_t = bc (V_t - vs_t)."""
    h = dict(HP_DEFAULT)
    h.update(hp)
    pi, mu, rew, disc, val = (np.asarray(x, np.float64) for x in (pi, mu, rew, disc, val))
    act = np.asarray(act, np.int64)
    T, B, A = pi.shape
    assert ((act >= 0) & (act < A)).all()
    lp = _log_softmax(pi)
    lm = _log_softmax(mu)
    idx = act[..., None]
    lpa = np.take_along_axis(lp, idx, -1)[..., 0]
    log_rho = lpa - np.take_along_axis(lm, idx, -1)[..., 0]
    with np.errstate(over="ignore", under="ignore"):
        ratio = np.exp(log_rho)
    rho = np.minimum(h["rho_bar"], ratio)
    c = h["lambda_"] * np.minimum(h["c_bar"], ratio)
    pg_rho = np.minimum(h["pg_rho_bar"], ratio)
    acc = np.zeros((T + 1, B))
    for t in range(T - 1, -1, -1):
        acc[t] = rho[t] * (rew[t] + disc[t] * val[t + 1] - val[t]) + disc[t] * c[t] * acc[t + 1]
    vs = val + acc                                  # row T is the bootstrap: vs_T = V_T
    adv = pg_rho * (rew + disc * vs[1:] - val[:T])
    p = np.exp(lp)
    plogp = (p * lp).sum(-1)
    onehot = np.arange(A) == idx
    dlogits = -adv[..., None] * (onehot - p) + h["entropy_cost"] * p * (lp - plogp[..., None])
    dvalue = np.zeros((T + 1, B))
    dvalue[:T] = h["baseline_cost"] * (val[:T] - vs[:T])
    losses = np.array([(-adv * lpa).sum(), 0.5 * (acc[:T] ** 2).sum(), plogp.sum()])
    return dict(vs=vs[:T], pg_adv=adv, dlogits=dlogits, dvalue=dvalue, losses=losses,
                log_rho=log_rho)


COND_MAX = 10.0


def condition_numbers(pi, mu, act, rew, disc, val, **hp):
    """How much larger the terms of each output are than the bar's own measure max(1, |output|).
    The kernels' arithmetic is fp32 with hardware exp2 / log2: a term such as rho (r + g V' - V)
    carries about a dozen roundings and two 1-ulp transcendentals whose argument errors are
    amplified by the exponent's size, together up to u = 2^-20 (about 1e-6) relative to the term.
    (The bracket itself adds exact fp32 inputs: it carries a rounding, 2^-23 = u / 8 of the inputs'
    magnitudes, hence the second summand of acc_mag and adv_mag.)
    A sum of terms then carries up to u * sum |term|, and the project's bar 1e-5 * max(1, |sum|)
    can only judge the kernel where sum |term| <= 10 * max(1, |sum|): where a sum cancels further,
    the bar measures the cancellation of the inputs, not the kernel. The matrix's unit-scale cases
    are built so that this holds (COND_MAX), and tests/test_vtrace_reference.py asserts it.
    Kept apart from ref_numpy: this recomputes the weights and runs the recurrence on magnitudes."""
    h = dict(HP_DEFAULT)
    h.update(hp)
    ref = ref_numpy(pi, mu, act, rew, disc, val, **hp)
    pi, rew, disc, val = (np.asarray(x, np.float64) for x in (pi, rew, disc, val))
    T, B, A = pi.shape
    with np.errstate(over="ignore", under="ignore"):
        ratio = np.exp(ref["log_rho"])
    rho, c = np.minimum(h["rho_bar"], ratio), h["lambda_"] * np.minimum(h["c_bar"], ratio)
    pg_rho = np.minimum(h["pg_rho_bar"], ratio)
    lp = _log_softmax(pi)
    idx = np.asarray(act, np.int64)[..., None]
    lpa, p, onehot = np.take_along_axis(lp, idx, -1)[..., 0], np.exp(lp), np.arange(A) == idx
    inputs = (np.abs(rew) + disc * np.abs(val[1:]) + np.abs(val[:T])) / 8
    mag = np.zeros((T + 1, B))
    for t in range(T - 1, -1, -1):
        mag[t] = (rho[t] * (np.abs(rew[t] + disc[t] * val[t + 1] - val[t]) + inputs[t])
                  + disc[t] * c[t] * mag[t + 1])
    adv_mag = pg_rho * (np.abs(rew + disc * val[1:] - val[:T]) + disc * mag[1:] + inputs)
    acc = ref["vs"] - val[:T]
    one = lambda x: np.maximum(1.0, np.abs(x))  # noqa: E731
    return dict(vs=float((mag[:T] / one(ref["vs"])).max()),
                pg_adv=float((adv_mag / one(ref["pg_adv"])).max()),
                dlogits=float((adv_mag[..., None] * np.abs(onehot - p) / one(ref["dlogits"])).max()),
                pg_loss=float((adv_mag * np.abs(lpa)).sum() / one(ref["losses"][0])),
                baseline_loss=float((np.abs(acc) * mag[:T]).sum() / one(ref["losses"][1])))


# ------------------------------------------------------------------------------------------
# case builders
# ------------------------------------------------------------------------------------------
def rand_case(seed, T, B, A, scale=1.0, done_p=0.02, gamma=0.99):
    rs = np.random.RandomState(seed)
    pi = (rs.randn(T, B, A) * scale).astype(np.float32)
    mu = (rs.randn(T, B, A) * scale).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.choice([-1.0, 0.0, 1.0], (T, B)).astype(np.float32)
    disc = np.where(rs.rand(T, B) < done_p, 0.0, gamma).astype(np.float32)
    val = rs.randn(T + 1, B).astype(np.float32)
    return pi, mu, act, rew, disc, val


def unit_case(seed, T, B, A, scale=1.0, done_p=0.02, gamma=0.99):
    """rand_case with rewards in {1, 1, 2} and values 0.2 * randn: every delta_t has the same sign,
    so acc, pg_adv and the loss sums add up instead of cancelling and the project's bar, relative
    to max(1, |output|), judges the kernel (condition_numbers). Logits, actions, discounts and
    episode ends are rand_case's."""
    rs = np.random.RandomState(seed)
    pi = (rs.randn(T, B, A) * scale).astype(np.float32)
    mu = (rs.randn(T, B, A) * scale).astype(np.float32)
    act = rs.randint(0, A, (T, B)).astype(np.int32)
    rew = rs.choice([1.0, 1.0, 2.0], (T, B)).astype(np.float32)
    disc = np.where(rs.rand(T, B) < done_p, 0.0, gamma).astype(np.float32)
    val = (0.2 * rs.randn(T + 1, B)).astype(np.float32)
    return pi, mu, act, rew, disc, val


BUILDERS = {}


def builder(name):
    def reg(fn):
        BUILDERS[name] = fn
        return fn
    return reg


def build(name, seed, T, B, A):
    """Builder `name` at shape (T, B, A): (pi, mu, act, rew, disc, val, hp)."""
    out = BUILDERS[name](seed, T, B, A)
    assert len(out) == 7
    return out


@builder("base")
def _base(seed, T, B, A):
    """The shape sections' inputs. The three bars and lambda are pairwise distinct and each bar binds
    on part of the rows, so an instantiation that reads one where another belongs shows at once."""
    return unit_case(seed, T, B, A) + (f32hp(rho_bar=1.0, c_bar=0.75, pg_rho_bar=1.5, lambda_=0.9),)


@builder("mixed_sign")
def _mixed(seed, T, B, A):
    """unit_case with rewards in {-1, 1}: deltas, acc and pg_adv take both signs. A row's own
    bracket does not cancel (|r| = 1 against values of 0.2), so the tensors stay well conditioned;
    the loss sums over rows of both signs cancel (condition_numbers), so the tensors alone are
    compared."""
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    rew = np.random.RandomState(seed + 1).choice([-1.0, 1.0], (T, B)).astype(np.float32)
    return pi, mu, act, rew, disc, val, f32hp(rho_bar=1.0, c_bar=0.75, pg_rho_bar=1.5, lambda_=0.9)


# ---- section e: hyper-parameter branches. The clip under test sits at 1.0 (it binds where
# pi(a) > mu(a): about half the rows of independent randn logits) or at 1e9 (never binds); the other
# two sit at 0.5 and 2.0, so the three bars are pairwise distinct and exchanging any two shows.
CLIPS = ("rho_bar", "c_bar", "pg_rho_bar")
HALF, NEVER, OTHERS = 1.0, 1e9, (0.5, 2.0)


def _clip_hp(which, value):
    rest = [k for k in CLIPS if k != which]
    return f32hp(**{which: value, rest[0]: OTHERS[0], rest[1]: OTHERS[1], "lambda_": 0.9})


HP_SETS = {}
for _k in CLIPS:
    HP_SETS[f"{_k}_half"] = _clip_hp(_k, HALF)
    HP_SETS[f"{_k}_never"] = _clip_hp(_k, NEVER)
for _l in (0.0, 0.5, 1.0):
    HP_SETS[f"lambda_{_l}"] = f32hp(lambda_=_l, rho_bar=1.5, c_bar=0.75, pg_rho_bar=1.25)
HP_SETS["baseline_cost_0"] = f32hp(baseline_cost=0.0)
HP_SETS["entropy_cost_0"] = f32hp(entropy_cost=0.0)
HP_SETS["both_costs_0"] = f32hp(baseline_cost=0.0, entropy_cost=0.0)
for _n, _h in HP_SETS.items():
    BUILDERS["hp:" + _n] = (lambda h: lambda seed, T, B, A: unit_case(seed, T, B, A, done_p=0.05) + (h,))(_h)


# ---- section f: input regimes
@builder("disc_zero")
def _disc_zero(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return pi, mu, act, rew, np.zeros_like(disc), val, f32hp()


@builder("disc_one_long_memory")
def _disc_one(seed, T, B, A):
    """disc = 1, lambda = 1, no clip binds: acc_t keeps every later delta, weighted by the product of
    the ratios between. Logits x 0.25 keep that product within a few decades over 65 steps."""
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A, scale=0.25)
    return pi, mu, act, rew, np.ones_like(disc), val, f32hp(rho_bar=NEVER, c_bar=NEVER, pg_rho_bar=NEVER)


@builder("disc_zero_at_edges")
def _disc_edges(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A, done_p=0.0)
    for t in (0, 31, 32, T - 1):
        if 0 <= t < T:
            disc[t] = 0.0
    return pi, mu, act, rew, disc, val, f32hp()


@builder("pi_equals_mu")
def _pi_eq_mu(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return pi, pi.copy(), act, rew, disc, val, f32hp()


@builder("equal_logits")
def _equal_logits(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return np.full_like(pi, 0.75), np.full_like(mu, -1.5), act, rew, disc, val, f32hp()


@builder("actions_first")
def _act_first(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return pi, mu, np.zeros_like(act), rew, disc, val, f32hp()


@builder("actions_last")
def _act_last(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return pi, mu, np.full_like(act, A - 1), rew, disc, val, f32hp()


@builder("rewards_zero")
def _rew_zero(seed, T, B, A):
    """No reward and no episode end; V_t = 0.05 * 1.1^t (1 % noise), so that g V_{t+1} - V_t is
    about 0.09 V_t for every t: the deltas keep one sign (condition_numbers) with rewards at 0."""
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A, done_p=0.0)
    rs = np.random.RandomState(seed + 1)
    val = (0.05 * 1.1 ** np.arange(T + 1)[:, None] * (1 + 0.01 * rs.randn(T + 1, B))).astype(np.float32)
    return pi, mu, act, np.zeros_like(rew), disc, val, f32hp()


SATURATION = 60.0


@builder("saturated")
def _saturated(seed, T, B, A):
    """randn logits x 60: softmaxes are one-hot to fp32, pi(a)/mu(a) overflows fp32 in some rows
    and underflows it in others. (x 30 saturates as well, but only 2.5 % of its ratios pass FLT_MAX
    and 1.7 % fall below FLT_MIN at T = 40, A = 6; tests/test_vtrace_reference.py asks for 5 %.)"""
    return unit_case(seed, T, B, A, scale=SATURATION) + (f32hp(),)


@builder("action_80_below_max")
def _a80(seed, T, B, A):
    """The taken action's logit is 80 below the row maximum in pi and in mu: pi(a) and mu(a) are
    about e^-80 = 2^-115, at the small end of fp32, while their ratio is of order 1."""
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    idx = act[..., None].astype(np.int64)
    for z in (pi, mu):
        np.put_along_axis(z, idx, np.float32(-1e4), -1)  # out of the row maximum
        np.put_along_axis(z, idx, z.max(-1, keepdims=True) - np.float32(80.0), -1)
    return pi, mu, act, rew, disc, val, f32hp()


def _offset(off):
    def fn(seed, T, B, A):
        pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
        return pi + np.float32(off), mu + np.float32(off), act, rew, disc, val, f32hp()
    return fn


BUILDERS["offset_plus_100"] = _offset(100.0)
BUILDERS["offset_minus_100"] = _offset(-100.0)


RETURNS_SCALE = 1e3


@builder("returns_1e3")
def _big(seed, T, B, A):
    pi, mu, act, rew, disc, val = unit_case(seed, T, B, A)
    return pi, mu, act, rew * np.float32(RETURNS_SCALE), disc, val * np.float32(RETURNS_SCALE), f32hp()


UNIT_REGIMES = ("disc_zero", "disc_one_long_memory", "disc_zero_at_edges", "pi_equals_mu",
                "equal_logits", "actions_first", "actions_last", "rewards_zero")
WIDE_REGIMES = ("saturated", "action_80_below_max", "offset_plus_100", "offset_minus_100",
                "returns_1e3")
EF_SHAPES = ((40, 16, 6), (65, 8, 18))


# ------------------------------------------------------------------------------------------
# the matrix's case lists: (builder, seed, T, B, A)
# ------------------------------------------------------------------------------------------
def str_shape_ok(T, A):
    """variant 4's limits (vtrace.hip str_supported, the source of truth): T <= 127, T * A <= 2048
    dlogits pieces, the two whole-sequence slots within 160 KB of LDS."""
    lds = 2 * 1024 * (2 * -(-T * 16 * A // 1024) + 3 * -(-T * 16 // 1024) + -(-(T + 1) * 16 // 1024)) + 256
    return T <= 127 and T * A <= 2048 and lds <= 160 * 1024


def _seed(T, B, A):
    return 7919 * T + 31 * B + A


def cases_a(A):
    """Section a: the production kernel at every chunk residue, one and three workgroups."""
    return [("base", _seed(T, B, A), T, B, A) for B in (8, 24) for T in range(1, 71)]


def cases_mixed(A):
    """One mixed-sign case per instantiation and fast kernel's column count: chunk residues 1 and
    9, three whole-or-part chunks."""
    return [("mixed_sign", _seed(T, B, A) + 6, T, B, A) for T, B in ((33, 8), (70, 24))]


B_TS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def cases_b(A, variant):
    """Section b: the on-request kernels. Variant 4's list is unfiltered: the test drops what
    str_shape_ok excludes and counts it."""
    return [("base", _seed(T, B, A) + 1, T, B, A) for B in ((8,) if variant == 3 else (4, 12)) for T in B_TS]


C_AS, C_BS, C_TS = (1, 2, 3, 5, 9, 17, 19, 21, 63, 64), (1, 7, 255, 256, 257, 513), (1, 2, 9)


def cases_c(A):
    return [("base", _seed(T, B, A) + 2, T, B, A) for B in C_BS for T in C_TS]


def cases_d(cus):
    """Section d: (variant, case). Persistent grids with a ragged last round, and the finalize
    kernel's 256 threads over nblk partials on both sides of 256."""
    b3 = next(B for B in range(8, 1 << 20, 8) if B // 2 > 2 * cus)
    shapes = [(4, 3, 4 * (cus + 1), 18), (4, 3, 4 * (2 * cus + 3), 18), (3, 3, b3, 18), (3, 3, b3 + 8, 18)]
    # sequences so short that a group has fewer DMA pieces than the streaming kernel has waves
    # (6 against 8), on workgroups that walk a second and a third group
    shapes += [(4, T, 4 * (2 * cus + 3), A) for T, A in ((1, 18), (2, 2), (32, 2), (16, 4))]
    shapes += [(1, 2, 8 * n, 2) for n in (1, 2, 255, 256, 257, 513)]
    shapes += [(2, 2, 256 * n - 1, 2) for n in (1, 2, 5)]
    return [(v, ("base", _seed(T, B, A) + 3, T, B, A)) for v, T, B, A in shapes]


def cases_e():
    return [("hp:" + n, _seed(T, B, A) + 4, T, B, A) for n in HP_SETS for T, B, A in EF_SHAPES]


def cases_f(names=UNIT_REGIMES + WIDE_REGIMES):
    return [(n, _seed(T, B, A) + 5, T, B, A) for n in names for T, B, A in EF_SHAPES]


def all_cases(cus=CUS_MI355X):
    """{section: [case]} of everything the GPU matrix runs."""
    out = {}
    for A in EVEN_A:
        out[f"a-A{A}"] = cases_a(A)
        out[f"m-A{A}"] = cases_mixed(A)
        out[f"b-A{A}"] = cases_b(A, 3) + [c for c in cases_b(A, 4) if str_shape_ok(c[2], A)]
    for A in C_AS:
        out[f"c-A{A}"] = cases_c(A)
    out["d"] = [c for _, c in cases_d(cus)]
    out["e"] = cases_e()
    out["f"] = cases_f()
    return out


# ------------------------------------------------------------------------------------------
# launching a kernel variant and holding it against a reference
# ------------------------------------------------------------------------------------------
GUARD_BYTES = 4096
SENTINEL = 0x7FC5A5A5  # a quiet-NaN payload: a sentinel read as an output fails the finite check too


class _Out:
    """A device output tensor; with guard, GUARD_BYTES of SENTINEL words on both sides of it (the
    tensor starts GUARD_BYTES into the allocation, so it keeps hipMalloc's 16-byte alignment)."""

    def __init__(self, nbytes, guard):
        from freeimpala_amd import hip
        self.nbytes, self.guard = nbytes, guard
        if guard:
            self.words = (nbytes + 3) // 4 + 2 * (GUARD_BYTES // 4)
            self.buf = hip.DeviceBuffer(4 * self.words)
            self.buf.upload(np.full(self.words, SENTINEL, np.uint32))
            self.ptr = self.buf.ptr + GUARD_BYTES
            assert self.ptr % 16 == 0
        else:
            self.buf = hip.DeviceBuffer(nbytes)
            self.ptr = self.buf.ptr

    def download(self, dtype, shape, what):
        if not self.guard:
            return self.buf.download(dtype, shape)
        raw = self.buf.download(np.uint32, (self.words,))
        g = GUARD_BYTES // 4
        lo, hi = raw[:g], raw[g + (self.nbytes + 3) // 4:]
        assert hi.size == g
        for side, w in (("below", lo), ("above", hi)):
            bad = np.flatnonzero(w != SENTINEL)
            assert bad.size == 0, f"{what}: {bad.size} guard words {side} the tensor overwritten, first at word {bad[0]}"
        return raw[g:].view(np.uint8)[:self.nbytes].view(dtype).reshape(shape).copy()


def run_vtrace(pi, mu, act, rew, disc, val, variant=0, guard=False, null_targets=False,
               logits_byte_shift=0, ws_short=0, **hp):
    """One launch of kernel `variant` through the C ABI. null_targets passes vs = adv = NULL;
    logits_byte_shift moves the pi pointer; ws_short declares the workspace that many bytes short
    (the last three are for the launcher's refusals)."""
    from freeimpala_amd import _abi, hip
    T, B, A = pi.shape
    h = dict(HP_DEFAULT)
    h.update(hp)
    H = _abi.VtraceHparams(**h)
    bufs = {k: hip.DeviceBuffer.from_array(np.ascontiguousarray(v, dt))
            for k, v, dt in [("pi", pi, np.float32), ("mu", mu, np.float32),
                             ("act", act, np.int32), ("rew", rew, np.float32),
                             ("disc", disc, np.float32), ("val", val, np.float32)]}
    vs = _Out(T * B * 4, guard)
    adv = _Out(T * B * 4, guard)
    dl = _Out(T * B * A * 4, guard)
    dv = _Out((T + 1) * B * 4, guard)
    loss = _Out(3 * 8, guard)
    wsb = _abi.lib().fi_vtrace_workspace_bytes(T, B, A)
    ws = hip.DeviceBuffer(wsb)
    ws.zero()
    rc = _abi.lib().fi_vtrace_loss_fp32_variant(
        variant, T, B, A, bufs["pi"].ptr + logits_byte_shift, bufs["mu"].ptr, bufs["act"].ptr,
        bufs["rew"].ptr, bufs["disc"].ptr, bufs["val"].ptr, C.byref(H),
        None if null_targets else vs.ptr, None if null_targets else adv.ptr, dl.ptr, dv.ptr,
        loss.ptr, ws.ptr, wsb - ws_short, None)
    _abi.check(rc, "fi_vtrace_loss_fp32_variant")
    hip.synchronize()
    return dict(vs=vs.download(np.float32, (T, B), "vs"), pg_adv=adv.download(np.float32, (T, B), "pg_adv"),
                dlogits=dl.download(np.float32, (T, B, A), "dlogits"),
                dvalue=dv.download(np.float32, (T + 1, B), "dvalue"),
                losses=loss.download(np.float64, (3,), "losses"))


def _close(a, b, tol=TOL, what=""):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert np.isfinite(a).all(), what
    assert err.max() <= tol, f"{what}: max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


def compare_tensors(out, ref, tol=TOL):
    for k in ("vs", "pg_adv", "dlogits", "dvalue"):
        _close(out[k], ref[k], tol, k)


def compare(out, ref, tol=TOL):
    compare_tensors(out, ref, tol)
    for i in range(3):
        r = ref["losses"][i]
        assert abs(out["losses"][i] - r) <= tol * max(1.0, abs(r)), (i, out["losses"], ref["losses"])


def assert_bitwise(x, y, keys=("vs", "pg_adv", "dlogits", "dvalue", "losses"), what=""):
    for k in keys:
        ax, ay = np.ascontiguousarray(x[k]), np.ascontiguousarray(y[k])
        assert ax.dtype == ay.dtype and ax.tobytes() == ay.tobytes(), f"{what}: {k} differs bitwise"


def device_cu_count():
    """The compute-unit count of the current device (hipDeviceGetAttribute)."""
    from freeimpala_amd import hip
    L = hip.hip()
    dev, n = C.c_int(0), C.c_int(0)
    assert L.hipGetDevice(C.byref(dev)) == 0
    assert L.hipDeviceGetAttribute(C.byref(n), 63, dev) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 1 <= n.value <= 4096, n.value
    return n.value


# ------------------------------------------------------------------------------------------
# the derived bar of the wide regimes (docstring of tests/test_gpu_vtrace_matrix.py)
# ------------------------------------------------------------------------------------------
def wide_scales(pi, mu, ref):
    """Multipliers of the 1e-5 bar: s (T, B) for what passes through a log-probability, s times
    max(1, |pg_adv_ref|) for dlogits, the mean row scale for the loss sums."""
    z = np.maximum(np.abs(np.asarray(pi, np.float64)).max(-1), np.abs(np.asarray(mu, np.float64)).max(-1))
    s = np.maximum(1.0, z)
    sd = s * np.maximum(1.0, np.abs(ref["pg_adv"]))
    s_dv = np.concatenate([s, np.ones((1, s.shape[1]))], 0)  # the bootstrap row is an exact 0
    return dict(vs=s, pg_adv=s, dvalue=s_dv, dlogits=sd[..., None], losses=np.full(3, s.mean()))


def scaled_errors(out, ref, scales):
    """Worst error of each output in units of its bar: |d| / (1e-5 * scale * max(1, |ref|))."""
    res = {}
    for k in ("vs", "pg_adv", "dlogits", "dvalue", "losses"):
        a, b = np.asarray(out[k], np.float64), np.asarray(ref[k], np.float64)
        if not np.isfinite(a).all():
            res[k] = float("inf")
            continue
        res[k] = float((np.abs(a - b) / (TOL * scales[k] * np.maximum(1.0, np.abs(b)))).max())
    return res
