// vmpo.hip -- the V-MPO objective on the learner (include/fi_vmpo.h, where the rule stands): an exact select
// of the top fraction of the T * B advantages on the device, the weighted-likelihood loss over that part
// with softmax(A / eta) weights, the temperature's Adam step, and every fi_vmpo_* entry point.
//
//   vmpo_clear_kernel    the three histograms and the key maximum to 0 (a kernel, not a memset node).
//   vmpo_hist_kernel<P>  pass P of a radix select over the order-preserving key of an advantage, digits of
//                        11, 11 and 10 bits from the top. A grid-stride stream over adv, 16 bytes per lane
//                        and access, two accesses in flight, a scalar tail. Passes 1 and 2 open with wave 0
//                        of every workgroup scanning the earlier global histograms from the top (32 bins per
//                        lane, a wave scan of the lane sums, then the lane that holds rank k walks its 32
//                        bins): the bin that holds rank k and the rank that remains; only rows whose prefix
//                        matches are counted. fp32 advantages sit in a handful of exponents, so pass 0 puts
//                        most rows into a few bins: each wave has its own 2,048-bin u32 histogram in LDS
//                        (32 KB per workgroup; no two waves meet on a word), and inside a wave the lanes
//                        whose digit equals the first active lane's are counted by one ds_add of their
//                        popcount; only the others issue their own. All-equal input costs one LDS atomic
//                        per wave and access. The four sub-histograms are added and flushed with global
//                        integer atomics, empty bins skipped. Pass 0 also takes the key maximum (a lane
//                        maximum, a wave maximum, one atomicMax per wave).
//   vmpo_sums_kernel     every workgroup resolves tau from the three histograms; m comes out of the same
//                        scan exactly (the counts above the chosen bins plus the last bin's), so it is not
//                        counted again. The stream then accumulates S and W over D in two fp64 accumulators
//                        per lane and quantity, wave_reduce, block_sums, one pair per workgroup. Workgroup 0
//                        leaves key_tau and m in the workspace and rows, selected, threshold, adv_max in
//                        the block.
//   vmpo_loss_kernel     surrogate_loss_kernel's grid and read pattern (row_stream.h) over pi: padded LDS
//                        rows, one lane per row, policy_row_grad_t<true> (policy_row.h); every workgroup adds
//                        the S and W partials itself in one fixed order, so no finalize launch stands
//                        between; dlogits leave through LDS as 16-byte pieces; three fp64 loss partials per
//                        workgroup; workgroup 0 writes loss_eta, d_eta, S and W into the block.
//   vmpo_eta_kernel      rule 5: one Adam step on eta in fp64 behind the optimiser.
//   vmpo_losses_kernel   the stand-alone entry's three loss scalars.
// No float atomics. learner.cpp names nothing of this file: fi_vmpo_enable hangs a VmpoBlock with the two
// launchers on the handle (kernels.h). The targets are surrogate.hip's rows and scan kernels, unchanged
// (surrogate_front_launch).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "atari.h"  // KernelTagger, TagScope
#include "fi_common.h"
#include "fi_vmpo.h"
#include "host_util.h"
#include "kernels.h"
#include "policy_row.h"
#include "row_stream.h"

namespace fi {

namespace {
static_assert(sizeof(fi_vmpo_state) == 88 && sizeof(fi_vmpo_params) == 32, "fi_vmpo.h fixes both sizes");

constexpr int kBins = 2048;        // 11 bits; the last digit's 10 bits use the lower half
constexpr int kSelThreads = 256;   // four waves
constexpr int kSelGridMax = 256;   // one workgroup per CU: the stream is 1.6 MB at T = 100, B = 4096
constexpr int kBinsPerLane = kBins / 64;
static_assert(kSelThreads == 64 * kWaves, "one sub-histogram per wave of a select workgroup");
// the selection's words in the workspace
enum { SEL_KEYMAX = 0, SEL_TAU = 1, SEL_M = 2 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SelArgs {
    const float* __restrict__ adv;
    uint32_t n, n4, k;
    int grid;
    uint32_t* hist;  // [3][kBins]
    uint32_t* sel;   // 64 words
    double* part;    // [grid][2]: S, W
    fi_vmpo_state* state;
};

// rule 1
__device__ __forceinline__ uint32_t key_of(float x) {
    const uint32_t u = __float_as_uint(x + 0.0f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// rule 3's e_i, one instruction sequence for the sums and the loss kernel; *d = a - Amax. A non-finite
// advantage gives NaN (rule 6)
__device__ __forceinline__ float weight_of(float adv, float amax, float eta, float* d) {
#pragma clang fp contract(off)  // the same roundings wherever this is inlined
    const float a = adv + 0.0f;
    *d = a - amax;
    return fabsf(a) <= 3.4028234664e38f ? expf(*d / eta) : __builtin_nanf("");
}

// The bin of a 2,048-bin histogram that holds rank k counted from the top (1 <= k <= the histogram's
// total), the count above it and its own. One wave: lane L holds the bins 2047 - 32 L - 31 .. 2047 - 32 L.
struct Pick {
    uint32_t bin, above, count;
};
__device__ __forceinline__ Pick wave_pick(const uint32_t* __restrict__ hist, uint32_t k, int lane) {
    const int base = kBins - kBinsPerLane * (lane + 1);
    const u32x4* __restrict__ h4 = (const u32x4*)(hist + base);
    uint32_t v[kBinsPerLane];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < kBinsPerLane / 4; ++j) {
        const u32x4 q = h4[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[4 * j + c] = q[c];
            mine += q[c];
        }
    }
    uint32_t inc = mine;  // inclusive scan, lane 0 the top bins
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    const unsigned long long hit = __ballot(inc >= k);
    const int src = hit ? __ffsll((long long)hit) - 1 : 63;
    uint32_t run = inc - mine, bin = (uint32_t)base, above = run, count = 0u;
    bool found = false;
#pragma unroll
    for (int j = kBinsPerLane - 1; j >= 0; --j) {
        if (!found) {
            bin = (uint32_t)(base + j), above = run, count = v[j];
            if (run + v[j] >= k) found = true;
            else run += v[j];
        }
    }
    return Pick{(uint32_t)__shfl((int)bin, src, 64), (uint32_t)__shfl((int)above, src, 64),
                (uint32_t)__shfl((int)count, src, 64)};
}

// Wave 0 walks the first `passes` histograms: pick[2 p] the bin of pass p, pick[2 p + 1] the rank handed on;
// behind three passes pick[6] = m. The other waves wait at the caller's barrier.
__device__ __forceinline__ void resolve(const SelArgs& a, int passes, uint32_t* pick, int lane, int w) {
    if (w != 0) return;
    uint32_t k = a.k, m = 0;
    for (int p = 0; p < passes; ++p) {
        const Pick c = wave_pick(a.hist + p * kBins, k, lane);
        k -= c.above;
        m += c.above;
        if (lane == 0) pick[2 * p] = c.bin, pick[2 * p + 1] = k;
        if (p == 2 && lane == 0) pick[6] = m + c.count;
    }
}

// One digit per lane into this wave's sub-histogram: the lanes that share the first valid lane's digit
// by one add of their count, the others by their own. Wave-uniform call.
__device__ __forceinline__ void count_digit(uint32_t* sub, uint32_t d, bool valid, int lane) {
    const unsigned long long act = __ballot(valid);
    if (!act) return;
    const int lead = __ffsll((long long)act) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, lead, 64);
    const bool same = valid && d == d0;
    const unsigned long long grp = __ballot(same);
    if (lane == lead) atomicAdd(&sub[d0], (uint32_t)__popcll(grp));
    else if (valid && !same) atomicAdd(&sub[d], 1u);
}
}  // namespace

__global__ __launch_bounds__(kSelThreads) void vmpo_clear_kernel(uint32_t* hist, uint32_t* sel) {
    const int i = blockIdx.x * kSelThreads + threadIdx.x;
    if (i < 3 * kBins) hist[i] = 0u;
    if (i < 64) sel[i] = 0u;
}

template <int PASS>
__global__ __launch_bounds__(kSelThreads) void vmpo_hist_kernel(SelArgs a) {
    __shared__ uint32_t sub[kWaves][kBins];
    __shared__ uint32_t pick[8];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    for (int i = tid; i < kWaves * kBins; i += kSelThreads) (&sub[0][0])[i] = 0u;
    resolve(a, PASS, pick, lane, w);
    __syncthreads();
    uint32_t prefix = 0;
    if (PASS == 1) prefix = pick[0];
    if (PASS == 2) prefix = (pick[0] << 11) | pick[2];
    uint32_t* const mysub = sub[w];
    uint32_t kmax = 0;
    auto take = [&](float x, bool inb) {
        const uint32_t key = key_of(x);
        if (PASS == 0) {
            if (inb) kmax = max(kmax, key);
            count_digit(mysub, key >> 21, inb, lane);
        } else if (PASS == 1) {
            count_digit(mysub, (key >> 10) & 0x7FFu, inb && (key >> 21) == prefix, lane);
        } else {
            count_digit(mysub, key & 0x3FFu, inb && (key >> 10) == prefix, lane);
        }
    };
    const f32x4* __restrict__ a4 = (const f32x4*)a.adv;
    const uint32_t stride = (uint32_t)a.grid * kSelThreads;
    // wave-uniform trips: two accesses of 16 bytes per lane in flight
    for (uint32_t base = blockIdx.x * kSelThreads + (uint32_t)w * 64u; base < a.n4; base += 2u * stride) {
        const uint32_t i0 = base + lane, i1 = i0 + stride;
        const bool in0 = i0 < a.n4, in1 = i1 < a.n4;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
        if (in0) v0 = a4[i0];
        if (in1) v1 = a4[i1];
#pragma unroll
        for (int j = 0; j < 4; ++j) take(v0[j], in0);
        if (__ballot(in1)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) take(v1[j], in1);
        }
    }
    if (blockIdx.x == 0 && w == 0) {  // the n mod 4 rows behind the last whole piece
        const uint32_t e = 4u * a.n4 + lane;
        const bool inb = e < a.n;
        take(inb ? a.adv[e] : 0.f, inb);
    }
    if (PASS == 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off, 64));
        if (lane == 0 && kmax) atomicMax(&a.sel[SEL_KEYMAX], kmax);
    }
    __syncthreads();
    uint32_t* const out = a.hist + PASS * kBins;
    for (int b = tid; b < kBins; b += kSelThreads) {
        uint32_t c = 0;
#pragma unroll
        for (int w2 = 0; w2 < kWaves; ++w2) c += sub[w2][b];
        if (c) atomicAdd(&out[b], c);
    }
}

__global__ __launch_bounds__(kSelThreads) void vmpo_sums_kernel(SelArgs a) {
    __shared__ uint32_t pick[8];
    __shared__ double red[kWaves * 2];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    resolve(a, 3, pick, lane, w);
    __syncthreads();
    const uint32_t tau = (pick[0] << 21) | (pick[2] << 10) | pick[4];
    const uint32_t kmax = a.sel[SEL_KEYMAX];
    const float amax = float_of(kmax), eta = (float)a.state->eta;
    double s[2] = {0.0, 0.0}, wsum[2] = {0.0, 0.0};
    auto take = [&](float x, bool inb, int acc) {
        float d;
        const float e = weight_of(x, amax, eta, &d);
        if (inb && (key_of(x) >= tau || !(e == e))) {
            s[acc] += (double)e;
            wsum[acc] += (double)e * (double)d;
        }
    };
    const f32x4* __restrict__ a4 = (const f32x4*)a.adv;
    const uint32_t stride = (uint32_t)a.grid * kSelThreads;
    for (uint32_t base = blockIdx.x * kSelThreads + (uint32_t)w * 64u; base < a.n4; base += 2u * stride) {
        const uint32_t i0 = base + lane, i1 = i0 + stride;
        const bool in0 = i0 < a.n4, in1 = i1 < a.n4;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
        if (in0) v0 = a4[i0];
        if (in1) v1 = a4[i1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            take(v0[j], in0, j & 1);
            take(v1[j], in1, j & 1);
        }
    }
    if (blockIdx.x == 0 && w == 0) {
        const uint32_t e = 4u * a.n4 + lane;
        const bool inb = e < a.n;
        take(inb ? a.adv[e] : 0.f, inb, 0);
    }
    double v[2] = {s[0] + s[1], wsum[0] + wsum[1]};
    block_sums<2, kWaves>(v, red);
    if (tid == 0) {
        a.part[2 * (size_t)blockIdx.x] = v[0];
        a.part[2 * (size_t)blockIdx.x + 1] = v[1];
        if (blockIdx.x == 0) {
            a.sel[SEL_TAU] = tau;
            a.sel[SEL_M] = pick[6];
            a.state->rows = a.n;
            a.state->selected = pick[6];
            a.state->threshold = float_of(tau);
            a.state->adv_max = amax;
        }
    }
}

namespace {
struct LossArgs {
    int T, B, A;
    int ct, slices, slice_len, nsel;
    const float* __restrict__ pi;
    const int32_t* __restrict__ act;
    const float* __restrict__ adv;
    const float* __restrict__ vs;
    const float* __restrict__ val;
    float* dlog;
    float* dval;
    const uint32_t* sel;
    const double* selpart;  // [nsel][2]
    double* part;           // [ct * slices][3]
    fi_vmpo_state* state;
    int* bad;
    int count_bad;
    float bc, ec, eps_eta;
};
}  // namespace

__global__ __launch_bounds__(64 * kWaves) void vmpo_loss_kernel(LossArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    __shared__ double red[kWaves * 3];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * kCols * S;  // this wave's pi rows, dlogits after the arithmetic
    const uint32_t n = (uint32_t)nb * A;
    // S and W: thread i adds the partials i, i + 256, ... in ascending order, then block_sums; every
    // workgroup holds the same bits
    double sw[2] = {0.0, 0.0};
    for (int i = tid; i < a.nsel; i += kStatThreads) {
        sw[0] += a.selpart[2 * i];
        sw[1] += a.selpart[2 * i + 1];
    }
    block_sums<2, kWaves>(sw, red);
    const uint32_t tau = a.sel[SEL_TAU];
    const float amax = float_of(a.sel[SEL_KEYMAX]);
    const double eta_d = a.state->eta, rows = (double)T * (double)B;
    const float eta = (float)eta_d;
    const double n_over_s = rows / sw[0];
    if (blockIdx.x == 0 && tid == 0) {  // rule 5's two scalars
        const double m = (double)a.sel[SEL_M], lsm = log(sw[0] / m), eps = (double)a.eps_eta;
        a.state->loss_eta = eta_d * eps + (double)amax + eta_d * lsm;
        a.state->d_eta = eps + lsm - sw[1] / (sw[0] * eta_d);
        a.state->sum_e = sw[0];
        a.state->sum_ea = sw[1];
    }
    if (s == 0 && tid < nb) a.dval[(size_t)T * B + b0 + tid] = 0.f;  // the bootstrap row has no gradient
    int nbad = 0;
    double sum[3] = {0.0, 0.0, 0.0};  // L_pg, baseline, entropy
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        const uint32_t g0 = ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A;
        int at = 0;
        float adv = 0.f, v = 0.f, vs = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            adv = a.adv[e];
            v = a.val[e];
            vs = a.vs[e];
        }
        if (live) load_run<false>(a.pi, nullptr, lp, nullptr, g0, n, A, S, lane);
        __syncthreads();  // the rows are in LDS
        if (mine) {
            float* __restrict__ z = lp + (uint32_t)lane * S;
            if ((unsigned)at >= A) ++nbad;
            const uint32_t ai = at < 0 ? 0u : ((uint32_t)at >= A ? A - 1u : (uint32_t)at);
            float d;
            const float e = weight_of(adv, amax, eta, &d);
            const bool in_d = key_of(adv) >= tau || !(e == e);
            const float g = in_d ? -(float)((double)e * n_over_s) : 0.f;  // -n psi
            float logp;
            const float plogp = policy_row_grad_t<true>(z, A, ai, g, a.ec, &logp);  // z holds dlogits now
            const float td = v - vs;
            a.dval[(size_t)t * B + b0 + lane] = a.bc * td;
            if (in_d) sum[0] += (double)g * (double)logp;
            sum[1] += 0.5 * (double)td * (double)td;
            sum[2] += (double)plogp;
        }
        __syncthreads();  // the dlogits rows are complete
        if (live) store_run(a.dlog, lp, g0, n, A, S, lane);
        __syncthreads();  // the rows have left: the next round may overwrite them
    }
    block_sums<3, kWaves>(sum, red);
    if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = sum[tid];
    if (a.count_bad) {
        const unsigned long long any = __ballot(nbad != 0);
        if (any) {  // wave-uniform; the rare path
            int tot = nbad;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
            if (lane == 0) atomicAdd(a.bad, tot);
        }
    }
}

// One workgroup, the stand-alone entry: the loss partials added in a fixed order; NaN when an action was
// outside [0, A) (that entry has no synchronous status to return)
__global__ __launch_bounds__(kStatThreads) void vmpo_losses_kernel(const double* __restrict__ part, int nblk,
                                                                   const int* __restrict__ bad, double* losses) {
    __shared__ double red[kWaves * 3];
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += kStatThreads) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += part[(size_t)i * 3 + j];
    }
    block_sums<3, kWaves>(v, red);
    if (threadIdx.x != 0) return;
    const bool poisoned = *bad != 0;
    for (int i = 0; i < 3; ++i) losses[i] = poisoned ? __builtin_nan("") : v[i];
}

// Rule 5's update: one lane. skip (nullable): the optimiser's flag words.
__global__ __launch_bounds__(64) void vmpo_eta_kernel(fi_vmpo_state* st, fi_vmpo_params p, const int* __restrict__ skip) {
    if (threadIdx.x != 0 || !p.adapt) return;
    if (skip && (skip[0] | skip[1]) != 0) return;  // the update was skipped: so is this
    const double g = st->d_eta;
    if (!(fabs(g) < __builtin_inf())) return;  // NaN or Inf
    const double b1 = 0.9, b2 = 0.999;
    const double t = (double)(st->updates + 1);
    const double m1 = b1 * st->m1 + (1.0 - b1) * g, m2 = b2 * st->m2 + (1.0 - b2) * g * g;
    const double mh = m1 / (1.0 - pow(b1, t)), vh = m2 / (1.0 - pow(b2, t));
    const double eta = st->eta - (double)p.lr_eta * mh / (sqrt(vh) + 1e-8);
    st->m1 = m1;
    st->m2 = m2;
    st->eta = fmax((double)p.eta_min, eta);
    st->updates = st->updates + 1;
}

// ------------------------------------------------------------------ the launchers
namespace {
size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: three histograms | the selection's words (256 bytes) | 256 pairs of S, W partials -- so far
// FI_VMPO_SELECT_WS_BYTES -- | loss partials | the stand-alone entry's bad-action counter
struct Layout {
    size_t sel, selpart, part, bad, total;
};
constexpr size_t kHistBytes = 3 * (size_t)kBins * sizeof(uint32_t);
static_assert(kHistBytes + 256 + kSelGridMax * 2 * sizeof(double) == FI_VMPO_SELECT_WS_BYTES, "fi_vmpo.h names the size");
Layout layout_of(const TilePlan& p) {
    Layout l{};
    l.sel = kHistBytes;
    l.selpart = l.sel + 256;
    l.part = FI_VMPO_SELECT_WS_BYTES;
    l.bad = l.part + pad256((size_t)p.ct * p.slices * 3 * sizeof(double));
    l.total = l.bad + 256;
    return l;
}

int select_blocks(int64_t n) {
    if (n < 1 || n >= ((int64_t)1 << 31)) return 0;
    const int64_t want = (n / 4 + kSelThreads - 1) / kSelThreads;
    return (int)(want < 1 ? 1 : (want > kSelGridMax ? kSelGridMax : want));
}

// FI_ERR_INVALID, `who` opens the message
int check_params(const std::string& who, const fi_vmpo_params* p) {
    FI_REQUIRE(p, who + ": null params");
    FI_REQUIRE(std::isfinite(p->top_fraction) && p->top_fraction > 0.f && p->top_fraction <= 1.f,
               who + ": top_fraction " + std::to_string(p->top_fraction) + " must be in (0, 1]");
    FI_REQUIRE(std::isfinite(p->eps_eta) && p->eps_eta > 0.f, who + ": eps_eta " + std::to_string(p->eps_eta) + " must be finite and > 0");
    FI_REQUIRE(std::isfinite(p->eta_min) && p->eta_min > 0.f, who + ": eta_min " + std::to_string(p->eta_min) + " must be finite and > 0");
    FI_REQUIRE(std::isfinite(p->eta_init) && p->eta_init >= p->eta_min,
               who + ": eta_init " + std::to_string(p->eta_init) + " must be finite and >= eta_min");
    FI_REQUIRE(std::isfinite(p->lr_eta) && p->lr_eta >= 0.f, who + ": lr_eta " + std::to_string(p->lr_eta) + " must be finite and >= 0");
    FI_REQUIRE(p->adapt <= 1u, who + ": adapt " + std::to_string(p->adapt) + " must be 0 or 1");
    return FI_OK;
}

int check_eta(const std::string& who, double eta) {
    FI_REQUIRE(std::isfinite(eta) && eta > 0.0, who + ": eta " + std::to_string(eta) + " must be finite and > 0");
    return FI_OK;
}

int select_launch(int64_t n, const float* adv, const fi_vmpo_params* prm, void* state, void* ws, size_t ws_bytes,
                  hipStream_t stream, KernelTagger* tg) {
    FI_TRY(check_params("vmpo_select", prm));
    FI_REQUIRE(adv && state && ws, "vmpo_select: null argument");
    const int grid = select_blocks(n);
    FI_REQUIRE(grid > 0, "vmpo_select: n = " + std::to_string(n) + " outside 1 .. 2^31 - 1");
    FI_REQUIRE((uintptr_t)adv % 16 == 0, "vmpo_select: adv must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)state % 8 == 0 && (uintptr_t)ws % 16 == 0, "vmpo_select: the state block must be 8-byte, ws 16-byte aligned");
    FI_REQUIRE(ws_bytes >= FI_VMPO_SELECT_WS_BYTES,
               "vmpo_select: ws_bytes " + std::to_string(ws_bytes) + " < FI_VMPO_SELECT_WS_BYTES = " + std::to_string(FI_VMPO_SELECT_WS_BYTES));
    char* w = (char*)ws;
    SelArgs a{};
    a.adv = adv;
    a.n = (uint32_t)n, a.n4 = (uint32_t)(n / 4);
    const double fk = std::floor((double)prm->top_fraction * (double)n);
    a.k = fk < 1.0 ? 1u : (uint32_t)fk;
    a.grid = grid;
    a.hist = (uint32_t*)w, a.sel = (uint32_t*)(w + kHistBytes), a.part = (double*)(w + kHistBytes + 256);
    a.state = (fi_vmpo_state*)state;
    const dim3 g((unsigned)grid), t(kSelThreads);
    {
        TagScope s(tg, "vmpo_clear");
        hipLaunchKernelGGL(vmpo_clear_kernel, dim3(3 * kBins / kSelThreads), t, 0, stream, a.hist, a.sel);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope s(tg, "vmpo_hist0");
        hipLaunchKernelGGL(vmpo_hist_kernel<0>, g, t, 0, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope s(tg, "vmpo_hist1");
        hipLaunchKernelGGL(vmpo_hist_kernel<1>, g, t, 0, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope s(tg, "vmpo_hist2");
        hipLaunchKernelGGL(vmpo_hist_kernel<2>, g, t, 0, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope s(tg, "vmpo_sums");
        hipLaunchKernelGGL(vmpo_sums_kernel, g, t, 0, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    return FI_OK;
}

// count_bad: the loss kernel counts the out-of-range actions (the stand-alone entry; on a handle the rows
// kernel in front has counted them)
int loss_launch(int T, int B, int A, const float* pi, const int32_t* act, const float* adv, const float* vs, const float* val,
                const fi_vtrace_hparams& hp, const fi_vmpo_params* prm, void* state, float* dlog, float* dval, double* losses,
                void* ws, size_t ws_bytes, int* bad, bool count_bad, hipStream_t stream, KernelTagger* tg,
                const double** partials, int* nblk_out) {
    FI_TRY(check_params("vmpo_loss", prm));
    FI_REQUIRE(pi && act && adv && vs && val && state && dlog && dval && ws, "vmpo_loss: null argument");
    TilePlan p{};
    FI_TRY(tile_plan("vmpo_loss", T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)dlog % 16 == 0,
               "vmpo_loss: pi and dlogits must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)act % 4 == 0 && (uintptr_t)adv % 4 == 0 && (uintptr_t)vs % 4 == 0 && (uintptr_t)val % 4 == 0 &&
                   (uintptr_t)dval % 4 == 0 && (uintptr_t)bad % 4 == 0,
               "vmpo_loss: act, adv, vs, val, dvalue and bad must be 4-byte aligned");
    FI_REQUIRE((uintptr_t)losses % 8 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)ws % 16 == 0,
               "vmpo_loss: losses and the state block must be 8-byte, ws 16-byte aligned");
    const Layout lay = layout_of(p);
    FI_REQUIRE(ws_bytes >= lay.total, "vmpo_loss: ws_bytes " + std::to_string(ws_bytes) + " < " + std::to_string(lay.total) +
                                          " = fi_vmpo_workspace_bytes(" + std::to_string(T) + ", " + std::to_string(B) + ", " +
                                          std::to_string(A) + ")");
    const size_t row_bytes = (size_t)kWaves * kCols * (A | 1) * sizeof(float);
    if (row_bytes > 64 * 1024) {  // more than 64 KB of dynamic LDS: A = 63, 64
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)vmpo_loss_kernel, raised, (size_t)kWaves * kCols * 65 * 4));
    }
    char* w = (char*)ws;
    LossArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = p.ct, a.slices = p.slices, a.slice_len = p.slice_len;
    a.nsel = select_blocks((int64_t)T * B);
    a.pi = pi, a.act = act, a.adv = adv, a.vs = vs, a.val = val;
    a.dlog = dlog, a.dval = dval;
    a.sel = (const uint32_t*)(w + lay.sel), a.selpart = (const double*)(w + lay.selpart), a.part = (double*)(w + lay.part);
    a.state = (fi_vmpo_state*)state;
    a.bad = bad ? bad : (int*)(w + lay.bad);
    a.count_bad = count_bad ? 1 : 0;
    a.bc = hp.baseline_cost, a.ec = hp.entropy_cost, a.eps_eta = prm->eps_eta;
    if (!bad) FI_HIP_CHECK(hipMemsetAsync(a.bad, 0, sizeof(int), stream));
    const unsigned nblk = (unsigned)(p.ct * p.slices);
    {
        TagScope s(tg, "vmpo_loss");
        hipLaunchKernelGGL(vmpo_loss_kernel, dim3(nblk), dim3(64 * kWaves), row_bytes, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (losses) {
        hipLaunchKernelGGL(vmpo_losses_kernel, dim3(1), dim3(kStatThreads), 0, stream, (const double*)a.part, (int)nblk,
                           (const int*)a.bad, losses);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (partials) *partials = a.part;
    if (nblk_out) *nblk_out = (int)nblk;
    return FI_OK;
}

int eta_launch(void* state, const fi_vmpo_params* prm, const int* skip, hipStream_t stream) {
    FI_TRY(check_params("vmpo_eta_step", prm));
    FI_REQUIRE(state, "vmpo_eta_step: null state block");
    FI_REQUIRE((uintptr_t)state % 8 == 0, "vmpo_eta_step: the state block must be 8-byte aligned");
    FI_REQUIRE((uintptr_t)skip % 4 == 0, "vmpo_eta_step: skip must be 4-byte aligned");
    hipLaunchKernelGGL(vmpo_eta_kernel, dim3(1), dim3(64), 0, stream, (fi_vmpo_state*)state, *prm, skip);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's block
int block_launch(const VmpoBlock* b, int T, int B, int A, const float* pi, const float* front_pi, const float* mu,
                 const int32_t* act, const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp, float* vs,
                 float* adv, float* dlog, float* dval, int* bad, hipStream_t stream, KernelTagger* tg, const double** partials,
                 int* nblk) {
    SurrogateFront f{};
    FI_TRY(surrogate_front_launch(T, B, A, front_pi, mu, act, rew, disc, val, hp, vs, adv, b->front_ws, b->front_bytes, bad,
                                  stream, tg, &f));
    FI_TRY(select_launch((int64_t)T * B, adv, &b->prm, b->state, b->ws, b->ws_bytes, stream, tg));
    return loss_launch(T, B, A, pi, act, adv, vs, val, hp, &b->prm, b->state, dlog, dval, nullptr, b->ws, b->ws_bytes, bad,
                       false, stream, tg, partials, nblk);
}

int block_eta(const VmpoBlock* b, const int* skip, hipStream_t stream) { return eta_launch(b->state, &b->prm, skip, stream); }

void block_free(void* p) {
    VmpoBlock* b = (VmpoBlock*)p;
    if (!b) return;
    for (void* q : {b->state, b->ws, b->front_ws})
        if (q) (void)hipFree(q);
    delete b;
}

int block_create(const VmpoView& v, float eta_init, VmpoBlock** out) {
    TilePlan p{};
    if (tile_plan("vmpo_enable", v.T, v.B, v.A, &p) != FI_OK)
        return fail(FI_ERR_INVALID,
                    "vmpo_enable: the learner's shape is outside the kernels' (" + std::string(fi_last_error()) + ")");
    VmpoBlock* b = new (std::nothrow) VmpoBlock();
    FI_REQUIRE(b, "vmpo_enable: out of host memory");
    b->launch = block_launch;
    b->eta = block_eta;
    b->ws_bytes = layout_of(p).total;
    b->front_bytes = surrogate_workspace_bytes(v.T, v.B, v.A);
    int rc = dev_alloc(&b->state, sizeof(fi_vmpo_state), "vmpo_enable: state block");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "vmpo_enable: workspace");
    if (rc == FI_OK) rc = dev_alloc(&b->front_ws, b->front_bytes, "vmpo_enable: the targets' workspace");
    if (rc == FI_OK) {
        fi_vmpo_state st{};
        st.eta = (double)eta_init;
        hipError_t e = hipMemcpyAsync(b->state, &st, sizeof(st), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v.stream);  // st is the stack's
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "vmpo_enable: initialising the block failed");
        }
    }
    if (rc != FI_OK) {
        block_free(b);
        return rc;
    }
    *out = b;
    return FI_OK;
}

// the view of a handle whose block exists
int enabled_view(fi_learner* l, const char* who, VmpoView* v) {
    FI_TRY(learner_vmpo_view(l, v));
    if (!v->block)
        return fail(FI_ERR_STATE, std::string(who) + ": the objective was never on on this handle (fi_vmpo_enable first)");
    FI_HIP_CHECK(hipSetDevice(v->dev));
    return FI_OK;
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_vmpo_enable(fi_learner* l, const fi_vmpo_params* params) {
    FI_REQUIRE(l, "vmpo_enable: null learner");
    FI_TRY(check_params("vmpo_enable", params));
    VmpoView v{};
    FI_TRY(learner_vmpo_view(l, &v));
    if (v.nranks > 1)
        return fail(FI_ERR_STATE, "vmpo_enable: the handle is attached to a communicator of " + std::to_string(v.nranks) +
                                      " ranks; the selection is over the whole batch and each rank holds a shard of it");
    VmpoBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("vmpo_enable", FI_ERR_OOM, [&] { return block_create(v, params->eta_init, &b); }));
        learner_set_vmpo_block(l, b, block_free);
    }
    b->prm = *params;  // by value into every later launch; the block's eta is kept
    b->on = true;
    if (v.surrogate) v.surrogate->on = false;  // one objective at a time
    return FI_OK;
}

extern "C" int fi_vmpo_disable(fi_learner* l) {
    FI_REQUIRE(l, "vmpo_disable: null learner");
    VmpoView v{};
    FI_TRY(learner_vmpo_view(l, &v));
    if (v.block) v.block->on = false;
    return FI_OK;
}

extern "C" int fi_vmpo_set_eta(fi_learner* l, double eta) {
    FI_REQUIRE(l, "vmpo_set_eta: null learner");
    FI_TRY(check_eta("vmpo_set_eta", eta));
    VmpoView v{};
    FI_TRY(enabled_view(l, "vmpo_set_eta", &v));
    // behind every enqueued step; the rest of the block is kept
    FI_HIP_CHECK(hipMemcpyAsync(v.block->state, &eta, sizeof(eta), hipMemcpyHostToDevice, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    return FI_OK;
}

extern "C" int fi_vmpo_get_state(fi_learner* l, fi_vmpo_params* params, fi_vmpo_state* state, uint32_t* enabled) {
    FI_REQUIRE(l, "vmpo_get_state: null learner");
    VmpoView v{};
    FI_TRY(learner_vmpo_view(l, &v));
    const VmpoBlock* b = v.block;
    fi_vmpo_state st{};
    if (b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_HIP_CHECK(hipMemcpyAsync(&st, b->state, sizeof(st), hipMemcpyDeviceToHost, v.stream));
        FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    }
    if (params)
        *params = b ? b->prm
                    : fi_vmpo_params{FI_VMPO_TOP_FRACTION, FI_VMPO_EPS_ETA, FI_VMPO_ETA_INIT, FI_VMPO_ETA_MIN, FI_VMPO_LR_ETA, 1u,
                                     {0u, 0u}};
    if (state) *state = st;
    if (enabled) *enabled = b && b->on ? 1u : 0u;
    return FI_OK;
}

extern "C" int fi_vmpo_state_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "vmpo_state_dev: null argument");
    VmpoView v{};
    FI_TRY(enabled_view(l, "vmpo_state_dev", &v));
    *ptr = v.block->state;
    return FI_OK;
}

extern "C" size_t fi_vmpo_workspace_bytes(int T, int B, int A) {
    TilePlan p{};
    return tile_plan("vmpo_workspace_bytes", T, B, A, &p) == FI_OK ? layout_of(p).total : 0;
}

extern "C" int fi_vmpo_select_blocks(int64_t n) { return select_blocks(n); }

extern "C" int fi_vmpo_select_fp32(int64_t n, const float* adv, const fi_vmpo_params* params, void* state_dev, void* ws,
                                   size_t ws_bytes, void* stream) {
    return select_launch(n, adv, params, state_dev, ws, ws_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int fi_vmpo_loss_fp32(int T, int B, int A, const float* pi, const int32_t* act, const float* adv, const float* vs,
                                 const float* val, const fi_vtrace_hparams* hp, const fi_vmpo_params* params, void* state_dev,
                                 float* dlogits, float* dvalue, double* losses, void* ws, size_t ws_bytes, int* bad,
                                 void* stream) {
    FI_REQUIRE(hp, "vmpo_loss: null hparams");
    return loss_launch(T, B, A, pi, act, adv, vs, val, *hp, params, state_dev, dlogits, dvalue, losses, ws, ws_bytes, bad, true,
                       (hipStream_t)stream, nullptr, nullptr, nullptr);
}

extern "C" int fi_vmpo_eta_step(void* state_dev, const fi_vmpo_params* params, const int* skip, void* stream) {
    return eta_launch(state_dev, params, skip, (hipStream_t)stream);
}
