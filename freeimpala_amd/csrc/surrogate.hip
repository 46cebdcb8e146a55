// surrogate.hip -- the clipped surrogate policy loss on V-trace targets (include/fi_surrogate.h, where
// the rule stands): the kernels that take the place of the V-trace launch of a step, and every
// fi_surrogate_* entry point.
//
//   surrogate_rows_kernel   a stream over (t, b), row_stream.h's pattern: workgroup (c, s) owns the 64
//                           columns of tile c and the time steps of slice s, its four waves the steps
//                           t .. t + 3 of a round, lane = column; the pi and mu rows of one (t, tile)
//                           arrive in padded LDS rows (load_run<true>), then one lane per row. Writes
//                           d = rho^ (r + g V' - V), k = g c and log rho per row; counts bad actions.
//   surrogate_scan_kernel   acc_t = d_t + k_t acc_{t+1} down each column, one lane per column, one wave
//                           per workgroup (64 workgroups at B = 4096, spread over the CUs). The five loads
//                           of the next eight time steps are issued before the dependent chain of the
//                           current eight runs. Writes vs, A and one fp64 pair of moment partials.
//   surrogate_loss_kernel   the rows kernel's grid and read pattern over pi alone. Every workgroup adds
//                           the moment partials itself, in one fixed order: no finalize launch stands
//                           between the scan and the loss. dlogits are written over the lane's own pi
//                           row in LDS and leave as the run's 16-byte pieces. The three loss sums and the
//                           clipped count are reduced per wave by DPP / permlane: one partial per workgroup.
//   surrogate_stats_kernel  one workgroup: the clipped counts of all workgroups added in a fixed order
//                           and the 32-byte stats block (a count over the whole grid cannot be written
//                           by workgroup 0 of the loss kernel without an atomic or a grid-wide wait);
//                           for the stand-alone entry also the three loss scalars.
// No float atomics; the bad-action count is an integer atomic, as V-trace's. learner.cpp names nothing
// of this file: fi_surrogate_enable hangs a SurrogateBlock with the launcher on the handle (kernels.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "atari.h"  // KernelTagger, TagScope
#include "fi_common.h"
#include "fi_surrogate.h"
#include "host_util.h"
#include "kernels.h"
#include "policy_row.h"  // pair_log_prob, policy_row_grad, adv_moments: shared with target.hip
#include "row_stream.h"  // kCols, kWaves, load_run, store_run, wave_reduce, block_sums, tile_plan

namespace fi {

namespace {
constexpr int kAhead = 8;  // time steps of the scan whose loads are in flight ahead of the chain

struct StatsBlock {
    uint64_t rows, rows_clipped;
    double adv_mean, adv_std;
};
static_assert(sizeof(StatsBlock) == 32, "fi_surrogate.h fixes the block at 32 bytes");

struct SurArgs {
    int T, B, A;
    int ct, slices, slice_len, nscan;
    const float* __restrict__ pi;
    const float* __restrict__ mu;
    const int32_t* __restrict__ act;
    const float* __restrict__ rew;
    const float* __restrict__ disc;
    const float* __restrict__ val;
    float* vs;
    float* adv;
    float* dlog;
    float* dval;
    float* d;                     // workspace: [T * B] each
    float* k;
    float* lr;
    double* mom;                  // [nscan][2]: sums of A - pivot and of its square
    double* pivot;                // 1
    double* part;                 // [ct * slices][3]
    unsigned long long* clipped;  // [ct * slices]
    int* bad;
    fi_vtrace_hparams hp;
    float clip, adv_eps;
    uint32_t normalize;
};

// m and s of A from the scan's partials (policy_row.h): the loss kernel's workgroups and the stats kernel
// run the same sequence on the same numbers, so they hold the same bits
__device__ __forceinline__ void moments(const SurArgs& a, double* red, double& m, double& s) {
    adv_moments(a.mom, a.pivot, a.nscan, a.T, a.B, red, m, s);
}

}  // namespace

__global__ __launch_bounds__(64 * kWaves) void surrogate_rows_kernel(SurArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * 2 * kCols * S;  // this wave's pi rows, then its mu rows
    float* const lm = lp + kCols * S;
    const uint32_t n = (uint32_t)nb * A;
    int nbad = 0;
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        int at = 0;
        float rw = 0.f, g = 1.f, v = 0.f, vn = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            rw = a.rew[e];
            g = a.disc[e];
            v = a.val[e];
            vn = a.val[e + B];
        }
        if (live) load_run<true>(a.pi, a.mu, lp, lm, ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A, n, A, S, lane);
        __syncthreads();  // the rows are in LDS (a wave reads its own rows only; the round count is uniform)
        if (mine) {
            const float* __restrict__ zp = lp + (uint32_t)lane * S;
            const float* __restrict__ zm = lm + (uint32_t)lane * S;
            if ((unsigned)at >= A) ++nbad;
            const uint32_t ai = at < 0 ? 0u : ((uint32_t)at >= A ? A - 1u : (uint32_t)at);
            const f32x2 la = pair_log_prob(zp, zm, A, ai);  // log pi(a), log mu(a): one instruction sequence for both
            const float lr = la.x - la.y;
            const float rho = __expf(lr);
            const size_t e = (size_t)t * B + b0 + lane;
            a.d[e] = fminf(a.hp.rho_bar, rho) * (rw + g * vn - v);
            a.k[e] = g * (a.hp.lambda_ * fminf(a.hp.c_bar, rho));
            a.lr[e] = lr;
        }
        __syncthreads();  // the rows are read: the next round may overwrite them
    }
    const unsigned long long any = __ballot(nbad != 0);
    if (any) {  // wave-uniform; the rare path
        int tot = nbad;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
        if (lane == 0) atomicAdd(a.bad, tot);
    }
}

// One wave per workgroup, lane = column. cur / nxt: the loads of eight time steps each; the next
// eight are issued before the chain over the current eight, so the chain never waits for a load it
// could have had. Steps below t = 0 load row 0 again and are not used.
__global__ __launch_bounds__(64) void surrogate_scan_kernel(SurArgs a) {
    const int lane = threadIdx.x, b = (int)blockIdx.x * kCols + lane;
    const int T = a.T, B = a.B;
    const bool mine = b < B;
    const int bb = mine ? b : B - 1;
    double pivot;
    {
        const float p = a.rew[0] + a.disc[0] * a.val[B] - a.val[0];
        pivot = fabsf(p) <= 3.0e38f ? (double)p : 0.0;
    }
    if (blockIdx.x == 0 && lane == 0) *a.pivot = pivot;
    struct Step {
        float d, k, r, g, v;
    };
    auto load = [&](int t) {
        const size_t e = (size_t)(t < 0 ? 0 : t) * B + bb;
        return Step{a.d[e], a.k[e], a.rew[e], a.disc[e], a.val[e]};
    };
    Step cur[kAhead], nxt[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) cur[j] = load(T - 1 - j);
    float acc = 0.f, vs_next = a.val[(size_t)T * B + bb];
    double s1 = 0.0, s2 = 0.0;
    for (int t1 = T - 1; t1 >= 0; t1 -= kAhead) {
#pragma unroll
        for (int j = 0; j < kAhead; ++j) nxt[j] = load(t1 - kAhead - j);
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int t = t1 - j;
            if (t >= 0) {  // uniform
                const Step x = cur[j];
                acc = x.d + x.k * acc;
                const float vs = x.v + acc;
                const float adv = x.r + x.g * vs_next - x.v;
                vs_next = vs;
                if (mine) {
                    const size_t e = (size_t)t * B + b;
                    a.vs[e] = vs;
                    a.adv[e] = adv;
                    const double q = (double)adv - pivot;
                    s1 += q;
                    s2 += q * q;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kAhead; ++j) cur[j] = nxt[j];
    }
    s1 = wave_reduce(s1, lane);
    s2 = wave_reduce(s2, lane);
    if (lane == 0) {
        a.mom[2 * (size_t)blockIdx.x] = s1;
        a.mom[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

__global__ __launch_bounds__(64 * kWaves) void surrogate_loss_kernel(SurArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    __shared__ double red[kWaves * 4];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * kCols * S;  // this wave's pi rows, dlogits after the arithmetic
    const uint32_t n = (uint32_t)nb * A;
    double m = 0.0, sd = 1.0;
    if (a.normalize) moments(a, red, m, sd);  // uniform over the grid
    const double den = sd + (double)a.adv_eps;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    const float bc = a.hp.baseline_cost, ec = a.hp.entropy_cost;
    if (s == 0 && tid < nb) a.dval[(size_t)T * B + b0 + tid] = 0.f;  // the bootstrap row has no gradient
    double sum[4] = {0.0, 0.0, 0.0, 0.0};  // L_pg, baseline, entropy, clipped rows
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        const uint32_t g0 = ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A;
        int at = 0;
        float lr = 0.f, adv = 0.f, v = 0.f, vs = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            lr = a.lr[e];
            adv = a.adv[e];
            v = a.val[e];
            vs = a.vs[e];
        }
        if (live) load_run<false>(a.pi, nullptr, lp, nullptr, g0, n, A, S, lane);
        __syncthreads();  // the rows are in LDS
        if (mine) {
            float* __restrict__ z = lp + (uint32_t)lane * S;
            const uint32_t ai = at < 0 ? 0u : ((uint32_t)at >= A ? A - 1u : (uint32_t)at);
            const float rho = __expf(lr);
            const float an = a.normalize ? (float)(((double)adv - m) / den) : adv;
            const bool clipped = (an > 0.f && rho > hi) || (an < 0.f && rho < lo);
            const float rc = fminf(fmaxf(rho, lo), hi);
            const float g = clipped ? 0.f : -rho * an;
            const float plogp = policy_row_grad(z, A, ai, g, ec);  // sum pi log pi; z holds dlogits now
            const float td = v - vs;
            a.dval[(size_t)t * B + b0 + lane] = bc * td;
            sum[0] += (double)(-fminf(rho * an, rc * an));
            sum[1] += 0.5 * (double)td * (double)td;
            sum[2] += (double)plogp;
            sum[3] += clipped ? 1.0 : 0.0;
        }
        __syncthreads();  // the dlogits rows are complete
        if (live) store_run(a.dlog, lp, g0, n, A, S, lane);
        __syncthreads();  // the rows have left: the next round may overwrite them
    }
    block_sums<4, kWaves>(sum, red);
    if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = sum[tid];
    if (tid == 3) a.clipped[blockIdx.x] = (unsigned long long)sum[3];
}

// One workgroup: the stats block (nullable) and, for the stand-alone entry, the loss scalars (nullable;
// NaN when an action was outside [0, A): that entry has no synchronous status to return).
__global__ __launch_bounds__(kStatThreads) void surrogate_stats_kernel(SurArgs a, void* stats, double* losses) {
    __shared__ double red[kWaves * 4];
    double m, sd;
    moments(a, red, m, sd);
    const int nblk = a.ct * a.slices;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += kStatThreads) {
        v[0] += a.part[(size_t)i * 3];
        v[1] += a.part[(size_t)i * 3 + 1];
        v[2] += a.part[(size_t)i * 3 + 2];
        v[3] += (double)a.clipped[i];
    }
    block_sums<4, kWaves>(v, red);
    if (threadIdx.x != 0) return;
    if (stats) {
        StatsBlock* o = (StatsBlock*)stats;
        o->rows = (uint64_t)a.T * (uint64_t)a.B;
        o->rows_clipped = (uint64_t)v[3];
        o->adv_mean = m;
        o->adv_std = sd;
    }
    if (losses) {
        const bool poisoned = *a.bad != 0;
        for (int i = 0; i < 3; ++i) losses[i] = poisoned ? __builtin_nan("") : v[i];
    }
}

// ------------------------------------------------------------------ the launcher
namespace {
size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: d | k | log rho (T * B floats each) | moment partials | pivot | loss partials | clipped
// counts | the stand-alone entry's bad-action counter; every part on a 256-byte boundary
struct Layout {
    size_t row, mom, pivot, part, clipped, bad, total;
};
Layout layout_of(int T, int B, const TilePlan& p) {
    Layout l{};
    const size_t nblk = (size_t)p.ct * p.slices;
    l.row = pad256((size_t)T * B * sizeof(float));
    l.mom = 3 * l.row;
    l.pivot = l.mom + pad256((size_t)p.ct * 2 * sizeof(double));
    l.part = l.pivot + 256;
    l.clipped = l.part + pad256(nblk * 3 * sizeof(double));
    l.bad = l.clipped + pad256(nblk * sizeof(unsigned long long));
    l.total = l.bad + 256;
    return l;
}

}  // namespace

int surrogate_check_params(const std::string& who, const fi_surrogate_params* p) {
    FI_REQUIRE(p, who + ": null params");
    FI_REQUIRE(std::isfinite(p->clip) && p->clip > 0.f, who + ": clip " + std::to_string(p->clip) + " must be finite and > 0");
    FI_REQUIRE(std::isfinite(p->adv_eps) && p->adv_eps >= 0.f,
               who + ": adv_eps " + std::to_string(p->adv_eps) + " must be finite and >= 0");
    FI_REQUIRE(p->normalize <= 1u, who + ": normalize " + std::to_string(p->normalize) + " is neither 0 nor 1");
    return FI_OK;
}

size_t surrogate_workspace_bytes(int T, int B, int A) {
    TilePlan p{};
    return tile_plan("surrogate", T, B, A, &p) == FI_OK ? layout_of(T, B, p).total : 0;
}

int surrogate_loss_blocks(int T, int B, int A) {
    TilePlan p{};
    return tile_plan("surrogate", T, B, A, &p) == FI_OK ? p.ct * p.slices : 0;
}

namespace {
// What surrogate_launch and surrogate_front_launch share. prepare: every check, in one order and with one
// set of messages, and the kernels' arguments over ws; nothing is enqueued and no attribute changed.
// The front passes nullptr for dlog, dval, losses and stats, which it does not have.
int prepare(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew, const float* disc,
            const float* val, const fi_vtrace_hparams& hp, float* vs, float* adv, float* dlog, float* dval,
            const double* losses, const void* stats, void* ws, size_t ws_bytes, int* bad, SurArgs* out) {
    TilePlan p{};
    FI_TRY(tile_plan("surrogate", T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)mu % 16 == 0 && (uintptr_t)dlog % 16 == 0,
               "surrogate: pi, mu and dlogits must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)act % 4 == 0 && (uintptr_t)rew % 4 == 0 && (uintptr_t)disc % 4 == 0 && (uintptr_t)val % 4 == 0 &&
                   (uintptr_t)vs % 4 == 0 && (uintptr_t)adv % 4 == 0 && (uintptr_t)dval % 4 == 0 && (uintptr_t)bad % 4 == 0,
               "surrogate: act, rew, disc, val, vs, adv, dvalue and bad must be 4-byte aligned");
    FI_REQUIRE((uintptr_t)losses % 8 == 0 && (uintptr_t)stats % 8 == 0 && (uintptr_t)ws % 8 == 0,
               "surrogate: losses, stats_dev and ws must be 8-byte aligned");
    const Layout lay = layout_of(T, B, p);
    FI_REQUIRE(ws_bytes >= lay.total, "surrogate: ws_bytes " + std::to_string(ws_bytes) + " < " + std::to_string(lay.total) +
                                          " = fi_surrogate_workspace_bytes(" + std::to_string(T) + ", " + std::to_string(B) +
                                          ", " + std::to_string(A) + ")");
    char* w = (char*)ws;
    SurArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = p.ct, a.slices = p.slices, a.slice_len = p.slice_len, a.nscan = p.ct;  // the scan: a workgroup per column tile
    a.pi = pi, a.mu = mu, a.act = act, a.rew = rew, a.disc = disc, a.val = val;
    a.vs = vs, a.adv = adv, a.dlog = dlog, a.dval = dval;
    a.d = (float*)w, a.k = (float*)(w + lay.row), a.lr = (float*)(w + 2 * lay.row);
    a.mom = (double*)(w + lay.mom), a.pivot = (double*)(w + lay.pivot), a.part = (double*)(w + lay.part);
    a.clipped = (unsigned long long*)(w + lay.clipped);
    a.bad = bad ? bad : (int*)(w + lay.bad);  // stand-alone: count into the workspace
    a.hp = hp;
    *out = a;
    return FI_OK;
}

size_t row_bytes_of(int A) { return (size_t)kWaves * kCols * (A | 1) * sizeof(float); }
constexpr size_t kRowMost = (size_t)kWaves * kCols * 65 * 4;

// the rows and scan kernels on prepared arguments; own_bad: the counter inside ws is zeroed first
int launch_front(const SurArgs& a, bool own_bad, hipStream_t stream, KernelTagger* tg) {
    if (own_bad) FI_HIP_CHECK(hipMemsetAsync(a.bad, 0, sizeof(int), stream));
    const size_t row_bytes = row_bytes_of(a.A);
    if (2 * row_bytes > 64 * 1024) {  // more than 64 KB of dynamic LDS: A > 30
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)surrogate_rows_kernel, raised, 2 * kRowMost));
    }
    {
        TagScope t(tg, "surrogate_rows");
        hipLaunchKernelGGL(surrogate_rows_kernel, dim3((unsigned)(a.ct * a.slices)), dim3(64 * kWaves), 2 * row_bytes, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope t(tg, "surrogate_scan");
        hipLaunchKernelGGL(surrogate_scan_kernel, dim3((unsigned)a.nscan), dim3(64), 0, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    return FI_OK;
}
}  // namespace

int surrogate_front_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                           const float* disc, const float* val, const fi_vtrace_hparams& hp, float* vs, float* adv, void* ws,
                           size_t ws_bytes, int* bad, hipStream_t stream, KernelTagger* tg, SurrogateFront* out) {
    FI_REQUIRE(pi && mu && act && rew && disc && val && vs && adv && ws && out, "surrogate: null argument");
    SurArgs a{};
    FI_TRY(prepare(T, B, A, pi, mu, act, rew, disc, val, hp, vs, adv, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, bad,
                   &a));
    FI_TRY(launch_front(a, !bad, stream, tg));
    *out = SurrogateFront{a.lr, a.mom, a.pivot, a.bad, a.nscan, a.ct, a.slices, a.slice_len};
    return FI_OK;
}

int surrogate_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                     const float* disc, const float* val, const fi_vtrace_hparams& hp, const fi_surrogate_params& prm,
                     float* vs, float* adv, float* dlog, float* dval, double* losses, void* stats, void* ws, size_t ws_bytes,
                     int* bad, hipStream_t stream, KernelTagger* tg, const double** partials, int* nblk_out) {
    FI_REQUIRE(pi && mu && act && rew && disc && val && vs && adv && dlog && dval && ws, "surrogate: null argument");
    SurArgs a{};
    FI_TRY(prepare(T, B, A, pi, mu, act, rew, disc, val, hp, vs, adv, dlog, dval, losses, stats, ws, ws_bytes, bad, &a));
    a.clip = prm.clip, a.adv_eps = prm.adv_eps, a.normalize = prm.normalize;
    const size_t row_bytes = row_bytes_of(A);
    if (row_bytes > 64 * 1024) {  // more than 64 KB of dynamic LDS: A = 63, 64
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)surrogate_loss_kernel, raised, kRowMost));
    }
    FI_TRY(launch_front(a, !bad, stream, tg));
    const unsigned nblk = (unsigned)(a.ct * a.slices);
    {
        TagScope t(tg, "surrogate_loss");
        hipLaunchKernelGGL(surrogate_loss_kernel, dim3(nblk), dim3(64 * kWaves), row_bytes, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (stats || losses) {
        TagScope t(tg, "surrogate_stats");
        hipLaunchKernelGGL(surrogate_stats_kernel, dim3(1), dim3(kStatThreads), 0, stream, a, stats, losses);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (partials) *partials = a.part;
    if (nblk_out) *nblk_out = (int)nblk;
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's block
namespace {
int block_launch(const SurrogateBlock* b, int T, int B, int A, const float* pi, const float* mu, const int32_t* act,
                 const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp, float* vs, float* adv,
                 float* dlog, float* dval, int* bad, hipStream_t stream, KernelTagger* tg, const double** partials,
                 int* nblk) {
    const fi_surrogate_params prm{b->clip, b->normalize, b->adv_eps, 0u};
    return surrogate_launch(T, B, A, pi, mu, act, rew, disc, val, hp, prm, vs, adv, dlog, dval, nullptr, b->stats, b->ws,
                            b->ws_bytes, bad, stream, tg, partials, nblk);
}

void block_free(void* p) {
    SurrogateBlock* b = (SurrogateBlock*)p;
    if (!b) return;
    if (b->stats) (void)hipFree(b->stats);
    if (b->ws) (void)hipFree(b->ws);
    delete b;
}

int block_create(const SurrogateView& v, SurrogateBlock** out) {
    SurrogateBlock* b = new (std::nothrow) SurrogateBlock();
    FI_REQUIRE(b, "surrogate_enable: out of host memory");
    b->launch = block_launch;
    b->ws_bytes = surrogate_workspace_bytes(v.T, v.B, v.A);
    int rc = b->ws_bytes ? FI_OK : fail(FI_ERR_INVALID, "surrogate_enable: the learner's shape is outside the kernels' (" +
                                                            std::string(fi_last_error()) + ")");
    if (rc == FI_OK) rc = dev_alloc(&b->stats, sizeof(StatsBlock), "surrogate_enable: stats block");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "surrogate_enable: workspace");
    if (rc == FI_OK) {
        const hipError_t e = hipMemsetAsync(b->stats, 0, sizeof(StatsBlock), v.stream);
        if (e != hipSuccess || hipStreamSynchronize(v.stream) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "surrogate_enable: clearing the stats block failed");
        }
    }
    if (rc != FI_OK) {
        block_free(b);
        return rc;
    }
    *out = b;
    return FI_OK;
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_surrogate_enable(fi_learner* l, const fi_surrogate_params* params) {
    FI_REQUIRE(l, "surrogate_enable: null learner");
    FI_TRY(surrogate_check_params("surrogate_enable", params));
    SurrogateView v{};
    FI_TRY(learner_surrogate_view(l, &v));
    if (params->normalize && v.nranks > 1)
        return fail(FI_ERR_STATE, "surrogate_enable: the handle is attached to a communicator of " + std::to_string(v.nranks) +
                                      " ranks; the advantage moments of a normalising step would need an all-reduce");
    SurrogateBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("surrogate_enable", FI_ERR_OOM, [&] { return block_create(v, &b); }));
        learner_set_surrogate_block(l, b, block_free);
    }
    b->clip = params->clip;  // by value into every later launch
    b->normalize = params->normalize;
    b->adv_eps = params->adv_eps;
    b->on = true;
    return FI_OK;
}

extern "C" int fi_surrogate_disable(fi_learner* l) {
    FI_REQUIRE(l, "surrogate_disable: null learner");
    SurrogateView v{};
    FI_TRY(learner_surrogate_view(l, &v));
    if (v.block) v.block->on = false;
    return FI_OK;
}

extern "C" int fi_surrogate_get_state(fi_learner* l, fi_surrogate_state* out) {
    FI_REQUIRE(l && out, "surrogate_get_state: null argument");
    SurrogateView v{};
    FI_TRY(learner_surrogate_view(l, &v));
    std::memset(out, 0, sizeof(*out));
    out->clip = FI_SURROGATE_CLIP;
    out->adv_eps = FI_SURROGATE_ADV_EPS;
    const SurrogateBlock* b = v.block;
    if (!b) return FI_OK;
    StatsBlock st{};
    FI_HIP_CHECK(hipSetDevice(v.dev));
    FI_HIP_CHECK(hipMemcpyAsync(&st, b->stats, sizeof(st), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    out->enabled = b->on ? 1u : 0u;
    out->normalize = b->normalize;
    out->clip = b->clip;
    out->adv_eps = b->adv_eps;
    out->rows = st.rows;
    out->rows_clipped = st.rows_clipped;
    out->adv_mean = st.adv_mean;
    out->adv_std = st.adv_std;
    return FI_OK;
}

extern "C" int fi_surrogate_stats_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "surrogate_stats_dev: null argument");
    SurrogateView v{};
    FI_TRY(learner_surrogate_view(l, &v));
    if (!v.block)
        return fail(FI_ERR_STATE, "surrogate_stats_dev: the objective was never on on this handle (fi_surrogate_enable first)");
    *ptr = v.block->stats;
    return FI_OK;
}

extern "C" size_t fi_surrogate_workspace_bytes(int T, int B, int A) { return surrogate_workspace_bytes(T, B, A); }
extern "C" int fi_surrogate_loss_blocks(int T, int B, int A) { return surrogate_loss_blocks(T, B, A); }

extern "C" int fi_surrogate_loss_fp32(int T, int B, int A, const float* pi, const float* mu, const int32_t* act,
                                      const float* rew, const float* disc, const float* val, const fi_vtrace_hparams* hp,
                                      const fi_surrogate_params* params, float* vs, float* adv, float* dlogits, float* dvalue,
                                      double* losses, void* stats_dev, void* ws, size_t ws_bytes, int* bad, void* stream) {
    FI_REQUIRE(hp, "surrogate_loss: null hparams");
    FI_TRY(surrogate_check_params("surrogate_loss", params));
    return surrogate_launch(T, B, A, pi, mu, act, rew, disc, val, *hp, *params, vs, adv, dlogits, dvalue, losses, stats_dev,
                            ws, ws_bytes, bad, (hipStream_t)stream, nullptr, nullptr, nullptr);
}
