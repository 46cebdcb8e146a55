// diag.hip -- off-policy diagnostics of a learner step behind the C ABI of include/fi_diag.h (where
// the rule stands): rho statistics, KL(mu | pi), entropies, effective sample size, clip rates and the
// value head's explained variance, reduced on the device from the tensors a step leaves there. It
// runs beside the step, never inside it: learner.cpp names nothing of this file (kernels.h).
//
//   * offpolicy_diag_kernel: a pure read stream, (8 A + 24) bytes per (t, b), in row_stream.h's
//     pattern: workgroup (c, s) owns the 64 columns [64 c, 64 c + 64) and the time steps of slice s;
//     its four waves take the time steps t, t + 1, t + 2, t + 3 of a round, lane = column. The pi and
//     mu rows of one (t, tile) arrive in the wave's padded LDS rows (load_run<true>); then every lane
//     computes its own row out of LDS.
//     act / rew / disc / val / vs: 4 bytes per lane, 256 contiguous bytes per wave and tensor.
//     Per-row arithmetic is fp32 with vtrace.hip's intrinsics (v_exp_f32, v_log_f32), the pi and the
//     mu side as the two lanes of one 2-vector, so both get the same instruction sequence. Every
//     lane keeps its sums over its time steps in fp64; the four waves combine through LDS: the
//     per-column sums (used rows, kl, lr) need no atomics, the other sums are reduced over the wave
//     by DPP and permlane moves first. Every partial goes to the caller's workspace; nothing is zeroed beforehand.
//   * offpolicy_diag_finalize_kernel: one workgroup adds the partials in a fixed order in fp64,
//     derives the means, ESS and explained variance and writes the struct and the two column arrays.
// No float atomics, no HIP graphs, no global mutable state but the per-device flag of the LDS limit.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "fi_common.h"
#include "fi_diag.h"
#include "host_util.h"
#include "kernels.h"
#include "row_stream.h"  // kCols, kWaves, load_run, wave_reduce, combine, tile_plan

namespace fi {

namespace {
constexpr int kFinalThreads = 1024;

// the sums a workgroup hands on beside its per-column ones
enum {
    S_BAD_ACTION, S_NONFINITE, S_RHO_CLIP, S_C_CLIP, S_PG_CLIP, S_EPISODE_ENDS,
    S_RHO, S_RHO2, S_HPI, S_HMU, S_ABS_TD, S_REW, S_TD, S_TD2, S_VS, S_VS2,
    S_SUMS,               // the entries above are added; the two below are extremes
    S_MAX_RHO = S_SUMS, S_MIN_RHO, S_COUNT
};
enum { C_USED, C_KL, C_LR, C_COUNT };  // per column

struct DiagArgs {
    int T, B, A;
    int ct, slices, slice_len, bpad;  // bpad = ct * kCols
    const float* __restrict__ pi;
    const float* __restrict__ mu;
    const int32_t* __restrict__ act;
    const float* __restrict__ rew;
    const float* __restrict__ disc;
    const float* __restrict__ val;
    const float* __restrict__ vs;
    double* scal;  // [ct * slices][S_COUNT]
    double* colp;  // [C_COUNT][slices][bpad]
    float rho_bar, c_bar, pg_rho_bar;
};

// how entry i of a workgroup's sums (S_*) combines: added, or an extreme (row_stream.h's operators)
__device__ __forceinline__ constexpr int op_of(int i) { return i < S_SUMS ? OP_SUM : (i == S_MAX_RHO ? OP_MAX : OP_MIN); }
// row_stream.h's wave reduction for an operator that an unrolled loop's index decides: op is a constant
// at every call, so one of the three is left
__device__ __forceinline__ double wave_reduce_op(int op, double v, int lane) {
    return op == OP_SUM ? wave_reduce<OP_SUM>(v, lane) : (op == OP_MAX ? wave_reduce<OP_MAX>(v, lane) : wave_reduce<OP_MIN>(v, lane));
}

// the var(vs) sums run on vs - pivot: a variance does not depend on the shift, a constant vs gives
// exactly 0 and nothing cancels for a vs far from 0
__device__ __forceinline__ float vs_pivot(const float* vs) {
    const float p = vs[0];
    return fabsf(p) <= 3.0e38f ? p : 0.f;
}
}  // namespace

__global__ __launch_bounds__(64 * kWaves) void offpolicy_diag_kernel(DiagArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)dsm + (size_t)w * 2 * kCols * S;  // this wave's pi rows, then its mu rows
    float* const lm = lp + kCols * S;
    const uint32_t n = (uint32_t)nb * A;  // floats of a run
    const float pivot = vs_pivot(a.vs);

    double col[C_COUNT] = {0.0, 0.0, 0.0};
    double acc[S_COUNT];
#pragma unroll
    for (int i = 0; i < S_SUMS; ++i) acc[i] = 0.0;
    acc[S_MAX_RHO] = -INFINITY;
    acc[S_MIN_RHO] = INFINITY;

    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        int at = 0;
        float rw = 0.f, g = 1.f, v = 0.f, vt = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            rw = a.rew[e];
            g = a.disc[e];
            v = a.val[e];
            vt = a.vs[e];
        }
        if (live) load_run<true>(a.pi, a.mu, lp, lm, ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A, n, A, S, lane);
        __syncthreads();  // the rows are in LDS (a wave reads its own rows only; the round count is uniform)
        if (mine) {
            const float* __restrict__ zp = lp + (uint32_t)lane * S;
            const float* __restrict__ zm = lm + (uint32_t)lane * S;
            const bool act_ok = (unsigned)at < A;
            const uint32_t ai = act_ok ? (uint32_t)at : 0u;
            // x = {pi side, mu side}: one instruction sequence for both
            f32x2 mx = {zp[0], zm[0]}, nf = {0.f, 0.f};
            for (uint32_t i = 0; i < A; ++i) {
                const f32x2 z = {zp[i], zm[i]};
                mx = __builtin_elementwise_max(mx, z);
                nf += z * 0.f;  // NaN once a logit is NaN or Inf
            }
            const bool finite = nf.x == 0.f && nf.y == 0.f;
            f32x2 se = {0.f, 0.f}, sd = {0.f, 0.f};
            float skd = 0.f;
            for (uint32_t i = 0; i < A; ++i) {
                const f32x2 z = {zp[i], zm[i]};
                const f32x2 d = z - mx, x = d * L2E;
                const f32x2 e = {__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
                se += e;
                sd += e * d;
                skd += e.y * (d.y - d.x);
            }
            const f32x2 lg = f32x2{__builtin_amdgcn_logf(se.x), __builtin_amdgcn_logf(se.y)} * LN2;  // log sum e
            const f32x2 ent = lg - sd / se;                                                          // H = log Z - E[d]
            const f32x2 za = {zp[ai], zm[ai]};
            const f32x2 la = (za - mx) - lg;  // log pi(a), log mu(a)
            const float lr = la.x - la.y;
            const float rho = __expf(lr);
            // log mu_a - log pi_a = (d_mu - d_pi) + (lg_pi - lg_mu): both terms are exactly 0 for bit-equal rows
            const float kl = skd / se.y + (lg.x - lg.y);
            const float td = vt - v;
            const bool used = act_ok && finite;
            acc[S_BAD_ACTION] += act_ok ? 0.0 : 1.0;
            acc[S_NONFINITE] += (act_ok && !finite) ? 1.0 : 0.0;
            acc[S_EPISODE_ENDS] += g == 0.f ? 1.0 : 0.0;
            if (used) {
                col[C_USED] += 1.0;
                col[C_KL] += (double)kl;
                col[C_LR] += (double)lr;
                acc[S_RHO_CLIP] += rho > a.rho_bar ? 1.0 : 0.0;
                acc[S_C_CLIP] += rho > a.c_bar ? 1.0 : 0.0;
                acc[S_PG_CLIP] += rho > a.pg_rho_bar ? 1.0 : 0.0;
                acc[S_RHO] += (double)rho;
                acc[S_RHO2] += (double)rho * (double)rho;
                acc[S_HPI] += (double)ent.x;
                acc[S_HMU] += (double)ent.y;
                acc[S_ABS_TD] += (double)fabsf(td);
                acc[S_REW] += (double)rw;
                acc[S_TD] += (double)td;
                acc[S_TD2] += (double)td * (double)td;
                const double q = (double)vt - (double)pivot;
                acc[S_VS] += q;
                acc[S_VS2] += q * q;
                acc[S_MAX_RHO] = fmax(acc[S_MAX_RHO], (double)rho);
                acc[S_MIN_RHO] = fmin(acc[S_MIN_RHO], (double)rho);
            }
        }
        __syncthreads();  // the rows are read: the next round may overwrite them
    }

    // the four waves' sums through LDS, in a fixed order: first the per-column ones, lane = column (no
    // wave reduction, so not block_sums)
    double* const red = (double*)dsm;
#pragma unroll
    for (int k = 0; k < C_COUNT; ++k) red[(w * C_COUNT + k) * kCols + lane] = col[k];
    __syncthreads();
    if (tid < C_COUNT * kCols) {
        const int k = tid >> 6, ln = tid & 63;
        double sum = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < kWaves; ++w2) sum += red[(w2 * C_COUNT + k) * kCols + ln];
        a.colp[((size_t)k * a.slices + s) * a.bpad + b0 + ln] = sum;  // columns >= B of the last tile: 0
    }
    __syncthreads();
    // the other sums: over the wave, then thread i combines quantity i over the waves. Not block_sums:
    // two entries are extremes, and only the S_COUNT threads that write a partial read red
#pragma unroll
    for (int i = 0; i < S_COUNT; ++i) {
        const double x = wave_reduce_op(op_of(i), acc[i], lane);
        if (lane == 0) red[w * S_COUNT + i] = x;
    }
    __syncthreads();
    if (tid < S_COUNT) {
        double x = red[tid];
#pragma unroll
        for (int w2 = 1; w2 < kWaves; ++w2) {
            x = combine(op_of(tid), x, red[w2 * S_COUNT + tid]);
        }
        a.scal[(size_t)blockIdx.x * S_COUNT + tid] = x;
    }
}

// One workgroup. Thread i adds the slices of the columns i, i + 1024, ... in ascending order (and
// writes their means) and the workgroups i, i + 1024, ...; then the threads' sums are combined over
// the wave (wave_reduce) and over the 16 waves through LDS: a fixed order, so the same partials give
// the same bits. The column partials are the bulk (24 bytes per column and slice, 0.9 MB at
// T = 100, B = 4096) and one CU reads them: eight slices of a column, 24 loads, are in flight per
// thread before the first is added.
__global__ __launch_bounds__(kFinalThreads) void offpolicy_diag_finalize_kernel(DiagArgs a, fi_offpolicy_diag* out,
                                                                                float* col_kl, float* col_log_rho) {
    constexpr int NV = C_COUNT + S_COUNT, NWV = kFinalThreads / 64, kInFlight = 8;
    __shared__ double red[NWV * NV];
    __shared__ double t[NV];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    v[C_COUNT + S_MAX_RHO] = -INFINITY;
    v[C_COUNT + S_MIN_RHO] = INFINITY;
    const size_t plane = (size_t)a.slices * a.bpad;
    for (int b = tid; b < a.B; b += kFinalThreads) {
        double cs[C_COUNT] = {0.0, 0.0, 0.0};
        for (int s0 = 0; s0 < a.slices; s0 += kInFlight) {
            double x[kInFlight][C_COUNT];
#pragma unroll
            for (int j = 0; j < kInFlight; ++j)
#pragma unroll
                for (int k = 0; k < C_COUNT; ++k)
                    x[j][k] = s0 + j < a.slices ? a.colp[k * plane + (size_t)(s0 + j) * a.bpad + b] : 0.0;
#pragma unroll
            for (int j = 0; j < kInFlight; ++j)
#pragma unroll
                for (int k = 0; k < C_COUNT; ++k) cs[k] += x[j][k];
        }
        const float nanf_ = __uint_as_float(0x7fc00000u);
        if (col_kl) col_kl[b] = cs[C_USED] > 0.0 ? (float)(cs[C_KL] / cs[C_USED]) : nanf_;
        if (col_log_rho) col_log_rho[b] = cs[C_USED] > 0.0 ? (float)(cs[C_LR] / cs[C_USED]) : nanf_;
#pragma unroll
        for (int k = 0; k < C_COUNT; ++k) v[k] += cs[k];
    }
    const int nwg = a.ct * a.slices;
    for (int i = tid; i < nwg; i += kFinalThreads) {
        const double* p = a.scal + (size_t)i * S_COUNT;
#pragma unroll
        for (int j = 0; j < S_SUMS; ++j) v[C_COUNT + j] += p[j];
        v[C_COUNT + S_MAX_RHO] = fmax(v[C_COUNT + S_MAX_RHO], p[S_MAX_RHO]);
        v[C_COUNT + S_MIN_RHO] = fmin(v[C_COUNT + S_MIN_RHO], p[S_MIN_RHO]);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double x = wave_reduce_op(i < C_COUNT ? OP_SUM : op_of(i - C_COUNT), v[i], lane);
        if (lane == 0) red[w * NV + i] = x;
    }
    __syncthreads();
    if (tid < NV) {  // quantity tid over the waves, ascending (not block_sums, as in the kernel above)
        double x = red[tid];
        for (int w2 = 1; w2 < NWV; ++w2) {
            x = combine(tid < C_COUNT ? OP_SUM : op_of(tid - C_COUNT), x, red[w2 * NV + tid]);
        }
        t[tid] = x;
    }
    __syncthreads();
    if (tid != 0) return;
#define SC(i) t[C_COUNT + (i)]
    const double n = t[C_USED];
    fi_offpolicy_diag o;
    o.struct_size = (uint32_t)sizeof(fi_offpolicy_diag);
    o.reserved = 0u;
    o.rows = (uint64_t)a.T * (uint64_t)a.B;
    o.rows_used = (uint64_t)n;
    o.rows_bad_action = (uint64_t)SC(S_BAD_ACTION);
    o.rows_nonfinite = (uint64_t)SC(S_NONFINITE);
    o.n_rho_clipped = (uint64_t)SC(S_RHO_CLIP);
    o.n_c_clipped = (uint64_t)SC(S_C_CLIP);
    o.n_pg_clipped = (uint64_t)SC(S_PG_CLIP);
    o.n_episode_ends = (uint64_t)SC(S_EPISODE_ENDS);
    const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
    if (n > 0.0) {
        o.mean_log_rho = t[C_LR] / n;
        o.mean_rho = SC(S_RHO) / n;
        o.kl_mu_pi = t[C_KL] / n;
        o.entropy_pi = SC(S_HPI) / n;
        o.entropy_mu = SC(S_HMU) / n;
        o.mean_abs_td = SC(S_ABS_TD) / n;
        o.mean_reward = SC(S_REW) / n;
        o.max_rho = SC(S_MAX_RHO);
        o.min_rho = SC(S_MIN_RHO);
        o.ess = SC(S_RHO) * SC(S_RHO) / (n * SC(S_RHO2));
        const double m_td = SC(S_TD) / n, m_vs = SC(S_VS) / n;
        const double var_td = SC(S_TD2) / n - m_td * m_td, var_vs = SC(S_VS2) / n - m_vs * m_vs;
        o.explained_variance = var_vs > 0.0 ? 1.0 - var_td / var_vs : nan_;
    } else {
        o.mean_log_rho = o.mean_rho = o.kl_mu_pi = o.entropy_pi = o.entropy_mu = o.mean_abs_td = o.mean_reward = nan_;
        o.max_rho = o.min_rho = o.ess = o.explained_variance = nan_;
    }
    *out = o;
#undef SC
}

// ------------------------------------------------------------------ the launcher
int diag_plan(int T, int B, int A, DiagPlan* out) {
    TilePlan p{};
    FI_TRY(tile_plan("offpolicy_diag", T, B, A, &p));
    *out = DiagPlan{p.ct, p.slices, p.slice_len};
    return FI_OK;
}

static size_t workspace_bytes(const DiagPlan& p) {
    const size_t nwg = (size_t)p.column_tiles * p.time_slices;
    return 8 * (nwg * S_COUNT + (size_t)C_COUNT * p.time_slices * p.column_tiles * kCols);
}

size_t diag_workspace_bytes(int T, int B, int A) {
    DiagPlan p{};
    return diag_plan(T, B, A, &p) == FI_OK ? workspace_bytes(p) : 0;
}

int offpolicy_diag_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                          const float* disc, const float* val, const float* vs, const fi_vtrace_hparams& hp,
                          fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, void* ws, size_t ws_bytes,
                          hipStream_t stream) {
    FI_REQUIRE(pi && mu && act && rew && disc && val && vs && out && ws, "offpolicy_diag: null argument");
    DiagPlan p{};
    FI_TRY(diag_plan(T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)mu % 16 == 0,
               "offpolicy_diag: pi and mu must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)act % 4 == 0 && (uintptr_t)rew % 4 == 0 && (uintptr_t)disc % 4 == 0 && (uintptr_t)val % 4 == 0 &&
                   (uintptr_t)vs % 4 == 0 && (uintptr_t)col_kl % 4 == 0 && (uintptr_t)col_log_rho % 4 == 0,
               "offpolicy_diag: act, rew, disc, val, vs and the column arrays must be 4-byte aligned");
    FI_REQUIRE((uintptr_t)out % 8 == 0 && (uintptr_t)ws % 8 == 0, "offpolicy_diag: out and ws must be 8-byte aligned");
    const size_t need = workspace_bytes(p);
    FI_REQUIRE(ws_bytes >= need, "offpolicy_diag: ws_bytes " + std::to_string(ws_bytes) + " < " + std::to_string(need) +
                                     " = fi_diag_workspace_bytes(" + std::to_string(T) + ", " + std::to_string(B) + ", " +
                                     std::to_string(A) + ")");
    DiagArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = p.column_tiles, a.slices = p.time_slices, a.slice_len = p.slice_len, a.bpad = p.column_tiles * kCols;
    a.pi = pi, a.mu = mu, a.act = act, a.rew = rew, a.disc = disc, a.val = val, a.vs = vs;
    a.scal = (double*)ws;
    a.colp = a.scal + (size_t)a.ct * a.slices * S_COUNT;
    a.rho_bar = hp.rho_bar, a.c_bar = hp.c_bar, a.pg_rho_bar = hp.pg_rho_bar;
    // the waves' padded rows, and behind the rounds the reductions' scratch (6 KiB, what A = 2 takes)
    const size_t lds = (size_t)kWaves * 2 * kCols * (A | 1) * sizeof(float);
    if (lds > 64 * 1024) {  // A > 30: above the default limit of dynamic LDS
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)offpolicy_diag_kernel, raised, (size_t)kWaves * 2 * kCols * 65 * sizeof(float)));
    }
    hipLaunchKernelGGL(offpolicy_diag_kernel, dim3((unsigned)(a.ct * a.slices)), dim3(64 * kWaves), lds, stream, a);
    FI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(offpolicy_diag_finalize_kernel, dim3(1), dim3(kFinalThreads), 0, stream, a, out, col_kl, col_log_rho);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's diagnostics block
namespace {
struct DiagBlock {
    int B = 0;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    char* dev = nullptr;   // fi_offpolicy_diag | col_kl [B] | col_log_rho [B]
    char* host = nullptr;  // the same, pinned
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;  // a result was enqueued
};

void block_free(void* p) {
    DiagBlock* b = (DiagBlock*)p;
    if (!b) return;
    if (b->done) (void)hipEventDestroy(b->done);
    if (b->ws) (void)hipFree(b->ws);
    if (b->dev) (void)hipFree(b->dev);
    if (b->host) (void)hipHostFree(b->host);
    delete b;
}

int block_create(const DiagView& v, DiagBlock** out) {
    DiagBlock* b = new (std::nothrow) DiagBlock();
    FI_REQUIRE(b, "diag_enqueue: out of host memory");
    b->B = v.B;
    b->ws_bytes = diag_workspace_bytes(v.T, v.B, v.A);
    b->bytes = sizeof(fi_offpolicy_diag) + 2 * sizeof(float) * (size_t)v.B;
    int rc = b->ws_bytes ? FI_OK : fail(FI_ERR_INVALID, "diag_enqueue: the learner's shape is outside the kernel's (" +
                                                            std::string(fi_last_error()) + ")");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "diag_enqueue: workspace");
    if (rc == FI_OK) rc = dev_alloc((void**)&b->dev, b->bytes, "diag_enqueue: results");
    if (rc == FI_OK && hipHostMalloc((void**)&b->host, b->bytes, hipHostMallocDefault) != hipSuccess) {
        b->host = nullptr;
        (void)hipGetLastError();
        rc = fail(FI_ERR_OOM, "diag_enqueue: hipHostMalloc(" + std::to_string(b->bytes) + ") for the results");
    }
    if (rc == FI_OK && hipEventCreateWithFlags(&b->done, hipEventDisableTiming) != hipSuccess) {
        b->done = nullptr;
        (void)hipGetLastError();
        rc = fail(FI_ERR_HIP, "diag_enqueue: hipEventCreate failed");
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

extern "C" size_t fi_diag_workspace_bytes(int T, int B, int A) { return diag_workspace_bytes(T, B, A); }

extern "C" int fi_diag_plan(int T, int B, int A, int* column_tiles, int* time_slices) {
    DiagPlan p{};
    FI_TRY(diag_plan(T, B, A, &p));
    if (column_tiles) *column_tiles = p.column_tiles;
    if (time_slices) *time_slices = p.time_slices;
    return FI_OK;
}

extern "C" int fi_diag_offpolicy(int T, int B, int A, const float* pi, const float* mu, const int32_t* act,
                                 const float* rew, const float* disc, const float* val, const float* vs,
                                 const fi_vtrace_hparams* hp, fi_offpolicy_diag* out_dev, float* col_kl_dev,
                                 float* col_log_rho_dev, void* ws, size_t ws_bytes, void* stream) {
    FI_REQUIRE(hp, "diag_offpolicy: null hparams");
    return offpolicy_diag_launch(T, B, A, pi, mu, act, rew, disc, val, vs, *hp, out_dev, col_kl_dev, col_log_rho_dev, ws,
                                 ws_bytes, (hipStream_t)stream);
}

extern "C" int fi_diag_enqueue(fi_learner* l) {
    DiagView v{};
    FI_TRY(learner_diag_view(l, &v));
    if (!v.stepped)
        return fail(FI_ERR_STATE, "diag_enqueue: no step has run on the handle: its loss tensors hold nothing yet");
    FI_HIP_CHECK(hipSetDevice(v.dev));
    DiagBlock* b = (DiagBlock*)v.block;
    if (!b) {
        FI_TRY(block_create(v, &b));
        learner_set_diag_block(l, b, block_free);
    }
    fi_offpolicy_diag* out = (fi_offpolicy_diag*)b->dev;
    float* col_kl = (float*)(b->dev + sizeof(fi_offpolicy_diag));
    // pi: the first T * B rows of the logits; val: the first T * B values. Stream order puts the
    // kernels behind the step that wrote them and in front of the next step's ingest
    FI_TRY(offpolicy_diag_launch(v.T, v.B, v.A, v.logits, v.mu, v.act, v.rew, v.disc, v.values, v.vs, v.hp, out, col_kl,
                                 col_kl + v.B, b->ws, b->ws_bytes, v.stream));
    FI_HIP_CHECK(hipMemcpyAsync(b->host, b->dev, b->bytes, hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipEventRecord(b->done, v.stream));
    b->pending = true;
    return FI_OK;
}

extern "C" int fi_diag_read(fi_learner* l, fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, int32_t n_cols) {
    DiagView v{};
    FI_TRY(learner_diag_view(l, &v));
    FI_REQUIRE(out, "diag_read: null destination");
    FI_REQUIRE((!col_kl && !col_log_rho) || n_cols == v.B,
               "diag_read: n_cols " + std::to_string(n_cols) + " != the learner's batch " + std::to_string(v.B));
    DiagBlock* b = (DiagBlock*)v.block;
    if (!b || !b->pending) return fail(FI_ERR_STATE, "diag_read: nothing was enqueued (fi_diag_enqueue first)");
    FI_HIP_CHECK(hipSetDevice(v.dev));
    FI_HIP_CHECK(hipEventSynchronize(b->done));
    std::memcpy(out, b->host, sizeof(fi_offpolicy_diag));
    const float* cols = (const float*)(b->host + sizeof(fi_offpolicy_diag));
    if (col_kl) std::memcpy(col_kl, cols, sizeof(float) * (size_t)v.B);
    if (col_log_rho) std::memcpy(col_log_rho, cols + v.B, sizeof(float) * (size_t)v.B);
    return FI_OK;
}

extern "C" int fi_diag_learner(fi_learner* l, fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, int32_t n_cols) {
    DiagView v{};
    FI_TRY(learner_diag_view(l, &v));
    FI_REQUIRE(out, "diag_learner: null destination");
    FI_REQUIRE((!col_kl && !col_log_rho) || n_cols == v.B,
               "diag_learner: n_cols " + std::to_string(n_cols) + " != the learner's batch " + std::to_string(v.B));
    FI_TRY(fi_diag_enqueue(l));
    return fi_diag_read(l, out, col_kl, col_log_rho, n_cols);
}
