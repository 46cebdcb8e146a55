// target.hip -- the learner's target network (include/fi_target.h, where the rule stands): IMPACT's
// clipped ratio around a slowly moving copy theta- of the parameters, and every fi_target_* entry point.
//
//   target_loss_kernel    surrogate_loss_kernel's grid and read pattern (row_stream.h) over two logit
//                         streams: the pi and pi_tgt rows of one (t, tile) arrive together in padded LDS
//                         rows (load_run<true>), then one lane per row. (log pi(a), log pi_tgt(a)) come
//                         from pair_log_prob, the softmax / entropy / gradient arithmetic is
//                         policy_row_grad: policy_row.h's one copy, shared with surrogate.hip. dlogits are
//                         written over the lane's pi row and leave as the run's 16-byte pieces. Six fp64
//                         sums per workgroup: L_pg, baseline, entropy | clipped rows, sum log r, sum (log r)^2.
//   target_stats_kernel   one workgroup: the partials added in a fixed order; the surrogate's 32-byte block,
//                         bytes 8 .. 31 of the target's, and for the stand-alone entry the three loss scalars.
//   target_update_kernel  theta- <- (tau == 1) ? theta : fmaf(tau, theta - theta-, theta-), 16 bytes per
//                         lane and access, a scalar tail, a grid stride; nothing when the optimiser skipped.
// The targets (vs, A, log rho_t against pi_tgt) are surrogate.hip's rows and scan kernels on (tlogits, mu),
// unchanged (surrogate_front_launch). No float atomics. learner.cpp names nothing of this file:
// fi_target_enable hangs a TargetBlock with the two launchers on the handle (kernels.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "atari.h"  // KernelTagger, TagScope
#include "fi_common.h"
#include "fi_target.h"
#include "host_util.h"
#include "kernels.h"
#include "policy_row.h"
#include "row_stream.h"

namespace fi {

namespace {
static_assert(sizeof(fi_target_stats) == 32 && sizeof(fi_target_params) == 16, "fi_target.h fixes both sizes");

struct SurStats {  // fi_surrogate.h's block
    uint64_t rows, rows_clipped;
    double adv_mean, adv_std;
};

struct TgtArgs {
    int T, B, A;
    int ct, slices, slice_len, nscan;
    const float* __restrict__ pi;
    const float* __restrict__ tgt;
    const int32_t* __restrict__ act;
    const float* __restrict__ val;
    const float* __restrict__ vs;   // the front's outputs
    const float* __restrict__ adv;
    const float* __restrict__ lr;   // log rho_t = log pi_tgt(a) - log mu(a)
    const double* mom;
    const double* pivot;
    float* dlog;
    float* dval;
    double* part;   // [ct * slices][3]: L_pg, baseline, entropy (what grad_sqnorm adds)
    double* extra;  // [ct * slices][3]: clipped rows, sum log r, sum (log r)^2
    const int* bad;
    float pg_rho_bar, bc, ec;
    float clip, adv_eps;
    uint32_t normalize;
};
}  // namespace

__global__ __launch_bounds__(64 * kWaves) void target_loss_kernel(TgtArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    __shared__ double red[kWaves * 6];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * 2 * kCols * S;  // this wave's pi rows (dlogits after the arithmetic),
    float* const lt = lp + kCols * S;                           // then its pi_tgt rows
    const uint32_t n = (uint32_t)nb * A;
    double m = 0.0, sd = 1.0;
    if (a.normalize) adv_moments(a.mom, a.pivot, a.nscan, T, B, red, m, sd);  // uniform over the grid
    const double den = sd + (double)a.adv_eps;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    if (s == 0 && tid < nb) a.dval[(size_t)T * B + b0 + tid] = 0.f;  // the bootstrap row has no gradient
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        const uint32_t g0 = ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A;
        int at = 0;
        float lrt = 0.f, adv = 0.f, v = 0.f, vs = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            lrt = a.lr[e];
            adv = a.adv[e];
            v = a.val[e];
            vs = a.vs[e];
        }
        if (live) load_run<true>(a.pi, a.tgt, lp, lt, g0, n, A, S, lane);
        __syncthreads();  // the rows are in LDS
        if (mine) {
            float* z = lp + (uint32_t)lane * S;
            const uint32_t ai = at < 0 ? 0u : ((uint32_t)at >= A ? A - 1u : (uint32_t)at);
            const f32x2 la = pair_log_prob(z, lt + (uint32_t)lane * S, A, ai);  // log pi(a), log pi_tgt(a)
            const float lr = la.x - la.y;
            const float r = __expf(lr);
            const float beta = fminf(a.pg_rho_bar, __expf(lrt));
            const float an = a.normalize ? (float)(((double)adv - m) / den) : adv;
            const bool clipped = (an > 0.f && r > hi) || (an < 0.f && r < lo);
            const float rc = fminf(fmaxf(r, lo), hi);
            const float g = clipped ? 0.f : -beta * r * an;
            const float plogp = policy_row_grad(z, A, ai, g, a.ec);
            const float td = v - vs;
            a.dval[(size_t)t * B + b0 + lane] = a.bc * td;
            sum[0] += (double)(-beta * fminf(r * an, rc * an));
            sum[1] += 0.5 * (double)td * (double)td;
            sum[2] += (double)plogp;
            sum[3] += clipped ? 1.0 : 0.0;
            sum[4] += (double)lr;
            sum[5] += (double)lr * (double)lr;
        }
        __syncthreads();  // the dlogits rows are complete
        if (live) store_run(a.dlog, lp, g0, n, A, S, lane);
        __syncthreads();  // the rows have left: the next round may overwrite them
    }
    block_sums<6, kWaves>(sum, red);
    if (tid < 3) a.part[(size_t)blockIdx.x * 3 + tid] = sum[tid];
    else if (tid < 6) a.extra[(size_t)blockIdx.x * 3 + (tid - 3)] = sum[tid];
}

// One workgroup. sur, tgt, losses: each nullable. The target block's first word, `updates`, is the update
// kernel's: not touched here.
__global__ __launch_bounds__(kStatThreads) void target_stats_kernel(TgtArgs a, void* sur, void* tgt, double* losses) {
    __shared__ double red[kWaves * 6];
    double m, sd;
    adv_moments(a.mom, a.pivot, a.nscan, a.T, a.B, red, m, sd);
    const int nblk = a.ct * a.slices;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += kStatThreads) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            v[j] += a.part[(size_t)i * 3 + j];
            v[3 + j] += a.extra[(size_t)i * 3 + j];
        }
    }
    block_sums<6, kWaves>(v, red);
    if (threadIdx.x != 0) return;
    const uint64_t rows = (uint64_t)a.T * (uint64_t)a.B;
    if (sur) {
        SurStats* o = (SurStats*)sur;
        o->rows = rows;
        o->rows_clipped = (uint64_t)v[3];
        o->adv_mean = m;
        o->adv_std = sd;
    }
    if (tgt) {
        fi_target_stats* o = (fi_target_stats*)tgt;
        o->rows = rows;
        o->mean_log_r = v[4] / (double)rows;
        o->mean_sq_log_r = v[5] / (double)rows;
    }
    if (losses) {
        const bool poisoned = *a.bad != 0;
        for (int i = 0; i < 3; ++i) losses[i] = poisoned ? __builtin_nan("") : v[i];
    }
}

// n4 = n / 4 whole quads, one float4 per lane and access; the n mod 4 elements behind them one per lane.
// skip (nullable): the optimiser's flag words; updates (nullable): the block's count. dst and src never alias.
__global__ __launch_bounds__(256) void target_update_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n,
                                                            size_t n4, float tau, const int* __restrict__ skip,
                                                            uint64_t* __restrict__ updates) {
    if (skip && (skip[0] | skip[1]) != 0) return;  // uniform over the grid: the update was skipped, so is this
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const float4* __restrict__ s4 = (const float4*)src;
    float4* __restrict__ d4 = (float4*)dst;
    if (tau == 1.0f) {
        for (size_t i = tid; i < n4; i += stride) d4[i] = s4[i];
        for (size_t i = 4 * n4 + tid; i < n; i += stride) dst[i] = src[i];
    } else {
        for (size_t i = tid; i < n4; i += stride) {
            const float4 p = s4[i];
            float4 q = d4[i];
            q.x = fmaf(tau, p.x - q.x, q.x);
            q.y = fmaf(tau, p.y - q.y, q.y);
            q.z = fmaf(tau, p.z - q.z, q.z);
            q.w = fmaf(tau, p.w - q.w, q.w);
            d4[i] = q;
        }
        for (size_t i = 4 * n4 + tid; i < n; i += stride) {
            const float q = dst[i];
            dst[i] = fmaf(tau, src[i] - q, q);
        }
    }
    if (updates && tid == 0) *updates = *updates + 1;
}

// ------------------------------------------------------------------ the launchers
namespace {
size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: a surrogate workspace | loss partials | the three further partials; each on a 256-byte boundary
struct Layout {
    size_t part, extra, total;
};
bool layout_of(int T, int B, int A, Layout* l) {
    const size_t sur = surrogate_workspace_bytes(T, B, A);
    if (!sur) return false;
    const size_t nblk = (size_t)surrogate_loss_blocks(T, B, A);
    l->part = pad256(sur);
    l->extra = l->part + pad256(nblk * 3 * sizeof(double));
    l->total = l->extra + pad256(nblk * 3 * sizeof(double));
    return true;
}

int check_tau(const std::string& who, float tau) {
    FI_REQUIRE(std::isfinite(tau) && tau > 0.f && tau <= 1.f, who + ": tau " + std::to_string(tau) + " must be in (0, 1]");
    return FI_OK;
}

int update_launch(float* dst, const float* src, size_t n, float tau, const int* skip, uint64_t* updates, hipStream_t s) {
    FI_REQUIRE(dst && src, "target_update: null argument");
    FI_TRY(check_tau("target_update", tau));
    FI_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 15) == 0,
               "target_update: params and target must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE(((uintptr_t)skip & 3) == 0, "target_update: skip must be 4-byte aligned");
    if (n == 0 && !updates) return FI_OK;
    const size_t n4 = n / 4;
    // one quad per lane up to 2,048 workgroups (8 per CU), publish_params_kernel's grid: the Atari policy's
    // 1.69 M parameters take 1,655; the grid stride takes the rest. At least one workgroup
    size_t wgs = (n4 + (n & 3) + 255) / 256;
    wgs = wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs);
    hipLaunchKernelGGL(target_update_kernel, dim3((unsigned)wgs), dim3(256), 0, s, dst, src, n, n4, tau, skip, updates);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int target_launch(int T, int B, int A, const float* pi, const float* tgt, const float* mu, const int32_t* act,
                  const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp,
                  const fi_surrogate_params& prm, float* vs, float* adv, float* dlog, float* dval, double* losses,
                  void* sur_stats, void* tgt_stats, void* ws, size_t ws_bytes, int* bad, hipStream_t stream, KernelTagger* tg,
                  const double** partials, int* nblk_out) {
    FI_REQUIRE(pi && tgt && mu && act && rew && disc && val && vs && adv && dlog && dval && ws, "target_loss: null argument");
    TilePlan p{};
    FI_TRY(tile_plan("target_loss", T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)tgt % 16 == 0 && (uintptr_t)mu % 16 == 0 && (uintptr_t)dlog % 16 == 0,
               "target_loss: pi, tgt, mu and dlogits must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)act % 4 == 0 && (uintptr_t)rew % 4 == 0 && (uintptr_t)disc % 4 == 0 && (uintptr_t)val % 4 == 0 &&
                   (uintptr_t)vs % 4 == 0 && (uintptr_t)adv % 4 == 0 && (uintptr_t)dval % 4 == 0 && (uintptr_t)bad % 4 == 0,
               "target_loss: act, rew, disc, val, vs, adv, dvalue and bad must be 4-byte aligned");
    FI_REQUIRE((uintptr_t)losses % 8 == 0 && (uintptr_t)sur_stats % 8 == 0 && (uintptr_t)tgt_stats % 8 == 0 &&
                   (uintptr_t)ws % 8 == 0,
               "target_loss: losses, the stats blocks and ws must be 8-byte aligned");
    Layout lay{};
    FI_REQUIRE(layout_of(T, B, A, &lay), "target_loss: the shape is outside the surrogate's kernels");
    FI_REQUIRE(ws_bytes >= lay.total, "target_loss: ws_bytes " + std::to_string(ws_bytes) + " < " + std::to_string(lay.total) +
                                          " = fi_target_workspace_bytes(" + std::to_string(T) + ", " + std::to_string(B) +
                                          ", " + std::to_string(A) + ")");
    // two padded row sets per wave: more than 64 KB of dynamic LDS at A > 30
    const size_t lds = 2 * (size_t)kWaves * kCols * (A | 1) * sizeof(float), lds_most = 2 * (size_t)kWaves * kCols * 65 * 4;
    if (lds > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)target_loss_kernel, raised, lds_most));
    }
    // 2. the targets: the surrogate's rows and scan kernels with pi_tgt in pi's place
    SurrogateFront f{};
    FI_TRY(surrogate_front_launch(T, B, A, tgt, mu, act, rew, disc, val, hp, vs, adv, ws, lay.part, bad, stream, tg, &f));
    char* w = (char*)ws;
    TgtArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = f.ct, a.slices = f.slices, a.slice_len = f.slice_len, a.nscan = f.nscan;
    a.pi = pi, a.tgt = tgt, a.act = act, a.val = val;
    a.vs = vs, a.adv = adv, a.lr = f.lr, a.mom = f.mom, a.pivot = f.pivot;
    a.dlog = dlog, a.dval = dval;
    a.part = (double*)(w + lay.part), a.extra = (double*)(w + lay.extra);
    a.bad = f.bad;
    a.pg_rho_bar = hp.pg_rho_bar, a.bc = hp.baseline_cost, a.ec = hp.entropy_cost;
    a.clip = prm.clip, a.adv_eps = prm.adv_eps, a.normalize = prm.normalize;
    const unsigned nblk = (unsigned)(f.ct * f.slices);
    {
        TagScope t(tg, "target_loss");
        hipLaunchKernelGGL(target_loss_kernel, dim3(nblk), dim3(64 * kWaves), lds, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (sur_stats || tgt_stats || losses) {
        TagScope t(tg, "target_stats");
        hipLaunchKernelGGL(target_stats_kernel, dim3(1), dim3(kStatThreads), 0, stream, a, sur_stats, tgt_stats, losses);
        FI_HIP_CHECK(hipGetLastError());
    }
    if (partials) *partials = a.part;
    if (nblk_out) *nblk_out = (int)nblk;
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's block
int block_launch(const TargetBlock* b, const SurrogateBlock* sb, int T, int B, int A, const float* pi, const float* mu,
                 const int32_t* act, const float* rew, const float* disc, const float* val, const fi_vtrace_hparams& hp,
                 float* vs, float* adv, float* dlog, float* dval, int* bad, hipStream_t stream, KernelTagger* tg,
                 const double** partials, int* nblk) {
    const fi_surrogate_params prm{sb->clip, sb->normalize, sb->adv_eps, 0u};
    return target_launch(T, B, A, pi, b->tlogits, mu, act, rew, disc, val, hp, prm, vs, adv, dlog, dval, nullptr, sb->stats,
                         b->stats, b->ws, b->ws_bytes, bad, stream, tg, partials, nblk);
}

int block_update(const TargetBlock* b, const float* params, const int* skip, hipStream_t stream) {
    return update_launch(b->theta, params, b->nparams, b->tau, skip, (uint64_t*)b->stats, stream);
}

void block_free(void* p) {
    TargetBlock* b = (TargetBlock*)p;
    if (!b) return;
    for (void* q : {(void*)b->theta, (void*)b->tlogits, (void*)b->tvalues, b->stats, b->ws})
        if (q) (void)hipFree(q);
    delete b;
}

int block_create(const TargetView& v, TargetBlock** out) {
    TargetBlock* b = new (std::nothrow) TargetBlock();
    FI_REQUIRE(b, "target_enable: out of host memory");
    b->launch = block_launch;
    b->update = block_update;
    b->nparams = v.nparams;
    Layout lay{};
    int rc = layout_of(v.T, v.B, v.A, &lay) ? FI_OK
                                            : fail(FI_ERR_INVALID, "target_enable: the learner's shape is outside the kernels' (" +
                                                                       std::string(fi_last_error()) + ")");
    b->ws_bytes = lay.total;
    const size_t rows = (size_t)(v.T + 1) * v.B;
    if (rc == FI_OK) rc = dev_alloc((void**)&b->theta, v.nparams * sizeof(float), "target_enable: target parameters");
    if (rc == FI_OK) rc = dev_alloc((void**)&b->tlogits, rows * v.A * sizeof(float), "target_enable: target logits");
    if (rc == FI_OK) rc = dev_alloc((void**)&b->tvalues, rows * sizeof(float), "target_enable: scratch values");
    if (rc == FI_OK) rc = dev_alloc(&b->stats, sizeof(fi_target_stats), "target_enable: stats block");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "target_enable: workspace");
    if (rc == FI_OK) {
        hipError_t e = hipMemsetAsync(b->stats, 0, sizeof(fi_target_stats), v.stream);
        if (e == hipSuccess) e = hipMemsetAsync(b->tlogits, 0, rows * v.A * sizeof(float), v.stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b->theta, v.params, v.nparams * sizeof(float), hipMemcpyDeviceToDevice, v.stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "target_enable: initialising the target failed");
        }
    }
    if (rc != FI_OK) {
        (void)hipStreamSynchronize(v.stream);
        block_free(b);
        return rc;
    }
    *out = b;
    return FI_OK;
}

// the view of a handle whose target exists
int enabled_view(fi_learner* l, const char* who, TargetView* v) {
    FI_TRY(learner_target_view(l, v));
    if (!v->block)
        return fail(FI_ERR_STATE, std::string(who) + ": the target was never on on this handle (fi_target_enable first)");
    FI_HIP_CHECK(hipSetDevice(v->dev));
    return FI_OK;
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_target_enable(fi_learner* l, const fi_target_params* params) {
    FI_REQUIRE(l && params, "target_enable: null argument");
    FI_REQUIRE(params->period >= 1u, "target_enable: period 0 (an update every K-th step, K >= 1)");
    FI_TRY(check_tau("target_enable", params->tau));
    TargetView v{};
    FI_TRY(learner_target_view(l, &v));
    TargetBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("target_enable", FI_ERR_OOM, [&] { return block_create(v, &b); }));
        learner_set_target_block(l, b, block_free);
    }
    b->period = params->period;  // by value into every later launch
    b->tau = params->tau;
    b->on = true;
    return FI_OK;
}

extern "C" int fi_target_disable(fi_learner* l) {
    FI_REQUIRE(l, "target_disable: null learner");
    TargetView v{};
    FI_TRY(learner_target_view(l, &v));
    if (v.block) v.block->on = false;
    return FI_OK;
}

extern "C" int fi_target_sync(fi_learner* l) {
    FI_REQUIRE(l, "target_sync: null learner");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_sync", &v));
    return update_launch(v.block->theta, v.params, v.nparams, 1.0f, nullptr, nullptr, v.stream);
}

extern "C" int fi_target_get_params(fi_learner* l, float* dst, size_t n) {
    FI_REQUIRE(l && dst, "target_get_params: null argument");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_get_params", &v));
    FI_REQUIRE(n == v.nparams, "target_get_params: n = " + std::to_string(n) + ", the policy has " + std::to_string(v.nparams));
    FI_HIP_CHECK(hipMemcpyAsync(dst, v.block->theta, n * sizeof(float), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    return FI_OK;
}

extern "C" int fi_target_set_params(fi_learner* l, const float* src, size_t n) {
    FI_REQUIRE(l && src, "target_set_params: null argument");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_set_params", &v));
    FI_REQUIRE(n == v.nparams, "target_set_params: n = " + std::to_string(n) + ", the policy has " + std::to_string(v.nparams));
    FI_HIP_CHECK(hipMemcpyAsync(v.block->theta, src, n * sizeof(float), hipMemcpyHostToDevice, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));  // src is the caller's again
    return FI_OK;
}

extern "C" int fi_target_get_state(fi_learner* l, fi_target_params* params, fi_target_stats* stats, uint32_t* enabled) {
    FI_REQUIRE(l, "target_get_state: null learner");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_get_state", &v));
    const TargetBlock* b = v.block;
    fi_target_stats st{};
    FI_HIP_CHECK(hipMemcpyAsync(&st, b->stats, sizeof(st), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    if (params) *params = fi_target_params{b->period, b->tau, {0u, 0u}};
    if (stats) *stats = st;
    if (enabled) *enabled = b->on ? 1u : 0u;
    return FI_OK;
}

extern "C" int fi_target_params_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "target_params_dev: null argument");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_params_dev", &v));
    *ptr = v.block->theta;
    return FI_OK;
}

extern "C" int fi_target_logits_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "target_logits_dev: null argument");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_logits_dev", &v));
    *ptr = v.block->tlogits;
    return FI_OK;
}

extern "C" int fi_target_stats_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "target_stats_dev: null argument");
    TargetView v{};
    FI_TRY(enabled_view(l, "target_stats_dev", &v));
    *ptr = v.block->stats;
    return FI_OK;
}

extern "C" size_t fi_target_workspace_bytes(int T, int B, int A) {
    Layout lay{};
    return layout_of(T, B, A, &lay) ? lay.total : 0;
}

extern "C" int fi_target_loss_fp32(int T, int B, int A, const float* pi, const float* tgt, const float* mu, const int32_t* act,
                                   const float* rew, const float* disc, const float* val, const fi_vtrace_hparams* hp,
                                   const fi_surrogate_params* surrogate_params, float* vs, float* adv, float* dlogits,
                                   float* dvalue, double* losses, void* surrogate_stats_dev, void* target_stats_dev, void* ws,
                                   size_t ws_bytes, int* bad, void* stream) {
    FI_REQUIRE(hp, "target_loss: null hparams");
    FI_TRY(surrogate_check_params("target_loss", surrogate_params));
    return target_launch(T, B, A, pi, tgt, mu, act, rew, disc, val, *hp, *surrogate_params, vs, adv, dlogits, dvalue, losses,
                         surrogate_stats_dev, target_stats_dev, ws, ws_bytes, bad, (hipStream_t)stream, nullptr, nullptr,
                         nullptr);
}

extern "C" int fi_target_update(const float* params, float* target, size_t n, float tau, const int* skip, void* stream) {
    return update_launch(target, params, n, tau, skip, nullptr, (hipStream_t)stream);
}
