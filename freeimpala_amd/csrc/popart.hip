// popart.hip -- PopArt value normalisation on the learner (include/fi_popart.h, where the rule
// stands): four small kernels between the launches of a step, and every fi_popart_* entry point.
//
//   popart_denorm_kernel    values = fmaf(sigma_f, values, mu_f)        (T+1) * B floats, in place
//   popart_scale_kernel     dvalue = dvalue / sigma_f                   T * B floats, in place
//   popart_moments_kernel   S1 = sum vs, S2 = sum vs^2 in fp64          one pair of doubles per workgroup
//   popart_finalize_kernel  the statistics move, the value column is rewritten; one workgroup
//
// The statistics live in a 32-byte device block {double mu, nu, sigma; uint64_t updates} that every
// kernel reads where it lies, so an enqueued step sees what the previous enqueued step left. At the
// flagship shape the streams are 1.6 MB: launch-sized kernels, written for few instructions and
// whole 16-byte accesses, not for occupancy. No atomics: every sum has one fixed order.
//
// learner.cpp names nothing of this file: fi_popart_enable hangs a PopartBlock with the three
// launchers on the handle (kernels.h), and run_step calls them while it is there.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "fi_common.h"
#include "fi_popart.h"
#include "host_util.h"
#include "kernels.h"

namespace fi {

namespace {

struct PopartState {  // the device block
    double mu, nu, sigma;
    uint64_t updates;
};
static_assert(sizeof(PopartState) == 32, "fi_popart.h fixes the block at 32 bytes");

constexpr int kBlock = 256;
constexpr int kMomentsPerGroup = 2048;  // targets per workgroup of the moments kernel: 8 per lane
constexpr int kMomentsGridMax = 256;    // one partial per lane of the finalize workgroup

// mu_f, sigma_f: one 8-byte vector load each per lane (volatile keeps the load a plain global one
// in every lane; the block is 32 bytes, every lane of the grid hits the same line)
__device__ __forceinline__ void load_mu_sigma(const void* state, float& mu_f, float& sigma_f) {
    const volatile double* st = (const volatile double*)state;
    mu_f = (float)st[0];
    sigma_f = (float)st[2];
}

// values = fmaf(sigma_f, values, mu_f) in place. The n4 whole quads go 16 bytes per lane by grid
// stride, the n mod 4 elements behind them one lane each; n4 = 0 (a pointer off a 16-byte boundary)
// sends every element down the scalar loop: the same fma, the same bits.
__global__ __launch_bounds__(kBlock) void popart_denorm_kernel(float* __restrict__ v, size_t n, size_t n4,
                                                               const void* __restrict__ state) {
    float mu, sg;
    load_mu_sigma(state, mu, sg);
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4* __restrict__ v4 = (float4*)v;
    for (size_t i = tid; i < n4; i += stride) {
        float4 x = v4[i];
        x.x = fmaf(sg, x.x, mu);
        x.y = fmaf(sg, x.y, mu);
        x.z = fmaf(sg, x.z, mu);
        x.w = fmaf(sg, x.w, mu);
        v4[i] = x;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) v[i] = fmaf(sg, v[i], mu);
}

// dvalue = dvalue / sigma_f in place: a correctly rounded division (not a product with a rounded
// reciprocal), so sigma = 1 is the identity and the result is within half an ulp of the quotient
__global__ __launch_bounds__(kBlock) void popart_scale_kernel(float* __restrict__ d, size_t n, size_t n4,
                                                              const void* __restrict__ state) {
    float mu, sg;
    load_mu_sigma(state, mu, sg);
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4* __restrict__ d4 = (float4*)d;
    for (size_t i = tid; i < n4; i += stride) {
        float4 x = d4[i];
        x.x = __fdiv_rn(x.x, sg);
        x.y = __fdiv_rn(x.y, sg);
        x.z = __fdiv_rn(x.z, sg);
        x.w = __fdiv_rn(x.w, sg);
        d4[i] = x;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) d[i] = __fdiv_rn(d[i], sg);
}

// a workgroup's four wave sums through LDS, added in one fixed order; every lane gets the result
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[kBlock / kWave]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// S1, S2 of one workgroup's share. Quad q = elements [4q, 4q + 4) belongs to lane q mod (grid * 256)
// whatever the pointer's alignment, so the sums have one order; kVec: vs is 16-byte aligned and the
// whole quads are read 16 bytes per lane. Squares of fp32 numbers are exact in fp64.
template <bool kVec>
__global__ __launch_bounds__(kBlock) void popart_moments_kernel(const float* __restrict__ vs, size_t n,
                                                                double* __restrict__ part) {
    __shared__ double red[2][kBlock / kWave];
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t nq = (n + 3) / 4;
    double s1 = 0.0, s2 = 0.0;
    for (size_t q = tid; q < nq; q += stride) {
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (kVec && 4 * q + 4 <= n) {
            const float4 t = ((const float4*)vs)[q];
            x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < n) x[k] = vs[4 * q + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double xd = (double)x[k];
            s1 += xd;
            s2 += xd * xd;
        }
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s1;
        part[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

__device__ __forceinline__ bool finite_bits(double v) {  // a bit test, immune to fast-math folding
    return (__double_as_longlong(v) & 0x7FF0000000000000LL) != 0x7FF0000000000000LL;
}

// One workgroup: lane i adds partial i (nparts <= 256), the state moves, lane j rewrites weight j of
// the value column (and the lanes wrap for H > 256), lane 0 the bias and, last, the state. Every lane
// has read the old state before the barrier inside block_sum2; the new one is stored behind a second
// barrier, so no lane can see it early.
__global__ __launch_bounds__(kBlock) void popart_finalize_kernel(const double* __restrict__ part, int nparts, double n,
                                                                 void* state, float* w, size_t w_stride, int H, float* b,
                                                                 double beta, double sigma_min, double sigma_max,
                                                                 const int* skip) {
#pragma clang fp contract(off)
    __shared__ double red[2][kBlock / kWave];
    if (skip && (skip[0] | skip[1]) != 0) return;  // wave-uniform: the update was skipped, so is this
    const volatile double* st = (const volatile double*)state;
    const double mu = st[0], nu = st[1], sigma = st[2];
    double s1 = 0.0, s2 = 0.0;
    if ((int)threadIdx.x < nparts) {
        s1 = part[2 * threadIdx.x];
        s2 = part[2 * threadIdx.x + 1];
    }
    block_sum2(s1, s2, red);
    if (!finite_bits(s1) || !finite_bits(s2)) return;  // uniform: every lane holds the same sums
    const double mu2 = (1.0 - beta) * mu + beta * (s1 / n);
    const double nu2 = (1.0 - beta) * nu + beta * (s2 / n);
    const double var = nu2 - mu2 * mu2;
    double sigma2 = sqrt(var > 0.0 ? var : 0.0);
    sigma2 = sigma2 < sigma_min ? sigma_min : (sigma2 > sigma_max ? sigma_max : sigma2);
    for (int j = threadIdx.x; j < H; j += kBlock) {
        float* wj = w + (size_t)j * w_stride;
        *wj = (float)((double)*wj * sigma / sigma2);
    }
    if (threadIdx.x == 0) *b = (float)((sigma * (double)*b + (mu - mu2)) / sigma2);
    __syncthreads();
    if (threadIdx.x == 0) {
        PopartState* out = (PopartState*)state;
        const uint64_t updates = out->updates;
        out->mu = mu2;
        out->nu = nu2;
        out->sigma = sigma2;
        out->updates = updates + 1;
    }
}

bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

// workgroups of a streaming kernel over `lanes` lanes of work
int stream_grid(size_t lanes) {
    const size_t g = (lanes + kBlock - 1) / kBlock;
    return (int)(g > (size_t)kPopartStreamGridMax ? (size_t)kPopartStreamGridMax : (g < 1 ? 1 : g));
}

}  // namespace

int popart_plan(size_t n) {
    if (n == 0) return 0;
    const size_t g = (n + kMomentsPerGroup - 1) / kMomentsPerGroup;
    return (int)(g > (size_t)kMomentsGridMax ? (size_t)kMomentsGridMax : g);
}

size_t popart_workspace_bytes(size_t n) { return (size_t)popart_plan(n) * 2 * sizeof(double); }

int popart_denorm_launch(float* values, size_t n, const void* state, hipStream_t s) {
    const size_t n4 = aligned16(values) ? n / 4 : 0;
    hipLaunchKernelGGL(popart_denorm_kernel, dim3(stream_grid(n4 ? n4 + (n & 3) : n)), dim3(kBlock), 0, s, values, n, n4,
                       state);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int popart_scale_launch(float* dvalue, size_t n, const void* state, hipStream_t s) {
    const size_t n4 = aligned16(dvalue) ? n / 4 : 0;
    hipLaunchKernelGGL(popart_scale_kernel, dim3(stream_grid(n4 ? n4 + (n & 3) : n)), dim3(kBlock), 0, s, dvalue, n, n4,
                       state);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int popart_update_launch(const float* vs, size_t n, void* state, float* w, size_t w_stride, int H, float* b, double beta,
                         double sigma_min, double sigma_max, const int* skip, void* ws, size_t ws_bytes, hipStream_t s) {
    const int grid = popart_plan(n);
    FI_REQUIRE(grid >= 1 && ws_bytes >= popart_workspace_bytes(n),
               "popart_update: the workspace holds " + std::to_string(ws_bytes) + " bytes, " + std::to_string(n) +
                   " targets need " + std::to_string(popart_workspace_bytes(n)));
    double* part = (double*)ws;
    if (aligned16(vs)) hipLaunchKernelGGL(popart_moments_kernel<true>, dim3(grid), dim3(kBlock), 0, s, vs, n, part);
    else hipLaunchKernelGGL(popart_moments_kernel<false>, dim3(grid), dim3(kBlock), 0, s, vs, n, part);
    hipLaunchKernelGGL(popart_finalize_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)part, grid, (double)n, state, w,
                       w_stride, H, b, beta, sigma_min, sigma_max, skip);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

namespace {

// beta and the bounds of fi_popart_enable / fi_popart_update: refused before any device call
int check_hparams(const std::string& who, double beta, double sigma_min, double sigma_max) {
    FI_REQUIRE(beta >= 0.0 && beta <= 1.0, who + ": beta " + std::to_string(beta) + " outside [0, 1]");
    FI_REQUIRE(std::isfinite(sigma_min) && sigma_min > 0.0 && sigma_min <= 1.0,
               who + ": sigma_min " + std::to_string(sigma_min) + " outside (0, 1]");
    FI_REQUIRE(std::isfinite(sigma_max) && sigma_max >= 1.0,
               who + ": sigma_max " + std::to_string(sigma_max) + " is below 1 or not finite");
    return FI_OK;
}

double clamp_sigma(double var, double lo, double hi) {
    const double s = std::sqrt(var > 0.0 ? var : 0.0);
    return s < lo ? lo : (s > hi ? hi : s);
}

void block_free(void* p) {
    PopartBlock* b = (PopartBlock*)p;
    if (!b) return;
    if (b->state) (void)hipFree(b->state);
    if (b->ws) (void)hipFree(b->ws);
    delete b;
}

int block_create(const PopartView& v, PopartBlock** out) {
    PopartBlock* b = new (std::nothrow) PopartBlock();
    FI_REQUIRE(b, "popart_enable: out of host memory");
    b->ws_bytes = popart_workspace_bytes((size_t)v.TB);
    b->denorm = popart_denorm_launch;
    b->scale = popart_scale_launch;
    b->update = popart_update_launch;
    int rc = dev_alloc(&b->state, sizeof(PopartState), "popart_enable: state");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "popart_enable: workspace");
    if (rc == FI_OK) {
        const PopartState init{0.0, 1.0, 1.0, 0};
        const hipError_t e = hipMemcpyAsync(b->state, &init, sizeof(init), hipMemcpyHostToDevice, v.stream);
        if (e != hipSuccess || hipStreamSynchronize(v.stream) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "popart_enable: writing the initial state failed");
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

extern "C" int fi_popart_enable(fi_learner* l, double beta, double sigma_min, double sigma_max) {
    FI_REQUIRE(l, "popart_enable: null learner");
    FI_TRY(check_hparams("popart_enable", beta, sigma_min, sigma_max));
    PopartView v{};
    FI_TRY(learner_popart_view(l, &v));
    if (v.nranks > 1)
        return fail(FI_ERR_STATE, "popart_enable: the handle is attached to a communicator of " + std::to_string(v.nranks) +
                                      " ranks; per-rank statistics would make the ranks' value heads diverge");
    PopartBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("popart_enable", FI_ERR_OOM, [&] { return block_create(v, &b); }));
        learner_set_popart_block(l, b, block_free);
    }
    b->beta = beta;  // by value into every later finalize launch; the statistics stay
    b->sigma_min = sigma_min;
    b->sigma_max = sigma_max;
    return FI_OK;
}

extern "C" int fi_popart_get_state(fi_learner* l, fi_popart_state* out) {
    FI_REQUIRE(l && out, "popart_get_state: null argument");
    PopartView v{};
    FI_TRY(learner_popart_view(l, &v));
    std::memset(out, 0, sizeof(*out));
    out->beta = FI_POPART_BETA;
    out->sigma_min = FI_POPART_SIGMA_MIN;
    out->sigma_max = FI_POPART_SIGMA_MAX;
    out->nu = 1.0;
    out->sigma = 1.0;
    const PopartBlock* b = v.block;
    if (!b) return FI_OK;
    PopartState st{};
    FI_HIP_CHECK(hipSetDevice(v.dev));
    FI_HIP_CHECK(hipMemcpyAsync(&st, b->state, sizeof(st), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    out->enabled = 1;
    out->beta = b->beta;
    out->sigma_min = b->sigma_min;
    out->sigma_max = b->sigma_max;
    out->mu = st.mu;
    out->nu = st.nu;
    out->sigma = st.sigma;
    out->updates = st.updates;
    return FI_OK;
}

extern "C" int fi_popart_set_state(fi_learner* l, double mu, double nu) {
    FI_REQUIRE(l, "popart_set_state: null learner");
    PopartView v{};
    FI_TRY(learner_popart_view(l, &v));
    if (!v.block) return fail(FI_ERR_STATE, "popart_set_state: PopArt is off on this handle (fi_popart_enable first)");
    FI_REQUIRE(std::isfinite(mu) && std::isfinite(nu),
               "popart_set_state: mu " + std::to_string(mu) + " or nu " + std::to_string(nu) + " is not finite");
    FI_REQUIRE(nu >= mu * mu, "popart_set_state: nu " + std::to_string(nu) + " < mu^2 " + std::to_string(mu * mu) +
                                  ": no distribution has these moments");
    const double st[3] = {mu, nu, clamp_sigma(nu - mu * mu, v.block->sigma_min, v.block->sigma_max)};
    FI_HIP_CHECK(hipSetDevice(v.dev));
    // behind every enqueued step; `updates`, the fourth word, is kept
    FI_HIP_CHECK(hipMemcpyAsync(v.block->state, st, sizeof(st), hipMemcpyHostToDevice, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    return FI_OK;
}

extern "C" int fi_popart_state_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "popart_state_dev: null argument");
    PopartView v{};
    FI_TRY(learner_popart_view(l, &v));
    if (!v.block) return fail(FI_ERR_STATE, "popart_state_dev: PopArt is off on this handle (fi_popart_enable first)");
    *ptr = v.block->state;
    return FI_OK;
}

extern "C" int fi_popart_plan(size_t n) { return popart_plan(n); }
extern "C" size_t fi_popart_workspace_bytes(size_t n) { return popart_workspace_bytes(n); }

extern "C" int fi_popart_denormalize(float* values, size_t n, const void* state_dev, void* stream) {
    FI_REQUIRE(values && state_dev && n >= 1, "popart_denormalize: null argument or n = 0");
    FI_REQUIRE((uintptr_t)values % 4 == 0 && (uintptr_t)state_dev % 8 == 0,
               "popart_denormalize: values must be 4-byte and state_dev 8-byte aligned");
    return popart_denorm_launch(values, n, state_dev, (hipStream_t)stream);
}

extern "C" int fi_popart_scale_grad(float* dvalue, size_t n, const void* state_dev, void* stream) {
    FI_REQUIRE(dvalue && state_dev && n >= 1, "popart_scale_grad: null argument or n = 0");
    FI_REQUIRE((uintptr_t)dvalue % 4 == 0 && (uintptr_t)state_dev % 8 == 0,
               "popart_scale_grad: dvalue must be 4-byte and state_dev 8-byte aligned");
    return popart_scale_launch(dvalue, n, state_dev, (hipStream_t)stream);
}

extern "C" int fi_popart_update(const float* vs, size_t n, void* state_dev, float* w, size_t w_stride, int H, float* b,
                                double beta, double sigma_min, double sigma_max, const int* skip_dev, void* ws,
                                size_t ws_bytes, void* stream) {
    FI_REQUIRE(vs && state_dev && w && b && ws && n >= 1, "popart_update: null argument or n = 0");
    FI_REQUIRE(H >= 1 && w_stride >= 1, "popart_update: H and w_stride must be >= 1");
    FI_REQUIRE(((uintptr_t)vs | (uintptr_t)w | (uintptr_t)b | (uintptr_t)skip_dev) % 4 == 0 &&
                   ((uintptr_t)state_dev | (uintptr_t)ws) % 8 == 0,
               "popart_update: float pointers must be 4-byte, state_dev and ws 8-byte aligned");
    FI_TRY(check_hparams("popart_update", beta, sigma_min, sigma_max));
    return popart_update_launch(vs, n, state_dev, w, w_stride, H, b, beta, sigma_min, sigma_max, skip_dev, ws, ws_bytes,
                                (hipStream_t)stream);
}
