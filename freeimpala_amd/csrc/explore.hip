// explore.hip -- actor exploration behind the C ABI of include/fi_explore.h: the draw with a
// temperature and a per-environment epsilon, and the behaviour logits that go into a record's mu.
//
//   * sample_behaviour_kernel: sample_actions_kernel's layout (one lane per row, the row in
//     registers, AMAX in {8, 18, 32, 64}) with the rule of fi_explore.h; it writes the action and the
//     A behaviour logits of its row and leaves the policy's logits alone
//   * the handle's side (fi_explore_set / clear / get / behaviour_dev / read_behaviour) works on the
//     ExploreState an actor handle carries (kernels.h); fi_explore_set puts sample_behaviour_launch
//     there, and actor.hip's act calls call it where they launch the plain sampler. actor.hip names
//     nothing of this file
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fi_common.h"
#include "fi_explore.h"
#include "host_util.h"
#include "kernels.h"

namespace fi {

// The mu stores. A lane holds a whole row, so storing from the registers would put lane j's float a
// at byte 4 (j A + a): 64 lines touched per store instruction. The rows of a wave are contiguous in
// mu (64 A floats), so each wave turns its rows through LDS -- row r at r (AMAX + 1) floats, an odd
// stride: the 64 lanes of a column write hit distinct banks -- and stores float 64 k + j of the
// wave's range from lane j: 256 contiguous bytes per store instruction. The logits are read as
// sample_actions_kernel reads them.
template <int AMAX, int BLOCK>
__global__ __launch_bounds__(BLOCK) void sample_behaviour_kernel(const float* __restrict__ logits, int N, int A, float tau,
                                                                 const float* __restrict__ eps, uint64_t seed,
                                                                 uint64_t draw, int32_t* __restrict__ actions,
                                                                 float* __restrict__ mu, int* __restrict__ nonfinite) {
    constexpr int S = AMAX + 1;
    __shared__ float turn[BLOCK / 64][64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = i < N;
    float l[AMAX], p[AMAX];
    if (valid) {
        const float* __restrict__ row = logits + (size_t)i * A;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) l[a] = a < A ? row[a] : 0.f;
        float m = l[0];
        bool finite = true;
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
            if (a < A) {
                finite = finite && (fabsf(l[a]) <= 3.402823466e+38f);  // false for NaN and for +-Inf
                m = l[a] > m ? l[a] : m;
            }
        int act = 0;
        if (!finite) {  // l stays: the mu row is the policy's logits
            if (nonfinite) atomicAdd(nonfinite, 1);
        } else {
            float Z = 0.f;
#pragma unroll
            for (int a = 0; a < AMAX; ++a)
                if (a < A) {
                    l[a] = (l[a] - m) / tau;
                    p[a] = expf(l[a]);
                    Z += p[a];
                }
            const float e = eps ? eps[i] : 0.f;
            const float k = 1.f - e, c = (e * Z) / (float)A;
            float W = 0.f;
#pragma unroll
            for (int a = 0; a < AMAX; ++a)
                if (a < A) {
                    p[a] = fmaf(k, p[a], c);
                    W += p[a];
                }
            const uint4 x = philox4(seed, draw * (uint64_t)N + (uint64_t)i, ST_SAMPLE);
            const float u = (float)(x.x >> 8) * 0x1p-24f;
            const float thr = u * W;
            float run = 0.f;
            bool found = false;
            act = A - 1;
#pragma unroll
            for (int a = 0; a < AMAX; ++a)
                if (a < A) {
                    run += p[a];
                    if (!found && run > thr) {
                        act = a;
                        found = true;
                    }
                }
            if (c > 0.f) {  // not e > 0: an epsilon so small that c rounds to 0 leaves w_a = p_a, which may be 0
                const float lW = logf(W);
#pragma unroll
                for (int a = 0; a < AMAX; ++a)
                    if (a < A) l[a] = logf(p[a]) - lW;
            } else {
                const float lZ = logf(Z);
#pragma unroll
                for (int a = 0; a < AMAX; ++a)
                    if (a < A) l[a] = l[a] - lZ;
            }
        }
        actions[i] = act;
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
            if (a < A) turn[wave][lane * S + a] = l[a];
    }
    __syncthreads();
    const int row0 = blockIdx.x * BLOCK + wave * 64;  // the wave's first row
    const int rows = N - row0 < 64 ? N - row0 : 64;   // <= 0: a wave past the end
    const int count = rows * A;
    float* __restrict__ dst = mu + (size_t)row0 * A;
    // float f = r A + col of the range sits at r S + col: (r, col) advance by 64 floats without a division
    const int dr = 64 / A, dc = 64 - dr * A;
    int r = lane / A, col = lane - r * A;
    for (int f = lane; f < count; f += 64) {
        dst[f] = turn[wave][r * S + col];
        r += dr;
        col += dc;
        if (col >= A) {
            col -= A;
            ++r;
        }
    }
}

static int check_temperature(float tau, const char* who) {
    if (!(tau >= FI_EXPLORE_TAU_MIN && tau <= FI_EXPLORE_TAU_MAX))  // false for NaN
        return fail(FI_ERR_INVALID, std::string(who) + ": temperature " + std::to_string(tau) +
                                        " is not a finite number in [1/64, 64]");
    return FI_OK;
}

static int sample_behaviour_launch(const float* logits, int N, int A, float tau, const float* eps, uint64_t seed, uint64_t draw,
                            int32_t* actions, float* mu, int* nonfinite, hipStream_t s) {
    FI_REQUIRE(logits && actions && mu, "sample_behaviour: null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff - 255, "sample_behaviour: N must be >= 1 (and below 2^31 - 255)");
    FI_REQUIRE(A >= 2 && A <= 64, "sample_behaviour: 2 <= A <= 64");
    FI_TRY(check_temperature(tau, "sample_behaviour"));
    FI_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)mu % 4 == 0 && (uintptr_t)eps % 4 == 0 &&
                   (uintptr_t)actions % 4 == 0 && (uintptr_t)nonfinite % 4 == 0,
               "sample_behaviour: every pointer must be 4-byte aligned");
    // 4 waves of 64 (AMAX + 1) floats: 65,536 bytes of LDS are not enough at AMAX = 64, which takes 2 waves
#define FI_BEHAVE(M, B)                                                                                            \
    hipLaunchKernelGGL((sample_behaviour_kernel<M, B>), dim3((unsigned)((N + (B)-1) / (B))), dim3(B), 0, s, logits, N, A, \
                       tau, eps, seed, draw, actions, mu, nonfinite)
    if (A <= 8) FI_BEHAVE(8, 256);
    else if (A <= 18) FI_BEHAVE(18, 256);
    else if (A <= 32) FI_BEHAVE(32, 256);
    else FI_BEHAVE(64, 128);
#undef FI_BEHAVE
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

extern "C" int fi_sample_behaviour(const float* logits_dev, int N, int A, float temperature, const float* epsilon_dev,
                                   uint64_t seed, uint64_t draw, int32_t* actions_dev, float* mu_dev, int* nonfinite_dev,
                                   void* stream) {
    return fi::sample_behaviour_launch(logits_dev, N, A, temperature, epsilon_dev, seed, draw, actions_dev, mu_dev,
                                       nonfinite_dev, (hipStream_t)stream);
}

// ------------------------------------------------------------------ the handle
using namespace fi;

static int explore_set(fi_actor* a, float tau, const float* eps_host) {
    FI_REQUIRE(a, "explore_set: null actor");
    FI_TRY(check_temperature(tau, "explore_set"));
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    ExploreState& ex = *actor_explore_state(a);
    const size_t N = ai.N;
    bool plain = tau == 1.f;
    for (size_t i = 0; eps_host && i < N; ++i) {
        const float e = eps_host[i];
        if (!(e >= 0.f && e <= 1.f))  // false for NaN
            return fail(FI_ERR_INVALID, "explore_set: epsilon[" + std::to_string(i) + "] = " + std::to_string(e) +
                                            " is not in [0, 1]");
        plain = plain && e == 0.f;
    }
    if (plain) return fi_explore_clear(a);
    FI_HIP_CHECK(hipSetDevice(ai.dev));
    std::vector<float> next(N, 0.f);
    if (eps_host) std::memcpy(next.data(), eps_host, N * sizeof(float));
    for (float** p : {&ex.eps, &ex.mu}) {
        if (*p) continue;
        const size_t bytes = (p == &ex.eps ? N : N * (size_t)ai.A) * sizeof(float);
        FI_TRY(dev_alloc((void**)p, bytes, "explore_set"));
    }
    // in stream order behind every act call enqueued so far: their kernels read the old epsilons
    FI_HIP_CHECK(hipMemcpyAsync(ex.eps, next.data(), N * sizeof(float), hipMemcpyHostToDevice, ai.stream));
    FI_HIP_CHECK(hipStreamSynchronize(ai.stream));
    ex.eps_host.swap(next);
    ex.tau = tau;
    ex.launch = sample_behaviour_launch;
    ex.active = true;
    return FI_OK;
}

extern "C" int fi_explore_set(fi_actor* a, float temperature, const float* epsilon_host) {
    return guarded("explore_set", FI_ERR_OOM, [&] { return explore_set(a, temperature, epsilon_host); });
}

extern "C" int fi_explore_clear(fi_actor* a) {
    FI_REQUIRE(a, "explore_clear: null actor");
    ExploreState& ex = *actor_explore_state(a);
    ex.active = false;
    ex.tau = 1.f;
    ex.eps_host.clear();
    return FI_OK;
}

extern "C" int fi_explore_get(const fi_actor* a, float* temperature, float* epsilon_host, int* active) {
    FI_REQUIRE(a, "explore_get: null actor");
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    const ExploreState& ex = *actor_explore_state(const_cast<fi_actor*>(a));
    if (temperature) *temperature = ex.tau;
    if (epsilon_host)
        for (int i = 0; i < ai.N; ++i) epsilon_host[i] = ex.active ? ex.eps_host[i] : 0.f;
    if (active) *active = ex.active ? 1 : 0;
    return FI_OK;
}

static int no_behaviour(const char* who) {
    return fail(FI_ERR_STATE, std::string(who) + ": the last act call did not draw by fi_explore.h's rule "
                                                 "(fi_explore_set, sample mode, then an act call)");
}

extern "C" int fi_explore_behaviour_dev(fi_actor* a, const float** mu_dev) {
    FI_REQUIRE(a && mu_dev, "explore_behaviour_dev: null argument");
    *mu_dev = nullptr;
    const ExploreState& ex = *actor_explore_state(a);
    if (!ex.mu_valid) return no_behaviour("explore_behaviour_dev");
    *mu_dev = ex.mu;
    return FI_OK;
}

extern "C" int fi_explore_read_behaviour(fi_actor* a, float* dst, size_t n) {
    FI_REQUIRE(a && dst, "explore_read_behaviour: null argument");
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    const ExploreState& ex = *actor_explore_state(a);
    const size_t want = (size_t)ai.N * ai.A;
    FI_REQUIRE(n == want, "explore_read_behaviour: n != num_envs * num_actions = " + std::to_string(want));
    if (!ex.mu_valid) return no_behaviour("explore_read_behaviour");
    FI_HIP_CHECK(hipSetDevice(ai.dev));
    FI_HIP_CHECK(hipMemcpyAsync(dst, ex.mu, n * sizeof(float), hipMemcpyDeviceToHost, ai.stream));
    FI_HIP_CHECK(hipStreamSynchronize(ai.stream));
    return FI_OK;
}
