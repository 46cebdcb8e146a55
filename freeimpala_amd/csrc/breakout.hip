// breakout.hip -- Breakout on 84x84 planes behind include/fi_breakout.h (the rule is stated there):
// the second built-in environment, one whose ball direction no single plane shows. The handle is
// fi_env (env_handle.h); env.hip creates, steps and rolls it out and calls the three launches here.
//
// A step is two launches, as for Catch. breakout_update_kernel, one lane per environment, moves the
// paddle and the ball, clears a brick, resets finished episodes and writes the step's scalars;
// breakout_render_kernel then draws every plane from the new state, a launch of its own, so no
// lane reads what another lane of the same launch overwrites. Every store is an ordinary vector
// store; the two totals are 64-bit integer atomic adds, one pair per wave.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "env_handle.h"
#include "fi_breakout.h"
#include "fi_common.h"
#include "host_util.h"
#include "kernels.h"
#include "records.h"

namespace fi {

namespace {
constexpr int kCells = 21;       // the grid: 21 x 21 cells of 4 x 4 pixels
constexpr int kLastRow = 20;     // the paddle's row
constexpr int kBrickRow0 = 3;    // bricks on rows 3, 4, 5
constexpr int kBrickRows = 3;
constexpr int kStartRow = 6;     // a reset puts the ball below the bricks, moving down
constexpr uint64_t kFullMask = 0x7fffffffffffffffull;  // 63 = 3 * 21 bricks
constexpr int kStateWords = 8;
constexpr int kMaxStepsLimit = 65535;
static_assert(kBrickRows * kCells == 63, "the bricks fill 63 bits");
static_assert(kPlaneBytes / 4 == 84 * kCells && kPlanePieces * 16 == kPlaneBytes, "a plane dword never leaves its cell");

// the eight words of one environment, unpacked
struct Ball {
    int r, c, p, dr, dc;
    uint32_t k, t, score;
    uint64_t mask;
};
}  // namespace

__device__ __forceinline__ void breakout_load(const uint4* __restrict__ state, int i, Ball& b) {
    const uint4 lo = state[2 * (size_t)i], hi = state[2 * (size_t)i + 1];
    b.r = (int)lo.x;
    b.c = (int)lo.y;
    b.p = (int)lo.z;
    b.k = lo.w;
    b.dc = (hi.x & 1u) ? 1 : -1;
    b.dr = (hi.x & 2u) ? 1 : -1;
    b.t = hi.y & 0xffffu;
    b.score = hi.y >> 16;
    b.mask = (uint64_t)hi.z | ((uint64_t)hi.w << 32);
}

__device__ __forceinline__ void breakout_store(uint4* __restrict__ state, int i, const Ball& b) {
    state[2 * (size_t)i] = make_uint4((uint32_t)b.r, (uint32_t)b.c, (uint32_t)b.p, b.k);
    state[2 * (size_t)i + 1] = make_uint4((b.dc > 0 ? 1u : 0u) | (b.dr > 0 ? 2u : 0u), b.t | (b.score << 16),
                                          (uint32_t)b.mask, (uint32_t)(b.mask >> 32));
}

// Reset(i, k); b.k is the episode that starts
__device__ __forceinline__ void breakout_reset(uint64_t seed, int N, int i, Ball& b) {
    const uint4 w = philox4(seed, (uint64_t)b.k * (uint64_t)N + (uint64_t)i, ST_BREAKOUT);
    b.c = (int)__umulhi(w.x, (uint32_t)kCells);
    b.p = 1 + (int)__umulhi(w.y, 19u);
    b.dc = (w.z & 1u) ? 1 : -1;
    b.r = kStartRow;
    b.dr = 1;
    b.t = 0u;
    b.score = 0u;
    b.mask = kFullMask;
}

// ---------------------------------------------------------------- first state
__global__ __launch_bounds__(256) void breakout_init_kernel(uint4* __restrict__ state, int N, uint64_t seed,
                                                            uint8_t* __restrict__ start, float* __restrict__ rewards,
                                                            float* __restrict__ discounts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    Ball b;
    b.k = 0u;
    breakout_reset(seed, N, i, b);
    breakout_store(state, i, b);
    start[i] = 1;
    rewards[i] = 0.f;
    discounts[i] = 0.f;
}

// ---------------------------------------------------------------- state update
// One lane per environment: 32 bytes of state in and out, 4 + 9 bytes of action and scalars. The
// Philox draw runs only on the lanes whose episode ended. No lane leaves before the wave's sums:
// every lane of the block takes part in them.
__global__ __launch_bounds__(256) void breakout_update_kernel(uint4* __restrict__ state, const int32_t* __restrict__ actions,
                                                              int N, float gamma, uint64_t seed, uint32_t max_steps,
                                                              uint8_t* __restrict__ start, float* __restrict__ rewards,
                                                              float* __restrict__ discounts,
                                                              unsigned long long* __restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int ended = 0, ret = 0;
    if (i < N) {
        Ball b;
        breakout_load(state, i, b);
        const uint32_t m = (uint32_t)actions[i] % 3u;
        int q = b.p + (m == 2u ? 1 : 0) - (m == 1u ? 1 : 0);
        b.p = q < 1 ? 1 : (q > 19 ? 19 : q);
        int nc = b.c + b.dc;
        if (nc < 0 || nc >= kCells) {
            b.dc = -b.dc;
            nc = b.c + b.dc;
        }
        int nr = b.r + b.dr;
        if (nr < 0) {
            b.dr = 1;
            nr = b.r + b.dr;
        }
        float rew = 0.f;
        // nr - 3 in [0, 2] only on a brick row; elsewhere the shift count is masked and the bit unused
        const uint32_t brick_row = (uint32_t)(nr - kBrickRow0);
        const uint32_t bit = (brick_row * (uint32_t)kCells + (uint32_t)nc) & 63u;
        if (brick_row < (uint32_t)kBrickRows && ((b.mask >> bit) & 1ull)) {
            b.mask &= ~(1ull << bit);
            if (b.mask == 0ull) b.mask = kFullMask;
            rew = 1.f;
            b.score += 1u;
            b.dr = -b.dr;
            nr = b.r;
        } else if (nr == kLastRow) {
            const int d = nc - b.p;
            if (d >= -1 && d <= 1) {
                b.dr = -1;
                nr = b.r;
                if (d < 0) b.dc = -1;
                if (d > 0) b.dc = 1;
            } else {
                ended = 1;  // a miss
            }
        }
        b.r = nr;
        b.c = nc;
        b.t += 1u;
        if (b.t == max_steps) ended = 1;  // truncation; with a miss it still counts once
        float disc = gamma;
        if (ended) {
            ret = (int)b.score;
            disc = 0.f;
            b.k += 1u;
            breakout_reset(seed, N, i, b);
        }
        breakout_store(state, i, b);
        start[i] = (uint8_t)ended;
        rewards[i] = rew;
        discounts[i] = disc;
    }
    if (!totals) return;  // uniform
    const int n_ended = wave_sum(ended), sum = wave_sum(ret);  // 64 scores of at most 65,535 each
    if ((threadIdx.x & 63) == 0 && n_ended != 0) {
        atomicAdd(totals, (unsigned long long)n_ended);
        atomicAdd(totals + 1, (unsigned long long)(long long)sum);
    }
}

// ---------------------------------------------------------------- render
// The store stream of env_render_kernel, 7,056 B per environment: one lane per 16-byte piece, flat
// over the N * 441 pieces, so every wave stores 1 KiB contiguously. A piece is four dwords, a dword
// the four pixels of one cell in one pixel row: dword d of a plane lies in pixel row d / 21 and cell
// column d mod 21, and takes 255, 128, 64 or 0 in all four bytes. The brick test is one shift of the
// 64-bit mask. The 32 bytes of state an environment's 441 lanes read are one line in the L2.
__global__ __launch_bounds__(256) void breakout_render_kernel(const uint4* __restrict__ state, uint4* __restrict__ planes,
                                                              uint32_t pieces) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= pieces) return;
    const uint32_t env = g / (uint32_t)kPlanePieces, piece = g - env * (uint32_t)kPlanePieces;
    const uint4 lo = state[2 * (size_t)env], hi = state[2 * (size_t)env + 1];
    const uint32_t r = lo.x, c = lo.y, p = lo.z;
    const uint64_t mask = (uint64_t)hi.z | ((uint64_t)hi.w << 32);
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = piece * 4u + (uint32_t)j;
        const uint32_t y = d / (uint32_t)kCells, cx = d - y * (uint32_t)kCells, cy = y >> 2;
        const bool ball = cy == r && cx == c;
        const bool paddle = cy == (uint32_t)kLastRow && cx + 1u >= p && cx <= p + 1u;
        const uint32_t brick_row = cy - (uint32_t)kBrickRow0;  // wraps above the bricks: then >= 3
        const uint32_t bit = (brick_row * (uint32_t)kCells + cx) & 63u;
        const bool brick = brick_row < (uint32_t)kBrickRows && ((mask >> bit) & 1ull);
        v[j] = ball ? 0xffffffffu : (paddle ? 0x80808080u : (brick ? 0x40404040u : 0u));
    }
    planes[g] = make_uint4(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------- launches
int breakout_init_launch(void* state, int N, uint64_t seed, uint8_t* start, float* rewards, float* discounts,
                         hipStream_t s) {
    FI_REQUIRE(state && start && rewards && discounts && N >= 1, "breakout_init: bad argument");
    hipLaunchKernelGGL(breakout_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (uint4*)state, N, seed,
                       start, rewards, discounts);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int breakout_update_launch(void* state, const int32_t* actions, int N, float gamma, uint64_t seed, int max_steps,
                           uint8_t* start, float* rewards, float* discounts, void* totals, hipStream_t s) {
    FI_REQUIRE(state && actions && start && rewards && discounts, "breakout_update: null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlanePieces, "breakout_update: 1 <= N <= 4869582");
    FI_REQUIRE(max_steps >= 1 && max_steps <= kMaxStepsLimit, "breakout_update: max_steps outside [1, 65535]");
    FI_REQUIRE((uintptr_t)state % 32 == 0 && (uintptr_t)actions % 4 == 0 && (uintptr_t)rewards % 4 == 0 &&
                   (uintptr_t)discounts % 4 == 0 && (uintptr_t)totals % 8 == 0,
               "breakout_update: state must be 32-byte, totals 8-byte, actions, rewards and discounts 4-byte aligned");
    hipLaunchKernelGGL(breakout_update_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (uint4*)state, actions,
                       N, gamma, seed, (uint32_t)max_steps, start, rewards, discounts, (unsigned long long*)totals);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int breakout_render_launch(const void* state, uint8_t* planes, int N, hipStream_t s) {
    FI_REQUIRE(state && planes, "breakout_render: null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlanePieces, "breakout_render: 1 <= N <= 4869582");
    FI_REQUIRE((uintptr_t)state % 32 == 0 && (uintptr_t)planes % 16 == 0,
               "breakout_render: state must be 32-byte, planes 16-byte aligned");
    const uint32_t pieces = (uint32_t)N * (uint32_t)kPlanePieces;
    hipLaunchKernelGGL(breakout_render_kernel, dim3((pieces + 255u) / 256u), dim3(256), 0, s, (const uint4*)state,
                       (uint4*)planes, pieces);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

using namespace fi;

// ------------------------------------------------------------------ the C ABI
extern "C" int fi_breakout_create(int32_t device, int32_t num_envs, float gamma, uint64_t seed, int32_t max_steps,
                                  fi_env** out) {
    if (out) *out = nullptr;
    FI_REQUIRE(max_steps >= 1 && max_steps <= kMaxStepsLimit,
               "breakout_create: max_steps " + std::to_string(max_steps) + " outside [1, 65535]");
    return env_create_handle(FI_ENV_BREAKOUT, device, num_envs, gamma, seed, max_steps, "breakout_create", out);
}

extern "C" int32_t fi_breakout_max_steps(const fi_env* e) { return e && e->kind == FI_ENV_BREAKOUT ? e->max_steps : 0; }

static int require_breakout(const fi_env* e, const std::string& nm) {
    FI_REQUIRE(e, nm + ": null environment");
    FI_REQUIRE(e->kind == FI_ENV_BREAKOUT, nm + ": a Catch handle has no Breakout state: a Breakout handle is needed");
    return FI_OK;
}

extern "C" int fi_breakout_read_state(fi_env* e, int32_t* r, int32_t* c, int32_t* p, uint32_t* k, int32_t* dr,
                                      int32_t* dc, int32_t* t, int32_t* score, uint64_t* bricks) {
    FI_TRY(require_breakout(e, "breakout_read_state"));
    FI_HIP_CHECK(hipSetDevice(e->dev));
    FI_HIP_CHECK(hipEventSynchronize(e->stepped));
    return guarded("breakout_read_state", FI_ERR_OOM, [&]() -> int {
        std::vector<uint32_t> s((size_t)e->N * kStateWords);
        FI_HIP_CHECK(hipMemcpy(s.data(), e->state, s.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < e->N; ++i) {
            const uint32_t* w = s.data() + (size_t)i * kStateWords;
            if (r) r[i] = (int32_t)w[0];
            if (c) c[i] = (int32_t)w[1];
            if (p) p[i] = (int32_t)w[2];
            if (k) k[i] = w[3];
            if (dc) dc[i] = (w[4] & 1u) ? 1 : -1;
            if (dr) dr[i] = (w[4] & 2u) ? 1 : -1;
            if (t) t[i] = (int32_t)(w[5] & 0xffffu);
            if (score) score[i] = (int32_t)(w[5] >> 16);
            if (bricks) bricks[i] = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
        }
        return FI_OK;
    });
}

extern "C" int fi_breakout_set_state(fi_env* e, const int32_t* r, const int32_t* c, const int32_t* p, const uint32_t* k,
                                     const int32_t* dr, const int32_t* dc, const int32_t* t, const int32_t* score,
                                     const uint64_t* bricks) {
    FI_TRY(require_breakout(e, "breakout_set_state"));
    FI_REQUIRE(r && c && p && k && dr && dc && t && score && bricks, "breakout_set_state: null argument");
    const int N = e->N, ms = e->max_steps;
    auto bad = [](const char* field, int i, long long v, const std::string& range) {
        return fail(FI_ERR_INVALID, std::string("breakout_set_state: ") + field + "[" + std::to_string(i) + "] = " +
                                        std::to_string(v) + " outside " + range);
    };
    // every value is checked before anything is written
    for (int i = 0; i < N; ++i) {
        if (r[i] < 0 || r[i] > kLastRow - 1) return bad("r", i, r[i], "[0, 19]");
        if (c[i] < 0 || c[i] >= kCells) return bad("c", i, c[i], "[0, 20]");
        if (p[i] < 1 || p[i] > 19) return bad("p", i, p[i], "[1, 19]");
        if (dr[i] != 1 && dr[i] != -1) return bad("dr", i, dr[i], "{-1, +1}");
        if (dc[i] != 1 && dc[i] != -1) return bad("dc", i, dc[i], "{-1, +1}");
        if (t[i] < 0 || t[i] > ms - 1) return bad("t", i, t[i], "[0, " + std::to_string(ms - 1) + "]");
        const int top = kMaxStepsLimit - (ms - t[i]);
        if (score[i] < 0 || score[i] > top) return bad("score", i, score[i], "[0, " + std::to_string(top) + "]");
        if (bricks[i] < 1 || bricks[i] > kFullMask)
            return fail(FI_ERR_INVALID, "breakout_set_state: bricks[" + std::to_string(i) + "] = " +
                                            std::to_string(bricks[i]) + " outside [1, 9223372036854775807]");
    }
    FI_HIP_CHECK(hipSetDevice(e->dev));
    FI_HIP_CHECK(hipEventSynchronize(e->stepped));
    FI_TRY(guarded("breakout_set_state", FI_ERR_OOM, [&]() -> int {
        std::vector<uint32_t> s((size_t)N * kStateWords);
        for (int i = 0; i < N; ++i) {
            uint32_t* w = s.data() + (size_t)i * kStateWords;
            w[0] = (uint32_t)r[i];
            w[1] = (uint32_t)c[i];
            w[2] = (uint32_t)p[i];
            w[3] = k[i];
            w[4] = (dc[i] > 0 ? 1u : 0u) | (dr[i] > 0 ? 2u : 0u);
            w[5] = (uint32_t)t[i] | ((uint32_t)score[i] << 16);
            w[6] = (uint32_t)bricks[i];
            w[7] = (uint32_t)(bricks[i] >> 32);
        }
        FI_HIP_CHECK(hipMemcpy(e->state, s.data(), s.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return FI_OK;
    }));
    FI_TRY(breakout_render_launch(e->state, e->planes, N, nullptr));
    FI_HIP_CHECK(hipEventRecord(e->stepped, nullptr));
    FI_HIP_CHECK(hipStreamSynchronize(nullptr));
    return FI_OK;
}

// ------------------------------------------------------------------ standalone kernels
// The state pointer is checked to be device memory that holds the N states: a host pointer (an
// fi_env handle passed by mistake, say) is refused instead of being handed to a kernel.
static int check_state(const void* state_dev, int N, const std::string& nm) {
    FI_REQUIRE(state_dev, nm + ": null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlanePieces, nm + ": 1 <= N <= 4869582");
    int dev = 0;
    FI_HIP_CHECK(hipGetDevice(&dev));
    return check_dev_span(dev, state_dev, (size_t)N * kStateWords * 4, 1, nm + ": state_dev");  // the launch checks the alignment
}

extern "C" int fi_breakout_update(void* state_dev, const int32_t* actions_dev, int N, float gamma, uint64_t seed,
                                  int32_t max_steps, uint8_t* episode_start_dev, float* rewards_dev,
                                  float* discounts_dev, void* totals_dev, void* stream) {
    FI_TRY(check_state(state_dev, N, "breakout_update"));
    return breakout_update_launch(state_dev, actions_dev, N, gamma, seed, max_steps, episode_start_dev, rewards_dev,
                                  discounts_dev, totals_dev, (hipStream_t)stream);
}

extern "C" int fi_breakout_render(const void* state_dev, uint8_t* planes_dev, int N, void* stream) {
    FI_TRY(check_state(state_dev, N, "breakout_render"));
    return breakout_render_launch(state_dev, planes_dev, N, (hipStream_t)stream);
}
