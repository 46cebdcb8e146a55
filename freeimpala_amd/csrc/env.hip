// env.hip -- fi_env: Catch on 84x84 planes, N environments whose whole state lives in device
// memory, behind the C ABI of include/fi_env.h (the rule is stated there), and fi_env_rollout,
// which enqueues a whole unroll of a recording actor on its stream without a host wait. The handle
// (env_handle.h) has a kind: what is not Catch's own here -- create, step, tensors, stats, read_state,
// rollout -- serves a Breakout handle too (include/fi_breakout.h) and launches breakout.hip's kernels
// for it; a Catch handle launches exactly the three kernels below.
//
// A step is two launches. env_update_kernel, one lane per environment, moves the paddle and the
// ball, resets finished episodes and writes the step's scalars; env_render_kernel then draws every
// plane from the new state. The render reads state the update wrote: it is a launch of its own, so
// no lane reads what another lane of the same launch overwrites. Every store is an ordinary vector
// store; the two totals are 64-bit integer atomic adds, one pair per wave.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>
#include <vector>

#include "env_handle.h"
#include "fi_common.h"
#include "fi_env.h"
#include "host_util.h"
#include "kernels.h"
#include "records.h"

namespace fi {

namespace {
constexpr int kCells = 21;        // the grid: 21 x 21 cells of 4 x 4 pixels
constexpr int kLastRow = 20;      // the paddle's row; a ball that reaches it ends the episode
constexpr int kPlaneDwords = kPlaneBytes / 4;  // 1,764 = 84 rows of 21 cells: a dword is one cell's pixels of a row
static_assert(kPlaneDwords == 84 * kCells && kPlanePieces * 4 == kPlaneDwords, "a plane dword never leaves its cell");
constexpr size_t kAlign = 256;
size_t round_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
}  // namespace

// Reset(i, k): the ball's column and the paddle's centre of episode k of environment i
__device__ __forceinline__ void env_reset(uint64_t seed, uint32_t k, int N, int i, uint32_t& c, uint32_t& p) {
    const uint4 w = philox4(seed, (uint64_t)k * (uint64_t)N + (uint64_t)i, ST_ENV);
    c = __umulhi(w.x, (uint32_t)kCells);
    p = 1u + __umulhi(w.y, 19u);
}

// ---------------------------------------------------------------- first state
__global__ __launch_bounds__(256) void env_init_kernel(uint4* __restrict__ state, int N, uint64_t seed,
                                                       uint8_t* __restrict__ start, float* __restrict__ rewards,
                                                       float* __restrict__ discounts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t c, p;
    env_reset(seed, 0u, N, i, c, p);
    state[i] = make_uint4(0u, c, p, 0u);
    start[i] = 1;
    rewards[i] = 0.f;
    discounts[i] = 0.f;
}

// ---------------------------------------------------------------- state update
// One lane per environment: 16 bytes of state in and out, 4 + 9 bytes of action and scalars. No
// lane leaves before the wave's sums: every lane of the block takes part in them.
__global__ __launch_bounds__(256) void env_update_kernel(uint4* __restrict__ state, const int32_t* __restrict__ actions,
                                                         int N, float gamma, uint64_t seed,
                                                         uint8_t* __restrict__ start, float* __restrict__ rewards,
                                                         float* __restrict__ discounts,
                                                         unsigned long long* __restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int ended = 0, ret = 0;
    if (i < N) {
        const uint4 s = state[i];
        uint32_t r = s.x, c = s.y, p = s.z, k = s.w;
        const uint32_t m = (uint32_t)actions[i] % 3u;
        int q = (int)p + (m == 2u ? 1 : 0) - (m == 1u ? 1 : 0);
        q = q < 1 ? 1 : (q > 19 ? 19 : q);
        p = (uint32_t)q;
        r += 1u;
        float rew = 0.f, disc = gamma;
        if (r == (uint32_t)kLastRow) {
            const int d = (int)c - q;
            ret = (d >= -1 && d <= 1) ? 1 : -1;
            ended = 1;
            rew = (float)ret;
            disc = 0.f;
            k += 1u;
            r = 0u;
            env_reset(seed, k, N, i, c, p);
        }
        state[i] = make_uint4(r, c, p, k);
        start[i] = (uint8_t)ended;
        rewards[i] = rew;
        discounts[i] = disc;
    }
    if (!totals) return;  // uniform
    const int n_ended = wave_sum(ended), sum = wave_sum(ret);
    if ((threadIdx.x & 63) == 0 && n_ended != 0) {
        atomicAdd(totals, (unsigned long long)n_ended);
        atomicAdd(totals + 1, (unsigned long long)(long long)sum);  // two's complement: the i64 sum
    }
}

// ---------------------------------------------------------------- render
// A pure store stream, 7,056 B per environment: one lane per 16-byte piece, flat over the N * 441
// pieces, so every wave stores 1 KiB contiguously. A piece is four dwords, a dword the four pixels
// of one cell in one pixel row (84 = 21 * 4): dword d of a plane lies in pixel row d / 21 and
// cell column d mod 21, and takes 255, 128 or 0 in all four bytes. The 16 bytes of state an
// environment's 441 lanes read are one line in the L2.
__global__ __launch_bounds__(256) void env_render_kernel(const uint4* __restrict__ state, uint4* __restrict__ planes,
                                                         uint32_t pieces) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= pieces) return;
    const uint32_t env = g / (uint32_t)kPlanePieces, piece = g - env * (uint32_t)kPlanePieces;
    const uint4 s = state[env];
    const uint32_t r = s.x, c = s.y, p = s.z;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = piece * 4u + (uint32_t)j;
        const uint32_t y = d / (uint32_t)kCells, cx = d - y * (uint32_t)kCells, cy = y >> 2;
        const bool ball = cy == r && cx == c;
        const bool paddle = cy == (uint32_t)kLastRow && cx + 1u >= p && cx <= p + 1u;
        v[j] = ball ? 0xffffffffu : (paddle ? 0x80808080u : 0u);
    }
    planes[g] = make_uint4(v[0], v[1], v[2], v[3]);
}

static int env_update_launch(void* state, const int32_t* actions, int N, float gamma, uint64_t seed, uint8_t* start,
                             float* rewards, float* discounts, void* totals, hipStream_t s) {
    FI_REQUIRE(state && actions && start && rewards && discounts, "env_update: null argument");
    FI_REQUIRE(N >= 1, "env_update: N must be >= 1");
    FI_REQUIRE((uintptr_t)state % 16 == 0 && (uintptr_t)actions % 4 == 0 && (uintptr_t)rewards % 4 == 0 &&
                   (uintptr_t)discounts % 4 == 0 && (uintptr_t)totals % 8 == 0,
               "env_update: state must be 16-byte, totals 8-byte, actions, rewards and discounts 4-byte aligned");
    hipLaunchKernelGGL(env_update_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (uint4*)state, actions, N,
                       gamma, seed, start, rewards, discounts, (unsigned long long*)totals);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

static int env_render_launch(const void* state, uint8_t* planes, int N, hipStream_t s) {
    FI_REQUIRE(state && planes, "env_render: null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlanePieces, "env_render: 1 <= N <= 4869582");
    FI_REQUIRE((uintptr_t)state % 16 == 0 && (uintptr_t)planes % 16 == 0,
               "env_render: state and planes must be 16-byte aligned");
    const uint32_t pieces = (uint32_t)N * (uint32_t)kPlanePieces;
    hipLaunchKernelGGL(env_render_kernel, dim3((pieces + 255u) / 256u), dim3(256), 0, s, (const uint4*)state,
                       (uint4*)planes, pieces);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

using namespace fi;

// ------------------------------------------------------------------ the handle (env_handle.h)
static void destroy(fi_env* e) {
    if (!e) return;
    if (e->stepped) {
        (void)hipEventSynchronize(e->stepped);
        (void)hipEventDestroy(e->stepped);
    }
    if (e->block) (void)hipFree(e->block);
    delete e;
}

// the first state of a handle and a step's update, by kind
static int init_launch(fi_env* e, hipStream_t s) {
    if (e->kind == FI_ENV_BREAKOUT)
        return breakout_init_launch(e->state, e->N, e->seed, e->start, e->rewards, e->discounts, s);
    hipLaunchKernelGGL(env_init_kernel, dim3((unsigned)((e->N + 255) / 256)), dim3(256), 0, s, e->state, e->N, e->seed,
                       e->start, e->rewards, e->discounts);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

static int render_launch(fi_env* e, hipStream_t s) {
    if (e->kind == FI_ENV_BREAKOUT) return breakout_render_launch(e->state, e->planes, e->N, s);
    return env_render_launch(e->state, e->planes, e->N, s);
}

static int create(int kind, int32_t device, int32_t num_envs, float gamma, uint64_t seed, int32_t max_steps,
                  const std::string& nm, fi_env** out) {
    FI_REQUIRE(out, nm + ": null argument");
    *out = nullptr;
    FI_REQUIRE(num_envs >= 1 && num_envs <= 0x7fffffff / kPlanePieces, nm + ": 1 <= num_envs <= 4869582");
    FI_REQUIRE(gamma >= 0.f && gamma <= 1.f, nm + ": gamma outside [0, 1]");
    FI_TRY(use_device(device, nm));
    fi_env* e = new (std::nothrow) fi_env();
    FI_REQUIRE(e, nm + ": out of host memory");
    std::unique_ptr<fi_env, void (*)(fi_env*)> guard(e, destroy);
    e->dev = device;
    e->N = num_envs;
    e->gamma = gamma;
    e->seed = seed;
    e->kind = kind;
    e->max_steps = max_steps;
    e->state_words = kind == FI_ENV_BREAKOUT ? 8 : 4;
    const size_t N = (size_t)num_envs;
    const size_t o_planes = round_up(N * (size_t)e->state_words * 4), o_start = o_planes + round_up(N * kPlaneBytes),
                 o_rew = o_start + round_up(N), o_disc = o_rew + round_up(N * sizeof(float)),
                 o_tot = o_disc + round_up(N * sizeof(float)), bytes = o_tot + kAlign;
    FI_TRY(dev_alloc((void**)&e->block, bytes, nm));
    e->state = (uint4*)e->block;
    e->planes = (uint8_t*)(e->block + o_planes);
    e->start = (uint8_t*)(e->block + o_start);
    e->rewards = (float*)(e->block + o_rew);
    e->discounts = (float*)(e->block + o_disc);
    e->totals = (unsigned long long*)(e->block + o_tot);
    FI_HIP_CHECK(hipEventCreateWithFlags(&e->stepped, hipEventDisableTiming));
    FI_HIP_CHECK(hipMemsetAsync(e->block, 0, bytes, nullptr));
    FI_TRY(init_launch(e, nullptr));
    FI_TRY(render_launch(e, nullptr));
    FI_HIP_CHECK(hipEventRecord(e->stepped, nullptr));
    FI_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = guard.release();
    return FI_OK;
}

int fi::env_create_handle(int kind, int32_t device, int32_t num_envs, float gamma, uint64_t seed, int32_t max_steps,
                          const char* nm, fi_env** out) {
    return guarded(nm, FI_ERR_OOM, [&] { return create(kind, device, num_envs, gamma, seed, max_steps, nm, out); });
}

extern "C" int fi_env_create(int32_t device, int32_t num_envs, float gamma, uint64_t seed, fi_env** out) {
    return env_create_handle(FI_ENV_CATCH, device, num_envs, gamma, seed, 0, "env_create", out);
}

extern "C" void fi_env_destroy(fi_env* e) {
    if (!e) return;
    (void)hipSetDevice(e->dev);
    destroy(e);
}

extern "C" int32_t fi_env_num_envs(const fi_env* e) { return e ? e->N : 0; }

// the step's two launches and the event, on s; the caller has checked the actions
static int enqueue_step(fi_env* e, const int32_t* actions, hipStream_t s) {
    if (e->kind == FI_ENV_BREAKOUT)
        FI_TRY(breakout_update_launch(e->state, actions, e->N, e->gamma, e->seed, e->max_steps, e->start, e->rewards,
                                      e->discounts, e->totals, s));
    else
        FI_TRY(env_update_launch(e->state, actions, e->N, e->gamma, e->seed, e->start, e->rewards, e->discounts, e->totals, s));
    FI_TRY(render_launch(e, s));
    FI_HIP_CHECK(hipEventRecord(e->stepped, s));
    return FI_OK;
}

extern "C" int fi_env_step(fi_env* e, const int32_t* actions_dev, void* ready_event, void* stream) {
    FI_REQUIRE(e, "env_step: null environment");
    FI_HIP_CHECK(hipSetDevice(e->dev));
    FI_TRY(check_dev_span(e->dev, actions_dev, (size_t)e->N * sizeof(int32_t), 4, "env_step: actions_dev"));
    if (ready_event) FI_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ready_event, 0));
    return enqueue_step(e, actions_dev, (hipStream_t)stream);
}

extern "C" int fi_env_tensors(fi_env* e, const uint8_t** planes_dev, const uint8_t** episode_start_dev,
                              const float** rewards_dev, const float** discounts_dev) {
    FI_REQUIRE(e, "env_tensors: null environment");
    if (planes_dev) *planes_dev = e->planes;
    if (episode_start_dev) *episode_start_dev = e->start;
    if (rewards_dev) *rewards_dev = e->rewards;
    if (discounts_dev) *discounts_dev = e->discounts;
    return FI_OK;
}

extern "C" void* fi_env_stepped_event(fi_env* e) { return e ? (void*)e->stepped : nullptr; }

extern "C" int fi_env_read_state(fi_env* e, int32_t* r, int32_t* c, int32_t* p, uint32_t* k) {
    FI_REQUIRE(e, "env_read_state: null environment");
    FI_HIP_CHECK(hipSetDevice(e->dev));
    FI_HIP_CHECK(hipEventSynchronize(e->stepped));
    return guarded("env_read_state", FI_ERR_OOM, [&]() -> int {
        const size_t W = (size_t)e->state_words;  // words 0-3 are r, c, p, k in every kind
        std::vector<uint32_t> s((size_t)e->N * W);
        FI_HIP_CHECK(hipMemcpy(s.data(), e->state, s.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < e->N; ++i) {
            if (r) r[i] = (int32_t)s[i * W];
            if (c) c[i] = (int32_t)s[i * W + 1];
            if (p) p[i] = (int32_t)s[i * W + 2];
            if (k) k[i] = s[i * W + 3];
        }
        return FI_OK;
    });
}

extern "C" int fi_env_stats(fi_env* e, uint64_t* episodes, int64_t* return_sum) {
    FI_REQUIRE(e, "env_stats: null environment");
    FI_HIP_CHECK(hipSetDevice(e->dev));
    FI_HIP_CHECK(hipEventSynchronize(e->stepped));
    unsigned long long t[2] = {0, 0};
    FI_HIP_CHECK(hipMemcpy(t, e->totals, sizeof(t), hipMemcpyDeviceToHost));
    if (episodes) *episodes = (uint64_t)t[0];
    if (return_sum) *return_sum = (int64_t)t[1];
    return FI_OK;
}

// ------------------------------------------------------------------ the whole unroll enqueued
extern "C" int fi_env_rollout(fi_env* e, fi_actor* a, int32_t n_steps, int32_t* steps_enqueued) {
    if (steps_enqueued) *steps_enqueued = 0;
    FI_REQUIRE(e && a, "env_rollout: null argument");
    FI_REQUIRE(n_steps >= 0, "env_rollout: n_steps must be >= 0");
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    FI_REQUIRE(ai.arch == FI_ARCH_ATARI, "env_rollout: the environment renders planes: an Atari actor handle takes them");
    FI_REQUIRE(ai.dev == e->dev, "env_rollout: the actor's device " + std::to_string(ai.dev) +
                                     " != the environment's " + std::to_string(e->dev));
    FI_REQUIRE(ai.N == e->N, "env_rollout: the actor's num_envs " + std::to_string(ai.N) + " != the environment's " +
                                 std::to_string(e->N));
    const int32_t* actions = nullptr;
    FI_TRY(fi_actor_outputs_dev(a, &actions, nullptr, nullptr, nullptr));
    FI_HIP_CHECK(hipSetDevice(e->dev));
    // the actor's stream still has to see the environment's last step, enqueued on whatever stream
    FI_HIP_CHECK(hipStreamWaitEvent(ai.stream, e->stepped, 0));
    for (int32_t j = 0; j < n_steps; ++j) {
        FI_TRY(fi_actor_act_planes_dev(a, e->planes, e->start, nullptr));  // a refusal: nothing of step j is enqueued
        FI_TRY(enqueue_step(e, actions, ai.stream));
        if (ai.recording) FI_TRY(fi_rollout_outcome_dev(a, e->rewards, e->discounts, nullptr));
        if (steps_enqueued) *steps_enqueued = j + 1;
    }
    return FI_OK;
}

// ------------------------------------------------------------------ standalone kernels
extern "C" int fi_env_update(void* state_dev, const int32_t* actions_dev, int N, float gamma, uint64_t seed,
                             uint8_t* episode_start_dev, float* rewards_dev, float* discounts_dev, void* totals_dev,
                             void* stream) {
    return env_update_launch(state_dev, actions_dev, N, gamma, seed, episode_start_dev, rewards_dev, discounts_dev,
                             totals_dev, (hipStream_t)stream);
}

extern "C" int fi_env_render(const void* state_dev, uint8_t* planes_dev, int N, void* stream) {
    return env_render_launch(state_dev, planes_dev, N, (hipStream_t)stream);
}
