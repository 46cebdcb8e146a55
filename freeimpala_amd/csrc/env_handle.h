// env_handle.h -- the built-in environments' handle and what env.hip (Catch, include/fi_env.h, and
// everything both environments share: create, step, tensors, stats, rollout) and breakout.hip
// (Breakout, include/fi_breakout.h) name of each other. Internal: not part of the C ABI. The
// functions of fi_env.h dispatch on `kind` where they launch; a Catch handle launches the kernels
// of env.hip and nothing else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fi_env.h"

enum { FI_ENV_CATCH = 0, FI_ENV_BREAKOUT = 1 };

struct fi_env {
    int dev = 0, N = 0;
    int kind = FI_ENV_CATCH;
    int max_steps = 0;          // Breakout: an episode is truncated there; 0 for Catch
    int state_words = 4;        // 32-bit words of state per environment: 4 (Catch) or 8 (Breakout)
    float gamma = 0.f;
    uint64_t seed = 0;
    char* block = nullptr;  // state | planes | episode_start | rewards | discounts | totals, each 256-byte aligned
    uint4* state = nullptr;
    uint8_t* planes = nullptr;
    uint8_t* start = nullptr;
    float* rewards = nullptr;
    float* discounts = nullptr;
    unsigned long long* totals = nullptr;
    hipEvent_t stepped = nullptr;  // behind the last step's render
};

namespace fi {

// env.hip: allocates a handle of `kind`, writes the first state and renders it
int env_create_handle(int kind, int32_t device, int32_t num_envs, float gamma, uint64_t seed, int32_t max_steps,
                      const char* nm, fi_env** out);

// breakout.hip: the three launches of a Breakout handle; state: N * 8 words, 32-byte aligned
int breakout_init_launch(void* state, int N, uint64_t seed, uint8_t* start, float* rewards, float* discounts,
                         hipStream_t s);
int breakout_update_launch(void* state, const int32_t* actions, int N, float gamma, uint64_t seed, int max_steps,
                           uint8_t* start, float* rewards, float* discounts, void* totals, hipStream_t s);
int breakout_render_launch(const void* state, uint8_t* planes, int N, hipStream_t s);

}  // namespace fi
