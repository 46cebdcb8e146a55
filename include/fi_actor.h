/* fi_actor.h -- C ABI of batched policy inference with action sampling (libfi_learner.so).
 *
 * The actor side of the loop: a forward-only handle that evaluates the policy the learner
 * publishes (the blob of fi_learner_get_params) on N environments at once and draws their
 * actions on the device. One handle serves N environments; an Atari handle also keeps their
 * 4-frame stacks in device memory, so a step sends one 84x84 plane (7,056 B) per environment.
 * Plain C types only; status codes as fi_learner.h (FI_OK / FI_ERR_*), message in
 * fi_last_error(). A handle owns one HIP stream and is used by one thread at a time, like a
 * learner handle; different handles may act concurrently from different threads.
 *
 * An act call enqueues, on the handle's stream: the H2D copy of the input (through a pinned
 * staging buffer the handle owns), for planes the stack push, the learner's own forward kernels,
 * the sampling kernel, the D2H copy of the outputs; it returns when the outputs are in host
 * memory. Outputs: actions[N] int32, logits[N*A] float (the policy's own logits: what goes into a
 * record's mu field), values[N] float; any of them may be NULL.
 *
 * Stack rule (one step at a time): with episode_start[i] != 0 all four
 * channels of environment i become the new plane; otherwise the channels shift down by one and
 * channel 3 becomes the new plane. A fresh or reset stack is zeros.
 *
 * Sampling rule: environment i of the act call with index `draw` takes x = the first word of
 * Philox4x32-10 (key = seed, counter = draw * N + i, stream 6), u = (x >> 8) * 2^-24. With
 * m = max_a l_a and p_a = expf(l_a - m), Z = sum of p_a in fp32 for a = 0..A-1 ascending; the
 * action is the smallest a whose running sum exceeds u * Z (A - 1 if none does). Greedy mode
 * returns the smallest index of the maximum. `draw` advances by one per act call in either mode.
 * A row whose logits hold a NaN or an Inf gets action 0 and is counted: the call still fills
 * every output, then returns FI_ERR_NONFINITE.
 */
#ifndef FI_ACTOR_H
#define FI_ACTOR_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fi_act_mode { FI_ACT_SAMPLE = 0, FI_ACT_GREEDY = 1 };

typedef struct fi_actor_config {
    uint32_t struct_size; /* sizeof(fi_actor_config), set by the init function              */
    int32_t arch;         /* fi_arch                                                       */
    int32_t num_envs;     /* N >= 1: rows of every act call                                */
    int32_t num_actions;  /* A: 2..64 (MLP), 2..18 (Atari)                                 */
    int32_t obs_dim;      /* MLP: 1..128                                                   */
    int32_t hidden;       /* MLP: 1..4096                                                  */
    int32_t device;       /* HIP device ordinal                                            */
    int32_t mode;         /* fi_act_mode                                                   */
    uint64_t seed;        /* key of the action draws                                       */
} fi_actor_config;

typedef struct fi_actor fi_actor;

void fi_actor_config_init(fi_actor_config* cfg);
int fi_actor_create(const fi_actor_config* cfg, fi_actor** out);
void fi_actor_destroy(fi_actor* a);
size_t fi_actor_param_count(const fi_actor* a);
/* the blob fi_learner_get_params publishes: fp32 (4 * count bytes) or bf16 (2 * count bytes,
 * widened to fp32 exactly as fi_learner_set_params does); any other size is FI_ERR_INVALID */
int fi_actor_set_params(fi_actor* a, const void* blob, size_t bytes, uint64_t version);
uint64_t fi_actor_version(const fi_actor* a);
int fi_actor_set_mode(fi_actor* a, int mode);
/* seed and draw together: `draw` is the index the next act call uses */
int fi_actor_seed(fi_actor* a, uint64_t seed, uint64_t draw);

/* One act call each; host pointers in and out. act_obs serves MLP handles, act_frames and
 * act_planes Atari handles (the wrong call is FI_ERR_INVALID); any of them before the first
 * fi_actor_set_params is FI_ERR_STATE. */
int fi_actor_act_obs(fi_actor* a, const float* obs /* N*obs_dim */, int32_t* actions, float* logits,
                     float* values);
int fi_actor_act_frames(fi_actor* a, const uint8_t* frames /* N*84*84*4, NHWC */, int32_t* actions,
                        float* logits, float* values);
int fi_actor_act_planes(fi_actor* a, const uint8_t* planes /* N*7056 */,
                        const uint8_t* episode_start /* N */, int32_t* actions, float* logits,
                        float* values);
int fi_actor_reset_stacks(fi_actor* a);                            /* all stacks to zero */
/* N*28224 bytes: the stacks the last act_planes ran the policy on (Atari handles) */
int fi_actor_read_stacks(fi_actor* a, uint8_t* dst, size_t bytes);

/* Profiling (scripts/actor_bench.py): with profiling on, every later act call records HIP events
 * between its phases; fi_actor_phase_times returns the mean device ms per call so far of H2D,
 * stack push, forward, sampling and D2H (ms[0..4]; n <= 5 values are written) and the number of
 * calls, and resets the sums. */
int fi_actor_set_profiling(fi_actor* a, int on);
int fi_actor_phase_times(fi_actor* a, float* ms, int n, int* n_calls);

/* Standalone kernels on device pointers (stream: hipStream_t or NULL).
 * fi_push_planes: stacks (N, 84, 84, 4) u8 updated in place from planes (N, 7056) u8 by the stack
 * rule; stacks and planes 16-byte aligned.
 * fi_sample_actions: logits (N, A) fp32, 2 <= A <= 64, actions (N) int32 by the sampling rule;
 * *nonfinite (nullable, int) is incremented once per row that holds a NaN or an Inf. */
int fi_push_planes(uint8_t* stacks_dev, const uint8_t* planes_dev, const uint8_t* episode_start_dev,
                   int N, void* stream);
int fi_sample_actions(const float* logits_dev, int N, int A, int mode, uint64_t seed, uint64_t draw,
                      int32_t* actions_dev, int* nonfinite_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
