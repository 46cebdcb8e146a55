/* fi_env.h -- C ABI of device-resident environments (libfi_learner.so).
 *
 * The last two PCIe crossings of the actor-learner loop removed: an actor handle acts on
 * observations that are in device memory already and only enqueues, the rewards and discounts come
 * from device memory too, and one small built-in environment (Catch on 84x84 planes) gives that
 * path a producer. A whole unroll -- act, environment step, outcome, record, T times -- is then
 * enqueued on the actor's stream without the host waiting once. Status codes and fi_last_error()
 * as fi_learner.h; one thread at a time per handle. Events are hipEvent_t, streams hipStream_t,
 * both passed as void*.
 *
 * ---- act and outcome on device pointers ---------------------------------------------------------
 * A device act call enqueues, on the handle's stream: a wait for ready_event (when not NULL), for
 * planes the stack push straight from the caller's pointers, the forward and the sampling kernel
 * of a host call (fi_actor.h), unchanged, and the record kernels when the handle records
 * (fi_rollout.h; they read the caller's planes or observations), then an event. There is no copy,
 * no staging and no wait: the call returns once this is enqueued. `draw` advances as in a host
 * call, and host and device calls may alternate on one handle: the outputs come from the same
 * kernels on the same rows, so they are the bits a host call on the same bytes returns. The
 * caller's buffers must stay as they are until the event has completed.
 *
 * Refused before anything is enqueued: FI_ERR_INVALID for the other policy's call, for a pointer
 * that is not 16-byte aligned, that is not device memory of the handle's device, or whose
 * allocation ends before the N rows do; FI_ERR_STATE before the first fi_actor_set_params and for
 * the recording refusals of fi_rollout.h (a missing outcome, a second outcome, the completing call
 * of unroll k+1 while unroll k is unreleased). A device act call cannot report rows with NaN / Inf
 * logits itself: they are counted on the device (their action is 0) and fi_actor_sync returns the
 * count.
 *
 * ---- Catch on 84x84 planes ------------------------------------------------------------------------
 * N environments whose whole state is in device memory. All of the rule is integer arithmetic, so
 * a host reproduces every byte (freeimpala_amd/env.py: catch_reference).
 *   Grid: 21 x 21 cells of 4 x 4 pixels. State of environment i: the ball's row r and column c,
 * the paddle's centre p in [1, 19], the episode index k (u32, from 0).
 *   Reset(i, k): (w0, w1, ., .) = Philox4x32-10 (key = seed, counter = k * N + i, stream 9);
 * c = (w0 * 21) >> 32, p = 1 + ((w1 * 19) >> 32), r = 0.
 *   Step with action a >= 0: m = a mod 3 (0 stay, 1 left, 2 right); p <- clamp(p + [m = 2] -
 * [m = 1], 1, 19); r <- r + 1. If r = 20: reward = +1 when |c - p| <= 1 and -1 otherwise,
 * discount = 0, k <- k + 1, Reset(i, k), episode_start = 1. Otherwise reward 0, discount gamma
 * (the handle's fp32 value), episode_start = 0. Every episode lasts exactly 20 steps.
 *   Render, pixel (y, x): 255 if (y >> 2, x >> 2) = (r, c); otherwise 128 if y >> 2 = 20 and
 * |(x >> 2) - p| <= 1; otherwise 0.
 * fi_env_create runs Reset(i, 0) and renders the first observation with episode_start = 1,
 * rewards and discounts 0.
 */
#ifndef FI_ENV_H
#define FI_ENV_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_learner.h"
#include "fi_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the actor on device pointers ------------------------------------------------------------ */
/* planes_dev: N*7056 u8, episode_start_dev: N u8 (Atari handles) */
int fi_actor_act_planes_dev(fi_actor* a, const uint8_t* planes_dev, const uint8_t* episode_start_dev,
                            void* ready_event);
/* obs_dev: N*obs_dim floats (MLP handles) */
int fi_actor_act_obs_dev(fi_actor* a, const float* obs_dev, void* ready_event);
/* The handle's own device outputs: int32[N], float[N*A], float[N], valid until the next act call on
 * the handle, and the event recorded behind the last device call (act or outcome): the last read
 * of the caller's buffers and the last write of the outputs. NULL before the first device call.
 * Any of the four may be NULL. */
int fi_actor_outputs_dev(fi_actor* a, const int32_t** actions_dev, const float** logits_dev,
                         const float** values_dev, void** done_event);
/* fi_rollout_outcome from device memory: N rewards and N discounts, the same state machine. The
 * stream waits for ready_event (nullable), the scatter kernel reads the caller's pointers, and the
 * handle's event is recorded behind it. */
int fi_rollout_outcome_dev(fi_actor* a, const float* rewards_dev, const float* discounts_dev, void* ready_event);
/* Waits for the handle's stream. *nonfinite_rows (nullable): the rows with NaN / Inf logits that
 * device act calls counted since the last sync; FI_ERR_NONFINITE when there were any. */
int fi_actor_sync(fi_actor* a, int64_t* nonfinite_rows);
/* the handle's hipStream_t: where the device calls are enqueued (to record events around them, or
 * to enqueue a producer of the next observation on) */
void* fi_actor_stream(fi_actor* a);

/* ---- the built-in environment ------------------------------------------------------------------- */
typedef struct fi_env fi_env;

int fi_env_create(int32_t device, int32_t num_envs, float gamma, uint64_t seed, fi_env** out);
void fi_env_destroy(fi_env* e);
int32_t fi_env_num_envs(const fi_env* e);
/* One step of all N environments with actions_dev (N int32, device memory of the handle's device,
 * 4-byte aligned), enqueued on stream (NULL: the null stream) behind a wait for ready_event
 * (nullable): the state update, then the render. It rewrites the handle's four tensors and
 * records the handle's event behind them. FI_ERR_INVALID for a bad pointer, before anything is
 * enqueued. */
int fi_env_step(fi_env* e, const int32_t* actions_dev, void* ready_event, void* stream);
/* planes u8[N*7056], episode_start u8[N], rewards float[N], discounts float[N]; every one 256-byte
 * aligned; any output may be NULL */
int fi_env_tensors(fi_env* e, const uint8_t** planes_dev, const uint8_t** episode_start_dev,
                   const float** rewards_dev, const float** discounts_dev);
/* the event recorded behind the last step (or the first render): what a consumer on another stream
 * waits for */
void* fi_env_stepped_event(fi_env* e);
/* waits for the last step; N values each, any may be NULL */
int fi_env_read_state(fi_env* e, int32_t* r, int32_t* c, int32_t* p, uint32_t* k);
/* waits for the last step; finished episodes and the sum of their returns since create, kept on
 * the device by integer adds: exact and independent of order */
int fi_env_stats(fi_env* e, uint64_t* episodes, int64_t* return_sum);

/* ---- the whole unroll enqueued ------------------------------------------------------------------ */
/* n_steps times, on the actor's stream: fi_actor_act_planes_dev on the environment's planes,
 * fi_env_step on the actor's actions, and on a recording handle fi_rollout_outcome_dev on the
 * environment's rewards and discounts. One stream, so no events between the parts; nothing waits.
 * A step that a refusal of the act call concerns is not enqueued: the call stops there and returns
 * that status. *steps_enqueued (nullable): the steps enqueued in full. FI_ERR_INVALID unless the
 * actor is an Atari handle on the environment's device with num_envs environments. */
int fi_env_rollout(fi_env* e, fi_actor* a, int32_t n_steps, int32_t* steps_enqueued);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------------ */
/* The two launches of a step, alone. state_dev: N quadruples (r, c, p, k) of 32-bit words, 16-byte
 * aligned. fi_env_update steps them in place with actions_dev (N int32) and writes episode_start
 * (N u8), rewards and discounts (N floats each); totals_dev (nullable, two 64-bit words, 8-byte
 * aligned) takes the finished episodes and the sum of their returns by integer atomic adds.
 * fi_env_render writes planes_dev (N, 7056) u8, 16-byte aligned, from the state. */
int fi_env_update(void* state_dev, const int32_t* actions_dev, int N, float gamma, uint64_t seed,
                  uint8_t* episode_start_dev, float* rewards_dev, float* discounts_dev, void* totals_dev,
                  void* stream);
int fi_env_render(const void* state_dev, uint8_t* planes_dev, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif
