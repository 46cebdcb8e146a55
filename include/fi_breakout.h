/* fi_breakout.h -- C ABI of the second built-in device environment (libfi_learner.so): Breakout on
 * 84x84 planes, an environment whose motion is visible only across frames.
 *
 * fi_breakout_create returns an fi_env handle (fi_env.h), and every function of fi_env.h that takes
 * one works on it unchanged: fi_env_destroy, fi_env_num_envs, fi_env_step, fi_env_tensors,
 * fi_env_stepped_event, fi_env_stats (the sum of returns is the sum of the finished episodes'
 * scores), fi_env_rollout, and fi_env_read_state, which returns words 0-3 of the state: r, c, p, k.
 * A step is two launches, the state update and the render, as for Catch. Status codes and
 * fi_last_error() as fi_learner.h; one thread at a time per handle.
 *
 * ---- the rule ---------------------------------------------------------------------------------------
 * All of it is integer arithmetic, so a host reproduces every byte (freeimpala_amd/breakout.py:
 * breakout_reference).
 *   Grid: 21 x 21 cells of 4 x 4 pixels. The paddle is on row 20: centre p in [1, 19], three cells
 * wide. The bricks are on rows 3, 4 and 5, held as a 63-bit mask: bit (row - 3) * 21 + col is set
 * while the brick stands.
 *   State of environment i: the ball's row r and column c, its directions dr, dc in {-1, +1}, p,
 * the step count t of the episode, the episode's score, the brick mask, the episode index k (u32,
 * from 0).
 *   Reset(i, k): (w0, w1, w2, .) = Philox4x32-10 (key = seed, counter = k * N + i, stream 10);
 * c = (w0 * 21) >> 32, p = 1 + ((w1 * 19) >> 32), dc = +1 if w2 & 1 else -1, r = 6, dr = +1,
 * t = 0, score = 0, mask = 2^63 - 1.
 *   Step with action a >= 0, in this order:
 *   1. m = a mod 3 (0 stay, 1 left, 2 right); p <- clamp(p + [m = 2] - [m = 1], 1, 19).
 *   2. nc = c + dc. If nc < 0 or nc > 20: dc <- -dc, nc = c + dc.
 *   3. nr = r + dr. If nr < 0: dr <- +1, nr = r + dr.
 *   4. reward = 0. If 3 <= nr <= 5 and bit (nr, nc) is set: clear it, reward = 1, score += 1,
 *      dr <- -dr, nr = r; a mask that is now 0 becomes 2^63 - 1 again. Else if nr = 20 and
 *      |nc - p| <= 1: dr <- -1, nr = r; if nc < p: dc <- -1; if nc > p: dc <- +1. Else if nr = 20:
 *      the episode ends (a miss).
 *   5. (r, c) <- (nr, nc); t += 1. If t = max_steps the episode ends (truncation, treated as
 *      termination). Ending by both counts once.
 *   6. Ended: discount 0, the totals take one episode and `score`, k += 1, Reset(i, k),
 *      episode_start = 1.
 *   7. Otherwise: discount gamma (the handle's fp32 value), episode_start = 0.
 * The ball may stand on a cell whose brick still stands: only the cell it moves into vertically is
 * tested.
 *   Render, pixel (y, x) in cell (cy, cx) = (y >> 2, x >> 2), the first matching case: 255 if
 * (cy, cx) = (r, c); 128 if cy = 20 and |cx - p| <= 1; 64 if 3 <= cy <= 5 and the brick stands;
 * 0 otherwise.
 *   fi_breakout_create runs Reset(i, 0) and renders the first observation with episode_start = 1,
 * rewards and discounts 0.
 *
 * ---- the state in device memory ---------------------------------------------------------------------
 * Eight 32-bit words per environment, 32-byte aligned: words 0-3 = r, c, p, k (Catch's four);
 * word 4 = bit 0: dc = +1, bit 1: dr = +1; word 5 = t | score << 16; words 6-7 = the mask, low
 * then high. max_steps is in [1, 65535], so t and score fit their 16 bits.
 */
#ifndef FI_BREAKOUT_H
#define FI_BREAKOUT_H

#include <stddef.h>
#include <stdint.h>

#include "fi_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The checks of fi_env_create, and FI_ERR_INVALID for max_steps outside [1, 65535]. */
int fi_breakout_create(int32_t device, int32_t num_envs, float gamma, uint64_t seed, int32_t max_steps,
                       fi_env** out);
/* 0 for a Catch handle (and for NULL) */
int32_t fi_breakout_max_steps(const fi_env* e);
/* Waits for the last step; N values each, any pointer may be NULL. dr and dc are -1 or +1.
 * FI_ERR_INVALID for a Catch handle. */
int fi_breakout_read_state(fi_env* e, int32_t* r, int32_t* c, int32_t* p, uint32_t* k, int32_t* dr, int32_t* dc,
                           int32_t* t, int32_t* score, uint64_t* bricks);
/* Waits for the last step, writes the state of every environment and renders it again;
 * episode_start, rewards, discounts and the totals stay as they are. None of the nine may be NULL.
 * The ranges are those of the states the rule reaches: r in [0, 19], c in [0, 20], p in [1, 19],
 * dr and dc in {-1, +1}, t in [0, max_steps - 1], score in [0, 65535 - (max_steps - t)] (so that
 * it cannot outgrow its 16 bits before the episode ends), bricks in [1, 2^63 - 1]; k is any value.
 * A value outside them is refused with FI_ERR_INVALID, the message naming the field, the
 * environment's index and the value, before anything is written. The caller must have nothing of
 * this environment in flight. FI_ERR_INVALID for a Catch handle. */
int fi_breakout_set_state(fi_env* e, const int32_t* r, const int32_t* c, const int32_t* p, const uint32_t* k,
                          const int32_t* dr, const int32_t* dc, const int32_t* t, const int32_t* score,
                          const uint64_t* bricks);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) ------------------------ */
/* The two launches of a step, alone, as fi_env_update / fi_env_render. state_dev: N * 8 words as
 * above, 32-byte aligned. fi_breakout_update steps them in place with actions_dev (N int32) and
 * writes episode_start (N u8), rewards and discounts (N floats each); totals_dev (nullable, two
 * 64-bit words, 8-byte aligned) takes the finished episodes and the sum of their scores by integer
 * atomic adds. fi_breakout_render writes planes_dev (N, 7056) u8, 16-byte aligned, from the state. */
int fi_breakout_update(void* state_dev, const int32_t* actions_dev, int N, float gamma, uint64_t seed,
                       int32_t max_steps, uint8_t* episode_start_dev, float* rewards_dev, float* discounts_dev,
                       void* totals_dev, void* stream);
int fi_breakout_render(const void* state_dev, uint8_t* planes_dev, int N, void* stream);

#ifdef __cplusplus
}
#endif
#endif
