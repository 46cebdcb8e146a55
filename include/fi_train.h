/* fi_train.h -- C ABI of the training recipe on a learner handle (libfi_learner.so): RMSProp as a
 * third optimiser, a learning rate that can change between steps (set directly, or annealed
 * linearly), and reward clipping in front of V-trace.
 *
 * Nothing of fi_learner.h changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * The recipe is configuration, like fi_learner_config, and is NOT part of fi_learner_save_state's
 * blob: the blob does not record which optimiser wrote it. A resuming process makes the same
 * fi_train_* calls on its fresh handle and then calls fi_learner_load_state. step_count is in the
 * blob, so a resumed schedule continues at the update it had reached.
 *
 * RMSProp. fi_train_set_rmsprop switches the handle from its configured optimiser to RMSProp. Only
 * while no update has been enqueued (step_count == 0 and nothing in flight): FI_ERR_STATE otherwise.
 * decay and momentum in [0, 1), eps > 0 and finite: FI_ERR_INVALID with the number otherwise. The
 * mean square lives in the slab Adam calls v and the momentum buffer in the slab Adam calls m (both
 * zero on a fresh handle), so fi_learner_state_bytes / save_state / load_state and the tensors
 * "adam_m" / "adam_v" work unchanged. One update, in fp32, element by element, with `scale` and the
 * skip flags exactly those of the Adam and SGD kernels (scale = max_norm / (norm + 1e-6) when the
 * global gradient norm exceeds max_norm > 0, else 1; a rejected batch or a non-finite norm leaves
 * p, v and m as they are):
 *   g' = g * scale
 *   v  = decay * v + (1 - decay) * g' * g'
 *   d  = eps_in_sqrt ? sqrtf(v + eps) : sqrtf(v) + eps      (0: torch / monobeast, 1: TensorFlow)
 *   momentum > 0:  m = momentum * m + g' / d;  p = p - lr * m
 *   momentum == 0: p = p - lr * g' / d;        m is neither read nor written
 *
 * Learning rate. fi_train_set_lr replaces the base rate lr_base (initially fi_learner_config.lr):
 * finite and >= 0, between any two steps. fi_train_set_lr_schedule(lr_end, n_steps), lr_end finite
 * and >= 0, n_steps >= 1, makes the update numbered s run at
 *   lr_s = (float)(lr_base + (lr_end - lr_base) * min(s - 1, n_steps) / n_steps)     (in double)
 * where s = step_count + 1 when the step is enqueued: the 1-based number Adam's bias correction
 * takes. Update 1 runs at lr_base, updates n_steps + 1 and later at lr_end. The rate travels by value
 * as a kernel argument: an asynchronous step keeps the rate it was enqueued with, and a step enqueued
 * behind a skipped one keeps its number and its rate. The schedule applies to Adam, SGD and RMSProp
 * alike. fi_train_clear_lr_schedule returns to the constant lr_base.
 *
 * Reward clipping. fi_train_set_reward_clip(c): c == 0 is off, c > 0 and finite is on, anything
 * else FI_ERR_INVALID. While on, every later step on every path (the resident step included) clamps
 * the learner's rewards tensor in place, behind the ingest and before V-trace:
 *   r > c ? c : (r < -c ? -c : r)
 * by comparison: a NaN stays a NaN (the step is still rejected with FI_ERR_NONFINITE), +-Inf becomes
 * +-c, -0.0 stays -0.0. The clamp is idempotent, so a resident batch stepped twice is clipped once
 * in effect. vs, pg_adv, the losses and a priority refresh all see the clipped rewards, and the
 * "rewards" tensor reads back clipped. While off, nothing is launched.
 *
 * The host form of all three rules in fp64: freeimpala_amd/train.py (rmsprop_reference, lr_at,
 * clip_rewards).
 */
#ifndef FI_TRAIN_H
#define FI_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_TRAIN_OPT_RMSPROP 2 /* fi_train_state.optimizer; 0 / 1 are fi_optimizer's */

typedef struct {
    uint32_t optimizer;   /* fi_optimizer, or FI_TRAIN_OPT_RMSPROP                             */
    uint32_t eps_in_sqrt; /* RMSProp (zero until fi_train_set_rmsprop, as the three below)     */
    float decay, momentum, eps;
    float lr_base, lr_end; /* lr_end and lr_steps: the last schedule set, 0 before any          */
    float lr_next;         /* the rate the next enqueued update gets                            */
    float reward_clip;     /* 0: off                                                            */
    uint32_t schedule_on;
    uint64_t lr_steps;
    uint64_t next_update; /* the number the next enqueued update gets: step_count + 1          */
} fi_train_state;         /* 56 bytes; offsets 0, 4, ..., 36, 40, 48                           */

int fi_train_set_rmsprop(fi_learner* l, float decay, float momentum, float eps, int eps_in_sqrt);
int fi_train_set_lr(fi_learner* l, float lr);
int fi_train_set_lr_schedule(fi_learner* l, float lr_end, uint64_t n_steps);
int fi_train_clear_lr_schedule(fi_learner* l);
int fi_train_set_reward_clip(fi_learner* l, float c);
int fi_train_get_state(fi_learner* l, fi_train_state* out);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) -------------------- */
/* One RMSProp update of n elements by the rule above. m may be NULL when momentum == 0 (it is not
 * touched then). sqnorm_dev: the squared gradient norm, read when max_norm > 0 (NULL allowed
 * otherwise). skip_dev: NULL, or the four flag words of the learner's optimiser kernels: the update
 * is skipped when skip[0] | skip[1] is non-zero, and then counted in skip[2] with its reasons in
 * skip[3]. Pointers 16-byte aligned move 16 bytes per lane; any other alignment (4 bytes at least)
 * takes the element-wise path with the same results.                                              */
int fi_train_rmsprop_update(float* p, const float* g, float* v, float* m, size_t n, float lr, float decay,
                            float momentum, float eps, int eps_in_sqrt, const double* sqnorm_dev, float max_norm,
                            int* skip_dev, void* stream);
/* r[i] clamped to [-c, c] in place by the rule above, i < n; c > 0 and finite.                    */
int fi_train_clip_rewards(float* r, size_t n, float c, void* stream);

#ifdef __cplusplus
}
#endif
#endif
