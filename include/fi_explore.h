/* fi_explore.h -- C ABI of actor exploration (libfi_learner.so): a sampling temperature and one
 * epsilon per environment, with the distribution the action was really drawn from recorded as mu.
 *
 * Nothing of the older headers changes: a handle that never calls fi_explore_set, or has called
 * fi_explore_clear since, allocates nothing new, enqueues exactly what it enqueued before and returns
 * the same bits. Status codes and fi_last_error() as fi_learner.h. One thread at a time per handle.
 *
 * V-trace is right only when a record's mu field holds the distribution its action was drawn from
 * (rho = pi / mu). An exploring actor therefore does not perturb the plain draw and record the
 * policy's logits: one kernel draws the action AND writes the behaviour logits, and the record
 * kernels of fi_rollout.h read those in place of the policy's. The learner takes the log-softmax of
 * whatever A floats sit in mu, so any vector whose softmax is the behaviour distribution is a valid mu.
 *
 * The rule. A handle holds a temperature tau (fp32, finite, 1/64 <= tau <= 64) and one eps_i per
 * environment (fp32, 0 <= eps_i <= 1). Row i with logits l_0 .. l_{A-1}, all finite, in sample mode;
 * every operation is fp32 and every sum runs a = 0 .. A-1 ascending:
 *     m   = max_a l_a
 *     z_a = (l_a - m) / tau                                   (IEEE division)
 *     p_a = expf(z_a)
 *     Z   = sum_a p_a
 *     w_a = fmaf(1 - eps_i, p_a, (eps_i * Z) / A)             (one fused multiply-add)
 *     W   = sum_a w_a
 * The draw is fi_actor.h's, with nothing new drawn: u = (x >> 8) * 2^-24, x the first word of
 * Philox4x32-10 (key = seed, counter = draw * N + i, stream 6). The action is the smallest a whose
 * running sum of w exceeds u * W, or A - 1 if none does. `draw` advances once per act call, as in
 * fi_actor.h. The behaviour logits of the row:
 *     c_i > 0:     mu_a = logf(w_a) - logf(W)        (w_a >= c_i > 0)
 *     c_i == 0:    mu_a = z_a - logf(Z)              (finite where p_a underflows to 0)
 * with c_i = (eps_i * Z) / A as computed in fp32. c_i > 0 whenever eps_i >= 2^-126 (Z >= 1 because p at
 * the maximum is 1, and A <= 64); a smaller positive eps_i whose c_i rounds to 0 draws and records
 * exactly as eps_i == 0 does.
 * Two consequences:
 *   * tau == 1 and eps_i == 0: z_a = l_a - m and w_a = p_a exactly, so W = Z and the action is
 *     bit-equal to fi_sample_actions' on the same logits, seed and draw.
 *   * eps_i == 1: every w_a is Z / A, so the draw is uniform whatever the logits are: the action
 *     depends on u alone and every mu_a is equal.
 * A row that holds a NaN or an Inf behaves as in fi_actor.h: action 0, counted once; its mu row is the
 * policy's logits copied through unchanged, so the learner still rejects the batch.
 * Greedy mode (FI_ACT_GREEDY, the evaluation mode) ignores tau and eps entirely: the plain kernel
 * runs and the policy's logits are recorded, as without this header.
 *
 * The handle. While exploration is active and the mode is FI_ACT_SAMPLE, every act call -- host or
 * device pointers, fi_env_rollout's included -- launches the kernel of this
 * header where it launched fi_actor.h's, and a recording handle writes the behaviour logits into the
 * record's mu field (plane records and MLP records alike). The logits an act call returns and
 * fi_actor_outputs_dev names stay the policy's own. The host reference of the rule:
 * freeimpala_amd/explore.py (behaviour_reference).
 */
#ifndef FI_EXPLORE_H
#define FI_EXPLORE_H

#include <stddef.h>
#include <stdint.h>

#include "fi_actor.h"
#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_EXPLORE_TAU_MIN (1.0f / 64.0f)
#define FI_EXPLORE_TAU_MAX 64.0f

/* Validates first -- FI_ERR_INVALID with the value (and an epsilon's index) in the message, and
 * nothing stored -- then copies the N epsilons (epsilon_host == NULL: all 0) on the actor's stream and
 * waits. Allowed between any two act calls, in the middle of an unroll too: records written before the
 * call hold the old rule's mu, later ones the new rule's. The first call allocates N floats for the
 * epsilons and N * A for the behaviour logits. A call with temperature == 1 and every epsilon == 0
 * is fi_explore_clear. */
int fi_explore_set(fi_actor* a, float temperature, const float* epsilon_host);
/* Back to the plain draw; the buffers stay. */
int fi_explore_clear(fi_actor* a);
/* temperature, epsilon_host (N floats) and active may each be NULL. An inactive handle reports
 * temperature 1, epsilons 0 and active 0. */
int fi_explore_get(const fi_actor* a, float* temperature, float* epsilon_host, int* active);
/* The N * A behaviour logits of the last act call, valid behind the event fi_actor_outputs_dev names
 * (and after any host act call). FI_ERR_STATE unless the last act call ran the rule of this header
 * (exploration active, sample mode). */
int fi_explore_behaviour_dev(fi_actor* a, const float** mu_dev);
/* Copies them to the host (n == N * A) and waits; FI_ERR_STATE as above. */
int fi_explore_read_behaviour(fi_actor* a, float* dst, size_t n);

/* The kernel alone on device pointers (stream: hipStream_t or NULL), beside fi_sample_actions:
 * logits (N, A) fp32, 2 <= A <= 64, N >= 1; epsilon_dev N floats or NULL (all 0); actions (N) int32
 * and mu (N, A) fp32 by the rule above; *nonfinite_dev (nullable, int) is incremented once per row
 * that holds a NaN or an Inf. No shortcut: temperature == 1 with a NULL epsilon runs this kernel too.
 * The temperature is checked as in fi_explore_set; the epsilons are device memory and are not.
 * Every pointer must be 4-byte aligned (FI_ERR_INVALID). */
int fi_sample_behaviour(const float* logits_dev, int N, int A, float temperature, const float* epsilon_dev,
                        uint64_t seed, uint64_t draw, int32_t* actions_dev, float* mu_dev, int* nonfinite_dev,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
