/* fi_upgo.h -- C ABI of the learner's upgoing policy update, UPGO (libfi_learner.so): Vinyals et al. 2019,
 * "Grandmaster level in StarCraft II using multi-agent reinforcement learning", Nature 575, Methods. Every
 * objective of the older headers weighs a row by an advantage against V-trace's target vs, which is cut
 * towards the value head wherever rho falls below 1: a good trajectory that the current policy no longer
 * follows teaches the policy almost nothing. This header adds a second policy-gradient term whose return
 * follows the behaviour trajectory's real rewards for as long as they beat the value estimate, and bootstraps
 * from V as soon as they do not.
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 *  1. Returns. fp32 on the device. Per column b, with r = rewards, g = discounts (gamma (1 - done) already),
 *     V = values (T + 1 rows; after PopArt's denormalisation when PopArt is on):
 *       up_t     = [ r_{t+1} + g_{t+1} V_{t+2} >= V_{t+1} ]     t = 0 .. T-2; a NaN in the comparison: not up
 *       up_{T-1} = 0
 *       G_t      = r_t + g_t (up_t ? G_{t+1} : V_{t+1})          t = T-1 .. 0
 *       AU_t     = G_t - V_t
 *     up depends on the inputs only, so the recurrence is affine in G with input-only coefficients and
 *     is evaluated as a parallel suffix scan over t (csrc/upgo.hip): the sums of one G_t are the serial
 *     loop's sums in another association. Where up_t = 0 the chain is cut, not multiplied by zero: a
 *     non-finite G_{t+1} stays where the serial loop leaves it.
 *  2. Term. Per row (t, b), pi = softmax(logits), mu = softmax(the batch's behaviour logits), a the action:
 *       rho        = min(rho_bar, exp(log pi(a) - log mu(a)))
 *       loss_u    -= rho AU log pi(a)                  rho and AU are constants of the gradient
 *       dlogits_j += coeff rho AU (pi_j - [j == a])
 *     An action outside [0, A) is clamped into it and a non-finite logit goes through the arithmetic, as
 *     in fi_surrogate.h's loss kernel; the objective's own launches count and report such a step. dvalue
 *     is not touched. pi and mu are always the learner's own logits and the batch's mu: with a target
 *     network on (fi_target.h) UPGO does not read the target logits.
 *  3. Finalize: one workgroup adds the per-workgroup fp64 / u64 partials in a fixed order and writes the
 *     block (fi_upgo_stats). No float atomics: two runs give the same bits. coeff and rho_bar are launch
 *     arguments; nothing adapts, so nothing runs behind the optimiser and a skipped update changes nothing.
 *
 * Place in the step: tags upgo_scan, upgo_grad, upgo_finalize, directly behind the objective's launches
 * (vtrace, the surrogate's, the target's or V-MPO's: the term only adds, under any of them) and behind
 * kl_penalty when that is on; in front of popart_scale and scale_columns, so column weights and importance
 * weights multiply it too.
 *
 * fi_step_stats keeps its layout and meaning: like the KL penalty, the term is not in total_loss. It is
 * read from the block. After fi_upgo_disable the next step is again the step without the term, bit for
 * bit; the block stays.
 *
 * Checkpointing: the block is not in fi_learner_save_state's blob; a resuming process calls fi_upgo_enable.
 * Communicators: the term needs no statistic of the batch, so it is accepted on any communicator; the
 * block then holds the rank's own shard.
 *
 * Shapes: as fi_surrogate.h (A in 2 .. 64, T * B * A < 2^31). The host form of the rule in fp64:
 * freeimpala_amd/upgo.py (upgo_reference).
 */
#ifndef FI_UPGO_H
#define FI_UPGO_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_UPGO_COEFF 1.0f   /* c_u                                                             */
#define FI_UPGO_RHO_BAR 1.0f /* AlphaStar's clip of the importance ratio                        */

typedef struct {
    float coeff;   /* c_u: finite, >= 0                                                        */
    float rho_bar; /* finite, > 0                                                              */
} fi_upgo_params;  /* 8 bytes                                                                  */

typedef struct {
    double loss_u;          /* - sum rho AU log pi(a) of the last step, without coeff          */
    double sum_au;          /* sum of AU                                                        */
    uint64_t rows;          /* T * B                                                            */
    uint64_t links_up;      /* the count of up_t = 1                                            */
    uint64_t rows_positive; /* rows with AU > 0                                                 */
} fi_upgo_stats;            /* 40 bytes, the device block's layout; offsets 0, 8, 16, 24, 32   */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns the term on. The first call allocates the block (zeroed) and the workspace; a later call replaces
 * the parameters (and turns a disabled block on again). A null pointer, a non-finite or negative coeff, a
 * non-finite rho_bar or rho_bar <= 0: FI_ERR_INVALID before any device call.                         */
int fi_upgo_enable(fi_learner* l, const fi_upgo_params* params);
int fi_upgo_disable(fi_learner* l);
/* Waits for the learner's stream, then reports the parameters, the block and whether the term is on (each
 * pointer nullable). FI_ERR_STATE before fi_upgo_enable.                                             */
int fi_upgo_get_state(fi_learner* l, fi_upgo_params* params, fi_upgo_stats* stats, uint32_t* enabled);
/* The device address of the 40-byte block. Read it on the learner's stream or behind an event of it.
 * FI_ERR_STATE before fi_upgo_enable.                                                                */
int fi_upgo_state_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Bytes of the workspace: AU (T * B floats) and the partials; 0 for a refused shape.               */
size_t fi_upgo_workspace_bytes(int T, int B, int A);
/* Rule 1 alone. rewards, discounts (T * B floats), values ((T + 1) * B) are read; au (T * B floats) is
 * written; g (T * B floats: G) and up (T * B bytes, 0 or 1) are written when not null. All float
 * pointers 16-byte aligned. T, B >= 1 and (T + 1) * B < 2^31.                                       */
int fi_upgo_returns_fp32(int T, int B, const float* rewards, const float* discounts, const float* values, float* au, float* g,
                         uint8_t* up, void* stream);
/* Rules 1 to 3 onto a caller's dlogits (read and written). logits, mu, dlogits (T * B * A floats), rewards,
 * discounts, values and ws (at least fi_upgo_workspace_bytes(T, B, A)) 16-byte aligned; actions (T * B
 * int32) 4-byte, stats_dev (40 bytes, written) 8-byte aligned. AU stays in the first T * B floats of ws. */
int fi_upgo_term_fp32(int T, int B, int A, const float* logits, const float* mu, const int32_t* actions, const float* rewards,
                      const float* discounts, const float* values, const fi_upgo_params* params, float* dlogits,
                      void* stats_dev, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
