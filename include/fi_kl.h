/* fi_kl.h -- C ABI of the learner's adaptive KL penalty (libfi_learner.so): Schulman et al. 2017,
 * "Proximal policy optimization algorithms", section 4, and APPO's use_kl_loss. The clipped surrogate of
 * fi_surrogate.h / fi_target.h holds its trust region by zeroing the gradient of the taken action's ratio
 * once it has left the band; nothing pulls the other A - 1 probabilities of a row back. This header adds
 * c * KL(q || pi) to the loss, q a reference policy of the very batch, with a coefficient c that adapts to
 * a KL target on the device: a step uses the coefficient the previous step's finalize left, whether or not
 * the host waited in between.
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * Reference q: FI_KL_REF_BEHAVIOUR, the batch's mu logits, or FI_KL_REF_TARGET, the target network's
 * logits of this batch (fi_target.h 1.).
 *
 *  1. Penalty. Per row (t, b), t < T, with pi = softmax(z) and q = softmax(zq):
 *       kl         = sum_j q_j (log q_j - log pi_j)          the direction fi_diag.h reports
 *       dlogits_j += c (pi_j - q_j)                          the exact gradient of c kl with respect to z
 *     (log pi, log q) and (pi, q) come from one instruction sequence on the pair, so bit-equal rows give
 *     kl = 0 and pi_j - q_j = 0 exactly. c = (float)coeff, read from the block where it lies. One fp64 sum
 *     of kl per workgroup. Row T is not touched.
 *  2. Finalize: one workgroup behind the optimiser (profiling tags in order: optimizer, popart_update,
 *     target_update, kl_adapt, weights_bf16).
 *       a. the per-workgroup partials are added in a fixed order: no atomics, two runs give the same bits;
 *       b. rows = T * B, kl_sum and mean_kl = kl_sum / rows are written, always;
 *       c. the optimiser's two flag words are read; if the update was skipped, nothing more is written;
 *       d. updates += 1;
 *       e. if adapt and mean_kl is finite, in fp64 on the widened floats:
 *            mean_kl > band * kl_target:       coeff = min(coeff * factor, coeff_max), raised += 1
 *            else mean_kl < kl_target / band:  coeff = max(coeff / factor, coeff_min), lowered += 1
 *
 * Place in the step: the penalty (tag kl_penalty) runs directly behind the objective's launches -- vtrace,
 * the surrogate's four, or the target's -- and in front of popart_scale and scale_columns, so column
 * weights and importance weights multiply the penalty too: the loss is sum_b w_b (L_b + c kl_b). It is
 * enqueued when the block is on and the reference is behaviour (under either objective), or the reference
 * is target and this step ran a target forward (surrogate objective and target on). A step that does not
 * enqueue it enqueues no kl_adapt either, and the block stays as it is.
 *
 * fi_step_stats keeps its layout and meaning: like the column weights, the penalty is not in total_loss.
 * It is read from the block. After fi_kl_disable the next step is again the step without the penalty, bit
 * for bit; the block stays.
 *
 * Checkpointing: the block is not in fi_learner_save_state's blob. A resuming process calls fi_kl_enable,
 * fi_kl_set_coeff, fi_learner_load_state.
 *
 * Communicators: a fixed coefficient (adapt = 0) is accepted on any communicator. adapt = 1 on more than
 * one rank is refused with FI_ERR_STATE, as fi_popart_enable is: each rank would see its own shard's mean,
 * and the replicas' coefficients would part.
 *
 * Shapes: as fi_surrogate.h (A in 2 .. 64, T * B * A < 2^31). The host form of the rule in fp64:
 * freeimpala_amd/kl.py (kl_reference, adapt_reference).
 */
#ifndef FI_KL_H
#define FI_KL_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_KL_REF_BEHAVIOUR 0u
#define FI_KL_REF_TARGET 1u

#define FI_KL_COEFF 1.0f            /* APPO's kl_coeff                                      */
#define FI_KL_TARGET 0.01f          /* APPO's kl_target                                     */
#define FI_KL_BAND 1.5f             /* the PPO paper's                                      */
#define FI_KL_FACTOR 2.0f           /* the PPO paper's                                      */
#define FI_KL_COEFF_MIN 9.5367431640625e-07f /* 2^-20: ten halvings of 1.0 stay exact       */
#define FI_KL_COEFF_MAX 1048576.0f  /* 2^20                                                 */

typedef struct {
    uint32_t reference; /* FI_KL_REF_BEHAVIOUR or FI_KL_REF_TARGET                          */
    uint32_t adapt;     /* 0: the coefficient stays; 1: rule 2.e                            */
    float coeff;        /* initial value, finite, >= 0                                      */
    float kl_target;    /* > 0                                                              */
    float band;         /* > 1                                                              */
    float factor;       /* > 1                                                              */
    float coeff_min;    /* 0 < coeff_min <= coeff_max                                       */
    float coeff_max;
} fi_kl_params;         /* 32 bytes                                                         */

typedef struct {
    double coeff;     /* the coefficient c                                                  */
    double mean_kl;   /* mean of kl over the rows of the last penalised step                */
    double kl_sum;    /* sum of kl, unscaled                                                */
    uint64_t rows;    /* rows of the last penalised step                                    */
    uint64_t updates; /* finalizes whose update was not skipped                             */
    uint32_t raised;  /* adaptations upwards                                                */
    uint32_t lowered; /* adaptations downwards                                              */
} fi_kl_stats;        /* 48 bytes, the device block's layout; offsets 0, 8, 16, 24, 32, 40, 44 */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns the penalty on. The first call allocates the block and the workspace and writes coeff; a later
 * call replaces the parameters but keeps the block's coeff (and turns a disabled block on again). A null
 * pointer, a non-finite or negative coeff, kl_target <= 0, band <= 1, factor <= 1, bounds that are not
 * 0 < coeff_min <= coeff_max (or not finite), an unknown reference or adapt > 1: FI_ERR_INVALID before any
 * device call. FI_ERR_STATE: reference target on a handle where fi_target_enable was never called; adapt
 * on a communicator of more than one rank.                                                         */
int fi_kl_enable(fi_learner* l, const fi_kl_params* params);
int fi_kl_disable(fi_learner* l);
/* The block's coeff <- c (finite, >= 0), ordered behind the steps already enqueued. FI_ERR_STATE before
 * fi_kl_enable.                                                                                    */
int fi_kl_set_coeff(fi_learner* l, double c);
/* Waits for the learner's stream, then reports the parameters (coeff: the value fi_kl_enable was last
 * given), the block and whether the penalty is on (each pointer nullable). FI_ERR_STATE before
 * fi_kl_enable.                                                                                    */
int fi_kl_get_state(fi_learner* l, fi_kl_params* params, fi_kl_stats* stats, uint32_t* enabled);
/* The device address of the 48-byte block. Read it on the learner's stream or behind an event of it.
 * FI_ERR_STATE before fi_kl_enable.                                                                */
int fi_kl_state_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Bytes of the workspace: one fp64 partial per workgroup; 0 for a refused shape.                   */
size_t fi_kl_workspace_bytes(int T, int B, int A);
/* Rule 1. pi, q (T * B * A floats each, read) and dlogits (read and written) 16-byte aligned; state_dev
 * (48 bytes: coeff is read) and ws (at least fi_kl_workspace_bytes(T, B, A), written) 8-byte aligned. */
int fi_kl_penalty_fp32(int T, int B, int A, const float* pi, const float* q, float* dlogits, const void* state_dev, void* ws,
                       size_t ws_bytes, void* stream);
/* Rule 2 on the partials fi_kl_penalty_fp32 left in ws for the same shape. params: checked as
 * fi_kl_enable checks them. skip (nullable): two device ints, the optimiser's flag words; without them
 * the update counts as made.                                                                       */
int fi_kl_finalize(int T, int B, int A, const fi_kl_params* params, void* state_dev, const void* ws, size_t ws_bytes,
                   const int* skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif
