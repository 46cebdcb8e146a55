/* fi_surrogate.h -- C ABI of the clipped surrogate policy loss on V-trace targets (libfi_learner.so):
 * Schulman et al. 2017, "Proximal policy optimization algorithms"; Luo et al. 2020, "IMPACT: importance
 * weighted asynchronous architectures with clipped target networks". A second objective of the learner
 * beside the V-trace policy gradient: the value targets stay V-trace's, the policy term becomes
 * -min(rho A, clip(rho, 1 - eps, 1 + eps) A), which stops pushing a row whose ratio has already moved far
 * in the direction its advantage asks for. That is what makes sample reuse from a replay ring safe.
 *
 * Nothing of fi_learner.h changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * A handle with the objective on replaces the V-trace launch of a step, and nothing else: PopArt, the
 * column weights, a priority refresh from |vs - V|, the diagnostics, the backward, the gradient norm and
 * the optimisers take its outputs as they took V-trace's.
 *
 * Inputs, as V-trace's: logits pi (T, B, A), mu (T, B, A), act, rew, disc (T, B), values (T + 1, B), the
 * handle's fi_vtrace_hparams (pg_rho_bar is not used), and clip = eps > 0, normalize in {0, 1}, adv_eps.
 *
 *  1. Log-ratio. log pi = log_softmax(pi), log mu = log_softmax(mu), both from one instruction sequence,
 *     so bit-equal logits give log rho = 0 and rho = 1 exactly. a is the action, clamped into [0, A) when
 *     outside: such rows are counted in the `bad` word and the batch is rejected, as on the V-trace path.
 *     log rho = log pi[a] - log mu[a], rho = exp(log rho).
 *  2. Targets, V-trace's own: rho^ = min(rho_bar, rho), c = lambda_ min(c_bar, rho),
 *       acc_t = rho^_t (r_t + g_t V_{t+1} - V_t) + g_t c_t acc_{t+1},  acc_T = 0
 *       vs_t  = V_t + acc_t
 *       A_t   = r_t + g_t vs_{t+1} - V_t,  vs_T = V_T
 *     The pg_adv tensor holds A, without the rho factor V-trace's pg_adv carries.
 *  3. Normalisation (normalize = 1), over the n = T * B rows in fp64: m = mean A, s = sqrt(mean (A - m)^2),
 *     from per-workgroup partial sums of A - pivot in a fixed order (no atomics; the pivot is the one-step
 *     advantage r + g V' - V of row (0, 0), 0 when that is not finite: a variance does not depend on the
 *     shift). A~ = (float)(((double)A - m) / (s + adv_eps)). With normalize = 0, A~ = A. The loss kernel
 *     reads the partial sums from device memory, never m and s by value: steps enqueued without a host
 *     wait equal waited steps.
 *  4. Loss and gradients, sums over (t, b). lo = 1.0f - clip, hi = 1.0f + clip, as floats.
 *       L_pg = sum -min(rho A~, clamp(rho, lo, hi) A~)
 *     A row is clipped when (A~ > 0 and rho > hi) or (A~ < 0 and rho < lo); its policy gradient is 0.
 *     Otherwise g = -rho A~.
 *       dlogits_j = g (1[j = a] - pi_j) + entropy_cost pi_j (log pi_j - sum_k pi_k log pi_k)
 *       dvalue_t  = baseline_cost (V_t - vs_t) for t < T; row T is 0
 *     baseline_loss = sum 1/2 (vs - V)^2 and entropy_loss = sum sum_k pi_k log pi_k, as V-trace's.
 *     The loss partials are [blocks][3] doubles; fi_step_stats.pg_loss is L_pg and total_loss keeps its
 *     formula.
 *  5. Stats block, 32 bytes of device memory, rewritten by every step: uint64 rows, uint64 rows_clipped,
 *     double adv_mean, double adv_std: m and s of A whether or not normalising.
 * With clip huge and normalize = 0, vs, dlogits and dvalue equal V-trace's at pg_rho_bar = 1e30. On an
 * on-policy batch nothing is clipped, whatever eps. No float atomics anywhere: two runs give the same bits.
 *
 * Shapes: any T >= 1, B >= 1, 2 <= A <= 64 with T * B * A < 2^31; no condition on B's alignment.
 *
 * The host form of the whole rule in fp64: freeimpala_amd/surrogate.py (surrogate_reference).
 */
#ifndef FI_SURROGATE_H
#define FI_SURROGATE_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_SURROGATE_CLIP 0.2f
#define FI_SURROGATE_ADV_EPS 1e-8f

typedef struct {
    float clip;         /* eps > 0, finite                                   */
    uint32_t normalize; /* 0 | 1                                             */
    float adv_eps;      /* >= 0, finite: added to s in the normalisation     */
    uint32_t reserved;  /* 0                                                 */
} fi_surrogate_params;  /* 16 bytes                                          */

typedef struct {
    uint32_t enabled;      /* 1 while the next step is a surrogate step                                  */
    uint32_t normalize;    /* the last fi_surrogate_enable's; 0 before any                               */
    float clip;            /* FI_SURROGATE_CLIP before any                                               */
    float adv_eps;         /* FI_SURROGATE_ADV_EPS before any                                            */
    uint64_t rows;         /* the stats block of the last surrogate step: T * B; 0 before any            */
    uint64_t rows_clipped; /* rows whose policy gradient the clip set to 0                               */
    double adv_mean;       /* m of A (NaN when a reward or value of the batch was not finite)            */
    double adv_std;        /* s of A                                                                     */
} fi_surrogate_state;      /* 48 bytes; offsets 0, 4, 8, 12, 16, 24, 32, 40                              */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns the objective on, or replaces the parameters of a handle that has it on. Between any two
 * steps. clip non-finite or <= 0, adv_eps < 0 or non-finite, normalize > 1 or a null pointer:
 * FI_ERR_INVALID before any device call. normalize = 1 on a handle attached to a communicator of more
 * than one rank: FI_ERR_STATE (the moments would need an all-reduce); without normalisation any
 * communicator is fine. The first call allocates the workspace and the stats block.                */
int fi_surrogate_enable(fi_learner* l, const fi_surrogate_params* params);
/* The next step is the V-trace step again, bit for bit. The parameters and the stats block stay.  */
int fi_surrogate_disable(fi_learner* l);
/* Waits for the learner's stream, then reports the parameters and the stats block.                */
int fi_surrogate_get_state(fi_learner* l, fi_surrogate_state* out);
/* The device address of the 32-byte block {uint64 rows, rows_clipped; double adv_mean, adv_std};
 * read it on the learner's stream or behind an event of it. FI_ERR_STATE before fi_surrogate_enable. */
int fi_surrogate_stats_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Bytes of the workspace: d, k, log rho per row and the per-workgroup partials; 0 for a refused shape. */
size_t fi_surrogate_workspace_bytes(int T, int B, int A);
/* Workgroups of the rows kernel and of the loss kernel (one grid: column tiles of 64 times slices of T),
 * the count of loss partials; the scan kernel runs (B + 63) / 64 workgroups. 0 for a refused shape. */
int fi_surrogate_loss_blocks(int T, int B, int A);
/* The whole rule. pi, mu, dlogits 16-byte aligned, every other float / int32 pointer 4-byte, losses,
 * stats_dev and ws 8-byte aligned. vs, adv (T, B); dlogits (T, B, A); dvalue (T + 1, B). losses
 * (nullable): 3 doubles in device memory {L_pg, baseline, entropy}, the partials summed in a fixed
 * order; NaN when an action was outside [0, A). stats_dev (nullable): the 32-byte block. bad
 * (nullable): a device int the out-of-range actions are added to (NULL: a counter inside ws, zeroed
 * by this call). ws: at least fi_surrogate_workspace_bytes(T, B, A).                               */
int fi_surrogate_loss_fp32(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                           const float* disc, const float* val, const fi_vtrace_hparams* hp,
                           const fi_surrogate_params* params, float* vs, float* adv, float* dlogits, float* dvalue,
                           double* losses, void* stats_dev, void* ws, size_t ws_bytes, int* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
