/* fi_popart.h -- C ABI of PopArt value normalisation on a learner handle (libfi_learner.so):
 * Hessel et al. 2018, "Multi-task deep reinforcement learning with PopArt"; van Hasselt et al. 2016,
 * "Learning values across many orders of magnitude". The value head predicts a normalised value n,
 * the statistics mu, sigma of the V-trace targets are tracked, and each time they move the head's
 * weights are rewritten so that the unnormalised output sigma * n + mu is preserved.
 *
 * Nothing of fi_learner.h changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * State per learner handle, in device memory, 32 bytes: double mu, nu, sigma; uint64_t updates.
 * After fi_popart_enable: mu = 0, nu = 1, sigma = 1, updates = 0. Every kernel reads the state from
 * that block, never by value: an asynchronously enqueued step sees the statistics the previous
 * enqueued step left, with no host wait. The statistics of step k are used throughout step k (its
 * denormalisation and its gradient scale) and move once, behind its optimiser.
 *
 * With mu_f = (float)mu and sigma_f = (float)sigma, one step on a handle with PopArt on:
 *  1. Denormalise, behind the forward and before V-trace: values[i] = fmaf(sigma_f, values[i], mu_f)
 *     in place over all (T+1) * B entries. From here on `values` holds unnormalised values: V-trace,
 *     a priority refresh, the diagnostics and the "values" tensor all see those.
 *  2. V-trace, unchanged: vs, pg_adv, the losses and dlogits are those of the unnormalised values
 *     (the policy gradient keeps unnormalised advantages).
 *  3. Scale the value gradient, behind V-trace and in front of the column weights:
 *     dvalue[i] = dvalue[i] / sigma_f for i < T * B; row T is not touched. PopArt's loss is
 *     1/2 (n - (vs - mu) / sigma)^2 with gradient (v - vs) / sigma in n; V-trace delivers d/dv, so
 *     one division by sigma gives d/dn. The reported losses stay V-trace's.
 *  4. Backward, all-reduce wait, gradient norm, optimiser: unchanged.
 *  5. Update and preserve, behind the optimiser, in two launches.
 *     Moments: S1 = sum vs, S2 = sum vs^2 over the T * B targets, in fp64, as one pair of partials
 *     per workgroup, every sum in a fixed order.
 *     Finalize, one workgroup: adds the partials in a fixed order. It does nothing -- the state and
 *     the head are left bit for bit -- when the optimiser's skip flags are set (skip[0] | skip[1],
 *     the words the optimiser kernels read: a rejected batch or a non-finite gradient norm) or when
 *     S1 or S2 is not finite. Otherwise, in fp64, with n = T * B:
 *       mu'    = (1 - beta) mu + beta S1 / n
 *       nu'    = (1 - beta) nu + beta S2 / n
 *       sigma' = clamp(sqrt(max(nu' - mu'^2, 0)), sigma_min, sigma_max)
 *     and for the value column of the heads (H weights w_j, one bias b):
 *       w_j = (float)((double)w_j sigma / sigma')
 *       b   = (float)((sigma (double)b + (mu - mu')) / sigma')
 *     (mu - mu' is taken first, so statistics that do not move -- beta = 0 -- leave b bit for bit.)
 *     It then stores mu', nu', sigma' and updates + 1. The optimiser's moments of these H + 1
 *     parameters are not rescaled, as in the paper.
 * No atomics anywhere: two runs give the same bits.
 *
 * The statistics are configuration-like state and NOT part of fi_learner_save_state's blob: the
 * format stays. A resuming process calls fi_popart_enable, fi_popart_set_state with the saved mu and
 * nu, then fi_learner_load_state, as the fi_train.h recipe does.
 *
 * An actor evaluates the published head as it is: its `values` are normalised n.
 * fi_popart_state_dev hands out the device address of the block for a caller that denormalises them.
 *
 * The host form of the whole rule in fp64: freeimpala_amd/popart.py (popart_reference).
 */
#ifndef FI_POPART_H
#define FI_POPART_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the paper's defaults */
#define FI_POPART_BETA 3e-4
#define FI_POPART_SIGMA_MIN 1e-4
#define FI_POPART_SIGMA_MAX 1e6

typedef struct {
    uint32_t enabled;  /* 0 on a handle that never called fi_popart_enable (then the neutral values below) */
    uint32_t reserved; /* 0                                                                                */
    double beta, sigma_min, sigma_max; /* the last fi_popart_enable's; the defaults before any             */
    double mu, nu, sigma;              /* 0, 1, 1 before any update                                        */
    uint64_t updates;                  /* finalize launches that moved the state (skipped ones excluded)   */
} fi_popart_state;                     /* 64 bytes; offsets 0, 4, 8, 16, ..., 56                           */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns PopArt on, or on a handle that has it on replaces beta and the bounds and keeps the
 * statistics. beta in [0, 1]; 0 < sigma_min <= 1 <= sigma_max, both finite: FI_ERR_INVALID with the
 * number otherwise, before any device call. Between any two steps. The first call allocates the
 * state block and the moments workspace. A handle attached to a communicator of more than one rank
 * is refused with FI_ERR_STATE: per-rank statistics would make the ranks' value heads diverge.
 * There is no disable.                                                                            */
int fi_popart_enable(fi_learner* l, double beta, double sigma_min, double sigma_max);
/* Waits for the learner's stream, then reports the state.                                         */
int fi_popart_get_state(fi_learner* l, fi_popart_state* out);
/* For resume: stores mu, nu and the sigma they imply (the clamp above), keeps `updates`, rewrites no
 * weight. FI_ERR_STATE before fi_popart_enable; a non-finite value or nu < mu^2 is FI_ERR_INVALID. */
int fi_popart_set_state(fi_learner* l, double mu, double nu);
/* The device address of the 32-byte block {double mu, nu, sigma; uint64_t updates}; read it on the
 * learner's stream or behind an event of it. FI_ERR_STATE before fi_popart_enable.                 */
int fi_popart_state_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Workgroups of the moments kernel over n targets, a fixed function of n alone; 0 for n = 0.      */
int fi_popart_plan(size_t n);
/* Bytes of the moments workspace for n targets: one pair of doubles per workgroup.                */
size_t fi_popart_workspace_bytes(size_t n);
/* values[i] = fmaf(sigma_f, values[i], mu_f), i < n. Pointers 16-byte aligned move 16 bytes per
 * lane; any other alignment (4 bytes at least) takes the element-wise path with the same results. */
int fi_popart_denormalize(float* values, size_t n, const void* state_dev, void* stream);
/* dvalue[i] = dvalue[i] / sigma_f, i < n; alignment as above.                                     */
int fi_popart_scale_grad(float* dvalue, size_t n, const void* state_dev, void* stream);
/* Step 5 of the rule on n targets vs: the moments, then the finalize on the H weights w[j * w_stride]
 * and the bias *b. skip_dev: NULL, or the flag words of the optimiser kernels (skip[0] | skip[1]
 * non-zero: nothing is written). ws: at least fi_popart_workspace_bytes(n), 8-byte aligned.        */
int fi_popart_update(const float* vs, size_t n, void* state_dev, float* w, size_t w_stride, int H, float* b,
                     double beta, double sigma_min, double sigma_max, const int* skip_dev, void* ws, size_t ws_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
