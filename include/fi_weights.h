/* fi_weights.h -- C ABI of per-column loss weights on the learner, and of the two exponents of
 * prioritised replay that need them (libfi_learner.so).
 *
 * fi_prio.h draws a step's replayed columns in proportion to a priority and corrects nothing: the
 * objective is biased towards entries of high TD magnitude. Here the learner gets a weight per batch
 * column, a prioritised ring gets the exponent alpha on the priority it stores and the exponent beta
 * of the importance-sampling weights, and those weights reach the loss through the column weights.
 * Nothing of fi_prio.h, fi_ring.h or fi_learner.h changes: with alpha = 1 and beta = 0 (the values
 * after fi_prio_enable) and no column weights set, every step enqueues the kernels it enqueued
 * before and returns the same bits. Status codes and fi_last_error() as fi_learner.h; one thread at
 * a time per handle.
 *
 * Column weights. The step's loss is a plain sum over the B columns (no division by B); with
 * weights w it becomes sum_b w_b * L_b, so the gradient is exactly w_b times the unweighted one:
 * between V-trace and the backward one kernel multiplies dlogits[t, b, :] and dvalue[t, b], t < T,
 * by w_b in place (row T of dvalue, the bootstrap row, is not touched). vs, pg_adv, logits and
 * values are unweighted, and so is the priority refresh that reads them. In fi_step_stats the
 * three losses and total_loss stay the UNWEIGHTED sums V-trace reports; grad_norm is the norm of
 * the weighted gradient. The weights are not part of fi_learner_save_state.
 *
 * alpha, applied when a priority is stored (the refresh of a prioritised step), with p_b as in
 * fi_prio.h: q_b = FI_PRIO_Q_MAX when p_b is NaN; otherwise q_b = quantise(p_b) when alpha == 1
 * (fi_prio.h's rule, bit for bit) and quantise(powf(p_b, alpha)) in fp32 otherwise. The table
 * therefore holds p^alpha and the draw of fi_prio.h, untouched, samples in proportion to it.
 * init_priority / q_init stay in the table's own domain: quantise(init_priority).
 *
 * beta, the importance weights of one prioritised step of B columns, n_fresh of them fresh. Every
 * number is taken before the call and after the step's q_init fill (n_valid, the window's total Q
 * in u64, the table values). A replayed column c that names entry e with table value q_e:
 *   ratio = (double)q_e * (double)n_valid / (double)Q     (the product is below 2^51: one rounding)
 *   u_c   = powf((float)ratio, -beta)
 * a fresh column has u_c = 1; m = max over all B columns of u_c, and w_c = u_c / m in fp32: the
 * largest weight is exactly 1. The step scales its gradients with w as with column weights. With
 * beta == 0, or n_fresh == B, nothing is computed or launched and the step is fi_prio.h's. The host
 * form of both rules: freeimpala_amd/weights.py (is_weights, td_priorities_alpha).
 */
#ifndef FI_WEIGHTS_H
#define FI_WEIGHTS_H

#include <stddef.h>
#include <stdint.h>

#include "fi_prio.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float alpha;
    float beta;
    uint32_t weights_valid; /* the ring's last prioritised step computed importance weights */
    uint32_t reserved;
} fi_prio_exponents_state;

/* ---- per-column loss weights on the learner ------------------------------------------------ */
/* n must equal the learner's batch B and every w_host[i] be finite and >= 0: FI_ERR_INVALID with the
 * index and the number otherwise, and nothing is stored. Copies into a 4 * B byte device buffer of
 * the handle (allocated on first use) on the learner's stream and waits for the copy. The weights
 * hold for every later step on every path until cleared.                                         */
int fi_learner_set_column_weights(fi_learner* l, const float* w_host, int32_t n);
int fi_learner_clear_column_weights(fi_learner* l);
/* Reads them back (n == B); all 1 after a clear or before any set.                               */
int fi_learner_column_weights(fi_learner* l, float* dst, int32_t n);

/* ---- the exponents of a prioritised ring ---------------------------------------------------- */
/* Both in [0, 1], FI_ERR_INVALID with the number otherwise; FI_ERR_STATE before fi_prio_enable. May
 * be called between any two steps: it changes later refreshes (alpha) and later steps (beta) only
 * and rewrites nothing in the table. After fi_prio_enable: alpha = 1, beta = 0.
 * A prioritised step with beta > 0 on a learner that has column weights set is refused with
 * FI_ERR_STATE before anything is enqueued, every counter unchanged: one source of weights per step. */
int fi_prio_set_exponents(fi_ring* r, float alpha, float beta);
int fi_prio_exponents(const fi_ring* r, fi_prio_exponents_state* out);
/* The weights of the ring's last prioritised step, n = that step's batch; waits for its refresh.
 * All 1 (for any n >= 1) when that step computed none, or no prioritised step was taken yet.      */
int fi_prio_last_weights(fi_ring* r, int32_t n, float* dst);

/* ---- standalone kernels on device pointers (stream: hipStream_t or NULL) -------------------- */
/* dlogits (T, B, A) and the first T rows of dvalue (.., B) times w[b], in place; dlogits 16-byte,
 * dvalue and w 4-byte aligned; T, B, A >= 1 and T * B * (A + 1) < 2^31.                          */
int fi_weights_scale_columns(float* dlogits, float* dvalue, const float* w, int32_t T, int32_t B, int32_t A,
                             void* stream);
/* fi_prio_from_td with alpha in [0, 1]; alpha == 1 is fi_prio_from_td itself.                    */
int fi_prio_from_td_alpha(const float* vs, const float* values, int32_t T, int32_t B, float eta, float alpha,
                          uint32_t* q_out, void* stream);
/* w_out[c], c < B, by the rule above from the entries a draw chose (entries_dev, as
 * fi_prio_fill_columns' entries_out_dev). table, capacity, lo and n_valid as there; chunk_ws as
 * fi_prio_fill_columns left it for the same window on the same stream (not read when n_fresh == B).
 * beta in [0, 1], 0 <= n_fresh <= B, n_valid >= 1 when n_fresh < B.                              */
int fi_prio_is_weights(const uint64_t* entries_dev, int32_t B, int32_t n_fresh, const uint32_t* table, int64_t capacity,
                       uint64_t lo, uint64_t n_valid, const void* chunk_ws, float beta, float* w_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
