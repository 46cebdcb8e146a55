/* fi_diag.h -- C ABI of the off-policy diagnostics of a learner step (libfi_learner.so): how hard
 * V-trace is working, reduced on the device from the tensors a step leaves there.
 *
 * Nothing of the older headers changes, and the step itself is untouched: the diagnostics run beside
 * it, on request, behind it in the learner's stream. A handle that never asks allocates nothing and
 * enqueues exactly what it enqueued before. Status codes and fi_last_error() as fi_learner.h. One
 * thread at a time per handle.
 *
 * The rule. Inputs: the policy's logits pi[T][B][A] (the first T * B rows of the learner's "logits",
 * whose (T+1)-th row block is the bootstrap), the behaviour logits mu[T][B][A], act[T][B] (int32),
 * rew, disc, vs [T][B], val = the first T * B of "values", and the thresholds rho_bar, c_bar and
 * pg_rho_bar of fi_vtrace_hparams. Per row (t, b), with the log-softmax over the A actions:
 *     lpi = log pi(.), lmu = log mu(.)
 *     lr  = lpi[a] - lmu[a],  rho = e^lr              (a = act[t][b])
 *     kl  = sum_a mu_a (lmu_a - lpi_a)                 (KL(mu | pi) of the row)
 *     Hpi = -sum_a pi_a lpi_a,  Hmu likewise
 *     td  = vs - V
 * A row is skipped, in this order: its action lies outside [0, A) (counted in rows_bad_action);
 * otherwise any of its 2 A logits is not finite (counted in rows_nonfinite). A skipped row enters no
 * sum, no count and no extreme below; rows_used counts the others. n_episode_ends alone runs over all
 * T * B rows. Clip tests are strict: rho > rho_bar, rho > c_bar, rho > pg_rho_bar.
 *
 * The kernel computes a row in fp32 with the same instruction sequence on the pi and the mu side, so a
 * row whose mu is bit-equal to its pi has lr = 0, rho = 1 and kl = 0 exactly: an on-policy batch at
 * the default thresholds (1, 1, 1) reports 0 clipped rows, mean_log_rho = kl_mu_pi = 0 and
 * max_rho = min_rho = ess = 1. Every sum over rows is fp64, the partial sums are added in a fixed
 * order and nothing is accumulated by atomics: two launches on the same inputs return the same bits.
 *
 * fi_train.h's reward clip rewrites the step's rewards in place, so mean_reward is the clipped one.
 * The host reference of the rule: freeimpala_amd/diag.py (offpolicy_reference).
 */
#ifndef FI_DIAG_H
#define FI_DIAG_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fi_offpolicy_diag {
    uint32_t struct_size;       /* sizeof(fi_offpolicy_diag), written by the library                  */
    uint32_t reserved;          /* 0                                                                  */
    uint64_t rows;              /* T * B                                                              */
    uint64_t rows_used;
    uint64_t rows_bad_action;
    uint64_t rows_nonfinite;
    uint64_t n_rho_clipped;     /* used rows with rho > rho_bar                                       */
    uint64_t n_c_clipped;       /* ... rho > c_bar                                                    */
    uint64_t n_pg_clipped;      /* ... rho > pg_rho_bar                                               */
    uint64_t n_episode_ends;    /* rows with disc == 0, skipped ones included                         */
    /* means over the used rows; with rows_used == 0 every double below is NaN                        */
    double mean_log_rho;
    double mean_rho;
    double kl_mu_pi;
    double entropy_pi;
    double entropy_mu;
    double mean_abs_td;         /* mean |vs - V|                                                      */
    double mean_reward;
    double max_rho;
    double min_rho;
    double ess;                 /* (sum rho)^2 / (rows_used * sum rho^2), in (0, 1]                   */
    double explained_variance;  /* 1 - Var(td) / Var(vs), population variances; NaN when Var(vs) == 0 */
} fi_offpolicy_diag;            /* 160 bytes; rows at 8, mean_log_rho at 72                           */

/* Bytes of the workspace fi_diag_offpolicy needs (the partial sums of every workgroup); 0 for a
 * shape it refuses. The workspace needs no initialisation: every word that is read was written by
 * the same call. */
size_t fi_diag_workspace_bytes(int T, int B, int A);
/* The grid the launcher uses for a shape: workgroup (c, s) owns the columns [64 c, 64 c + 64) and the
 * time steps of slice s. FI_ERR_INVALID for a shape fi_diag_offpolicy refuses. */
int fi_diag_plan(int T, int B, int A, int* column_tiles, int* time_slices);

/* The kernels alone on device pointers (stream: hipStream_t or NULL); enqueues only. Writes the
 * summary to *out_dev and, where the pointers are not NULL, per column b the mean of kl
 * (col_kl_dev[b]) and of lr (col_log_rho_dev[b]) over the column's used rows, fp32, NaN for a column
 * with no used row. Refused with nothing launched (FI_ERR_INVALID): T or B < 1, A outside 2 .. 64,
 * T * B * A >= 2^31, pi or mu not 16-byte aligned, out_dev not 8-byte or another pointer not 4-byte
 * aligned, ws not 8-byte aligned or ws_bytes < fi_diag_workspace_bytes(T, B, A). */
int fi_diag_offpolicy(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                      const float* disc, const float* val, const float* vs, const fi_vtrace_hparams* hp,
                      fi_offpolicy_diag* out_dev, float* col_kl_dev, float* col_log_rho_dev, void* ws, size_t ws_bytes,
                      void* stream);

/* On the learner's stream, over the tensors of the most recently enqueued step and with the handle's
 * thresholds: the kernels, an asynchronous copy of the results into pinned host memory and an event
 * behind it. No host wait. The workspace, the result buffers and the event are made by the first
 * call. Every writer of the tensors runs on the same stream, so steps enqueued afterwards do not
 * disturb a pending result. FI_ERR_STATE before the handle's first step. */
int fi_diag_enqueue(fi_learner* l);
/* Waits for the event of the last fi_diag_enqueue alone and copies its results out. col_kl and
 * col_log_rho may be NULL; otherwise n_cols must equal the learner's batch. FI_ERR_STATE when nothing
 * was enqueued. */
int fi_diag_read(fi_learner* l, fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, int32_t n_cols);
/* fi_diag_enqueue, then fi_diag_read. */
int fi_diag_learner(fi_learner* l, fi_offpolicy_diag* out, float* col_kl, float* col_log_rho, int32_t n_cols);

#ifdef __cplusplus
}
#endif
#endif
