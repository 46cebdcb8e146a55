/* fi_target.h -- C ABI of the learner's target network (libfi_learner.so): Luo et al. 2020, "IMPACT:
 * importance weighted asynchronous architectures with clipped target networks". A slowly moving copy
 * theta- of the learner's own parameters. The clipped surrogate of fi_surrogate.h clips rho = pi / mu
 * against the behaviour policy, which on a replayed column may be many versions old: the clip is then
 * saturated before the learner has moved, and nothing bounds how far one update moves pi from where the
 * learner was a few updates ago. With a target network V-trace's importance weights are taken against the
 * copy (pi_tgt / mu) and the trust region around it (pi / pi_tgt).
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * State: a second fp32 parameter slab theta- of fi_learner_param_count() floats on the learner's device,
 * and a 32-byte stats block {uint64 updates, uint64 rows, double mean_log_r, double mean_sq_log_r}.
 * Parameters: fi_target_params {period K >= 1, tau in (0, 1]}; tau = 1 is a hard copy. Defaults K = 4,
 * tau = 1.
 *
 *  1. Target forward. A step with the target on and the surrogate objective on first computes
 *     tlogits = forward(theta-, batch), (T + 1) * B * A floats of its own, on the learner's own network
 *     and activations (the Atari policy's bf16 weight images are converted from theta-, and converted
 *     back from the parameters before the learner's forward). The target's values go to a scratch buffer
 *     and are not used. Profiling tags: target_weights_bf16, target_forward, target_weights_back (the MLP
 *     has no weight images: target_forward alone). The time counts into the forward phase.
 *  2. Targets, V-trace's with pi_tgt where pi stood: log rho_t = log pi_tgt(a) - log mu(a),
 *     rho^ = min(rho_bar, rho_t), c = lambda_ min(c_bar, rho_t); acc, vs and A follow fi_surrogate.h 2.
 *     They come from the surrogate's rows and scan kernels on (tlogits, mu), so vs and pg_adv of a target
 *     step are bit-equal to what fi_surrogate_loss_fp32(pi := tlogits, mu, ...) writes.
 *  3. Loss. Per row, (log pi(a), log pi_tgt(a)) come from one instruction sequence on the pair, so
 *     bit-equal logits give log r = 0 and r = 1 exactly. r = exp(log r). beta = min(pg_rho_bar,
 *     exp(log rho_t)): the hyper-parameter the plain surrogate leaves unused. A~ is A, or the
 *     batch-normalised A, as fi_surrogate.h 3.; lo = 1.0f - clip, hi = 1.0f + clip as there. A row is
 *     clipped when (A~ > 0 and r > hi) or (A~ < 0 and r < lo); its g is 0, otherwise g = -beta r A~.
 *       L_pg      = sum -beta min(r A~, clamp(r, lo, hi) A~)
 *       dlogits_j = g (1[j = a] - pi_j) + entropy_cost pi_j (log pi_j - sum_k pi_k log pi_k)
 *       dvalue    = baseline_cost (V - vs), row T is 0
 *     The baseline and entropy sums are fi_surrogate.h's. The surrogate's own 32-byte block is still
 *     written (fi_surrogate_get_state keeps working: rows_clipped counts the rows clipped by this rule);
 *     the target block gets rows, mean log r and mean (log r)^2: fp64 sums per workgroup, added in a fixed
 *     order by a one-workgroup kernel. No float atomics: two runs give the same bits.
 *     With pi_tgt bit-equal to pi nothing is clipped and vs, dlogits and dvalue are V-trace's at the
 *     handle's pg_rho_bar.
 *  4. Update: one launch behind the optimiser (and behind PopArt's update, when that is on) of every step
 *     whose update number s satisfies s mod K = 0; s is the count of enqueued updates plus one, like the
 *     bias correction's, and travels by value. theta- <- (tau == 1) ? theta : fmaf(tau, theta - theta-,
 *     theta-). The kernel reads the flag words the optimiser read and writes nothing when the update was
 *     skipped (a rejected batch, a non-finite gradient norm); otherwise one lane adds 1 to `updates`.
 *     Two consequences: a due update that is skipped is not made up until the next multiple of K; and
 *     the period counts enqueued updates, while the handle's version is corrected for skipped updates
 *     when the host next looks, so after a skipped update the two counts differ by the skipped ones.
 *
 * With the target on but the objective "vtrace" no target forward is enqueued and the step equals the
 * plain V-trace step bit for bit; the updates go on. After fi_target_disable the next step is the plain
 * surrogate step (or the V-trace step), bit for bit, and no update is enqueued; theta- and the block stay.
 *
 * Checkpointing: theta- is not in fi_learner_save_state's blob, and fi_learner_set_params /
 * fi_learner_load_state do not touch it. A resuming process calls fi_target_enable, fi_target_set_params,
 * fi_learner_load_state; a process that only wants the target to follow a loaded state calls
 * fi_target_sync after the load.
 *
 * Any communicator is accepted: every rank applies the same update to the same parameters, so the
 * replicas' targets stay equal. Normalisation keeps fi_surrogate_enable's own refusal. Nothing of this
 * header has been run across ranks.
 *
 * Shapes: as fi_surrogate.h. The host form of the rule in fp64: freeimpala_amd/target.py
 * (target_reference, update_reference).
 */
#ifndef FI_TARGET_H
#define FI_TARGET_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"
#include "fi_surrogate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_TARGET_PERIOD 4u
#define FI_TARGET_TAU 1.0f

typedef struct {
    uint32_t period;      /* K >= 1: an update every K-th enqueued update             */
    float tau;            /* in (0, 1], finite; 1: theta- <- theta                    */
    uint32_t reserved[2]; /* 0                                                        */
} fi_target_params;       /* 16 bytes                                                 */

typedef struct {
    uint64_t updates;     /* target updates applied since fi_target_enable                               */
    uint64_t rows;        /* of the last target step: T * B; 0 before any                                */
    double mean_log_r;    /* mean over the rows of log r = log pi(a) - log pi_tgt(a)                     */
    double mean_sq_log_r; /* mean of (log r)^2                                                           */
} fi_target_stats;        /* 32 bytes, the device block's layout; offsets 0, 8, 16, 24                   */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns the target on. The first call allocates theta-, the target logits, the scratch values, the
 * workspace and the block, enqueues theta- <- theta and zeroes the block; a later call only replaces K
 * and tau (and turns a disabled target on again, with theta- as it was left). period 0, tau <= 0, > 1 or
 * non-finite, or a null pointer: FI_ERR_INVALID before any device call.                            */
int fi_target_enable(fi_learner* l, const fi_target_params* params);
int fi_target_disable(fi_learner* l);
/* Enqueues theta- <- theta now; `updates` is not counted. FI_ERR_STATE before fi_target_enable.    */
int fi_target_sync(fi_learner* l);
/* theta- to the host (waits for the learner's stream) and from the host (uploaded before it returns).
 * n must be fi_learner_param_count(). FI_ERR_STATE before fi_target_enable.                        */
int fi_target_get_params(fi_learner* l, float* dst, size_t n);
int fi_target_set_params(fi_learner* l, const float* src, size_t n);
/* Waits for the learner's stream, then reports the parameters, the block and whether the target is on
 * (each pointer nullable). FI_ERR_STATE before fi_target_enable.                                   */
int fi_target_get_state(fi_learner* l, fi_target_params* params, fi_target_stats* stats, uint32_t* enabled);
/* Device addresses: theta- (fp32, fi_learner_param_count() floats: what an evaluation actor reads through
 * fi_actor_set_params_ptr), the target logits (T + 1, B, A) of the last target step, and the 32-byte
 * block. Read them on the learner's stream or behind an event of it. FI_ERR_STATE before fi_target_enable. */
int fi_target_params_dev(fi_learner* l, const void** ptr);
int fi_target_logits_dev(fi_learner* l, const void** ptr);
int fi_target_stats_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Bytes of the workspace: a surrogate workspace and the loss kernel's partials; 0 for a refused shape. */
size_t fi_target_workspace_bytes(int T, int B, int A);
/* The whole rule from 2. on. pi, tgt, mu, dlogits 16-byte aligned, every other float / int32 pointer
 * 4-byte, losses, the two blocks and ws 8-byte aligned. Outputs and nullable arguments as
 * fi_surrogate_loss_fp32's; target_stats_dev (nullable): bytes 8 .. 31 of the 32-byte block are written,
 * `updates` is left as it is. ws: at least fi_target_workspace_bytes(T, B, A).                     */
int fi_target_loss_fp32(int T, int B, int A, const float* pi, const float* tgt, const float* mu, const int32_t* act,
                        const float* rew, const float* disc, const float* val, const fi_vtrace_hparams* hp,
                        const fi_surrogate_params* surrogate_params, float* vs, float* adv, float* dlogits, float* dvalue,
                        double* losses, void* surrogate_stats_dev, void* target_stats_dev, void* ws, size_t ws_bytes,
                        int* bad, void* stream);
/* target <- (tau == 1) ? params : fmaf(tau, params - target, target) over n floats; both 16-byte
 * aligned, never overlapping. skip (nullable): two device ints, the optimiser's flag words; when either
 * is non-zero nothing is written.                                                                  */
int fi_target_update(const float* params, float* target, size_t n, float tau, const int* skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif
