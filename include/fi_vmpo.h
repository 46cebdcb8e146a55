/* fi_vmpo.h -- C ABI of the V-MPO objective on the learner (libfi_learner.so): Song et al. 2020, "V-MPO:
 * on-policy maximum a posteriori policy optimization for discrete and continuous control". A third objective
 * beside the V-trace policy gradient and the clipped surrogate (fi_surrogate.h). It uses no importance
 * ratio in the policy term: the policy is fitted by weighted maximum likelihood to the better part of the
 * batch's advantages, with weights softmax(A / eta) over that part and a temperature eta that is learned on
 * the device from a dual loss. The value targets and the advantages stay V-trace's (fi_surrogate.h 1., 2.);
 * the trust region against a target network is fi_kl.h's penalty with reference target, unchanged.
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as
 * fi_learner.h; one thread at a time per handle.
 *
 * Inputs: logits pi (T, B, A), act, adv, vs (T, B), values (T + 1, B), the handle's fi_vtrace_hparams (only
 * baseline_cost and entropy_cost are used here), fi_vmpo_params and the device block fi_vmpo_state.
 *
 *  1. Key. a = adv + 0.0f (so -0.0 counts as +0.0), u = bits(a),
 *       key = u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)
 *     the order-preserving map of floats onto unsigned integers. Every comparison below is on keys.
 *  2. Selection. n = T * B, k = max(1, floor((double)top_fraction * n)). tau is the k-th largest key,
 *     D = {rows with key >= key_tau}: ties at tau are all taken, m = |D| >= k. Amax is the float of the
 *     largest key. The selection is exact: a radix select over the key's digits of 11, 11 and 10 bits.
 *  3. Weights. eta is read from the block in device memory, never by value, so steps enqueued without a
 *     host wait equal waited steps. In fp32: x_i = (a_i - Amax) / (float)eta, e_i = expf(x_i) for i in D.
 *     S = sum e_i and W = sum e_i (a_i - Amax) in fp64, from per-workgroup partials added in a fixed order.
 *     psi_i = e_i / S on D and 0 elsewhere.
 *  4. Loss and gradients. The project's losses are sums over (t, b), so the policy term is scaled by n:
 *       L_pg = -n sum_D psi_i log pi(a_i),   g_i = -n psi_i
 *       dlogits_j = g_i (1[j = a] - pi_j) + entropy_cost pi_j (log pi_j - sum_k pi_k log pi_k)
 *       dvalue_t  = baseline_cost (V_t - vs_t) for t < T; row T is 0
 *     baseline_loss and entropy_loss are the surrogate's; the loss partials are [blocks][3] doubles. An
 *     action outside [0, A) is clamped and counted in `bad`, and the batch is rejected, as everywhere.
 *  5. Temperature. With lsm = log(S / m):
 *       loss_eta = eta eps_eta + Amax + eta lsm          d_eta = eps_eta + lsm - W / (S eta)
 *     are written to the block by every step. The update (tag vmpo_eta) is one small launch behind the
 *     optimiser (tags in order: optimizer, popart_update, target_update, kl_adapt, vmpo_eta, weights_bf16).
 *     It does nothing when adapt = 0, when the optimiser's two flag words are set (the words fi_kl_finalize
 *     reads) or when d_eta is not finite. Otherwise one Adam step in fp64 on eta (beta1 0.9, beta2 0.999,
 *     epsilon 1e-8, bias-corrected by updates + 1, moments m1 and m2 in the block), then
 *     eta = max(eta_min, eta) and updates += 1.
 *  6. Non-finite advantages are outside the rule but for one guarantee: any of them makes S, hence every
 *     selected row's gradient, non-finite, and the update is skipped as for any non-finite gradient.
 * No float atomics anywhere; integer atomics build the histograms and the key maximum, whose results do
 * not depend on the order. Two runs give the same bits.
 *
 * Place in the step. A handle with the objective on replaces the V-trace launch by: surrogate_rows and
 * surrogate_scan (vs and the advantages; on the target logits after a target forward when fi_target_enable is
 * on, else on the learner's logits), vmpo_clear, vmpo_hist0, vmpo_hist1, vmpo_hist2, vmpo_sums, vmpo_loss
 * (always on the learner's own logits). With the target on, fi_kl.h's reference target sees this step's
 * target logits. Everything downstream takes the outputs as it took V-trace's. fi_vmpo_enable turns the
 * surrogate objective off and fi_surrogate_enable turns this one off; after fi_vmpo_disable the next step is
 * the V-trace step again, bit for bit. fi_step_stats keeps its layout: pg_loss is L_pg; loss_eta is read
 * from the block.
 *
 * Checkpointing: the block is not in fi_learner_save_state's blob. A resuming process calls
 * fi_vmpo_enable, fi_vmpo_set_eta, fi_learner_load_state (Adam's two moments of eta start again from 0).
 *
 * Communicators: the selection is over the whole batch, so fi_vmpo_enable on a handle attached to a
 * communicator of more than one rank is refused with FI_ERR_STATE, and so is a step of a handle that was
 * attached to one after the objective went on, before anything of that step is enqueued.
 *
 * Shapes: any T >= 1, B >= 1, 2 <= A <= 64 with T * B * A < 2^31. The host form of the rule in fp64:
 * freeimpala_amd/vmpo.py (vmpo_reference, select_reference, eta_step_reference).
 */
#ifndef FI_VMPO_H
#define FI_VMPO_H

#include <stddef.h>
#include <stdint.h>

#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FI_VMPO_TOP_FRACTION 0.5f
#define FI_VMPO_EPS_ETA 0.01f
#define FI_VMPO_ETA_INIT 1.0f
#define FI_VMPO_ETA_MIN 1e-8f
#define FI_VMPO_LR_ETA 1e-3f
/* bytes of workspace fi_vmpo_select_fp32 needs, whatever n: three histograms of 2,048 words, the selection
 * words and 256 pairs of fp64 partials */
#define FI_VMPO_SELECT_WS_BYTES 28928u

typedef struct {
    float top_fraction;   /* f in (0, 1]                                                     */
    float eps_eta;        /* > 0                                                             */
    float eta_init;       /* >= eta_min: the block's eta when it is made                     */
    float eta_min;        /* > 0                                                             */
    float lr_eta;         /* >= 0: Adam's step on eta                                        */
    uint32_t adapt;       /* 0: eta stays; 1: rule 5                                         */
    uint32_t reserved[2]; /* 0                                                               */
} fi_vmpo_params;         /* 32 bytes                                                        */

typedef struct {
    double eta;         /*  0: the temperature                                               */
    double m1;          /*  8: Adam's first moment of d_eta                                  */
    double m2;          /* 16: Adam's second moment                                          */
    uint64_t updates;   /* 24: temperature updates made                                      */
    uint64_t rows;      /* 32: n of the last step                                            */
    uint64_t selected;  /* 40: m of the last step                                            */
    float threshold;    /* 48: the float of key_tau                                          */
    float adv_max;      /* 52: Amax                                                          */
    double loss_eta;    /* 56                                                                */
    double d_eta;       /* 64                                                                */
    double sum_e;       /* 72: S                                                             */
    double sum_ea;      /* 80: W                                                             */
} fi_vmpo_state;        /* 88 bytes, the device block's layout                               */

/* ---- on a learner handle --------------------------------------------------------------------- */
/* Turns the objective on (and the surrogate objective off). The first call allocates the block and the
 * workspaces and writes eta = eta_init; a later call replaces the parameters but keeps the block. A null
 * pointer, top_fraction outside (0, 1], eps_eta <= 0, eta_min <= 0, eta_init < eta_min, lr_eta < 0, any of
 * them non-finite, or adapt > 1: FI_ERR_INVALID before any device call. A communicator of more than one
 * rank: FI_ERR_STATE.                                                                              */
int fi_vmpo_enable(fi_learner* l, const fi_vmpo_params* params);
/* The next step is the V-trace step again, bit for bit. The parameters and the block stay.        */
int fi_vmpo_disable(fi_learner* l);
/* The block's eta <- eta (finite, > 0), ordered behind the steps already enqueued; the rest of the block
 * is kept. FI_ERR_STATE before fi_vmpo_enable.                                                     */
int fi_vmpo_set_eta(fi_learner* l, double eta);
/* Waits for the learner's stream, then reports the parameters, the block and whether the objective is on
 * (each pointer nullable). Before fi_vmpo_enable: the defaults, a zero block and enabled = 0.      */
int fi_vmpo_get_state(fi_learner* l, fi_vmpo_params* params, fi_vmpo_state* state, uint32_t* enabled);
/* The device address of the 88-byte block. Read it on the learner's stream or behind an event of it.
 * FI_ERR_STATE before fi_vmpo_enable.                                                              */
int fi_vmpo_state_dev(fi_learner* l, const void** ptr);

/* ---- stand-alone on device pointers (stream: hipStream_t or NULL) ---------------------------- */
/* Bytes of the workspace of fi_vmpo_loss_fp32 (its first FI_VMPO_SELECT_WS_BYTES are the selection's);
 * 0 for a refused shape.                                                                           */
size_t fi_vmpo_workspace_bytes(int T, int B, int A);
/* Workgroups of the histogram and sums kernels for n rows: a fixed function of n, at most 256; a
 * workgroup takes 2,048 rows per trip of its grid-stride loop. 0 for n outside 1 .. 2^31 - 1.      */
int fi_vmpo_select_blocks(int64_t n);
/* Rules 1 to 3 on n advantages: writes rows, selected, threshold and adv_max into the block and leaves
 * key_tau and the partials of S and W in ws for fi_vmpo_loss_fp32. adv and ws (at least
 * FI_VMPO_SELECT_WS_BYTES; the histograms are read 16 bytes per lane) 16-byte aligned; state_dev (eta is
 * read) 8-byte aligned.                                                                            */
int fi_vmpo_select_fp32(int64_t n, const float* adv, const fi_vmpo_params* params, void* state_dev, void* ws,
                        size_t ws_bytes, void* stream);
/* Rules 4 and 5's two scalars, behind fi_vmpo_select_fp32 on the same adv (n = T * B), state_dev and ws.
 * pi, dlogits and ws 16-byte aligned, every other float / int32 pointer 4-byte, losses and state_dev
 * 8-byte aligned. dlogits (T, B, A); dvalue (T + 1, B). losses (nullable): 3 doubles in device memory
 * {L_pg, baseline, entropy}, NaN when an action was outside [0, A). bad (nullable): a device int the
 * out-of-range actions are added to (NULL: a counter inside ws, zeroed by this call).              */
int fi_vmpo_loss_fp32(int T, int B, int A, const float* pi, const int32_t* act, const float* adv, const float* vs,
                      const float* val, const fi_vtrace_hparams* hp, const fi_vmpo_params* params, void* state_dev,
                      float* dlogits, float* dvalue, double* losses, void* ws, size_t ws_bytes, int* bad, void* stream);
/* Rule 5's update on the block. skip (nullable): two device ints, the optimiser's flag words; without them
 * the update counts as made.                                                                       */
int fi_vmpo_eta_step(void* state_dev, const fi_vmpo_params* params, const int* skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif
