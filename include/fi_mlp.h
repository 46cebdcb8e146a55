/* fi_mlp.h -- C ABI of the MLP policy's numeric modes (libfi_learner.so). The MLP policy (obs_dim -> hidden
 * -> hidden -> num_actions + 1) computes in exact fp32 on v_mfma_f32_32x32x2_f32 (csrc/gemm_f32.hip); this
 * header adds an opt-in bf16 mode on the convention the Atari policy already follows: fp32 master
 * parameters, bf16 operand images rebuilt behind every write of the parameters, bf16 stored activations,
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16 (csrc/mlp_bf16.hip).
 *
 * Nothing of the older headers changes: a handle that never calls a function of this header enqueues the
 * kernels it enqueued before and returns the same bits. Status codes and fi_last_error() as fi_learner.h;
 * one thread at a time per handle. fi_learner_config and fi_actor_config keep their sizes.
 *
 * The numeric rule of FI_MLP_BF16 (host form in fp64: freeimpala_amd/mlp_bf16.py, mlp_bf16_reference):
 *  1. Operands. Every operand of every product is bf16: round-to-nearest-even of the fp32 parameter (the
 *     rounding of the published bf16 blob), of the fp32 observation, of the fp32 dlogits / dvalue, and the
 *     stored bf16 activation or data gradient. Every accumulation is fp32, in ascending k.
 *  2. Forward. z1 = rne(obs) . rne(W1) + b1, h1 = rne(relu(z1)); z2 = h1 . rne(W2) + b2, h2 = rne(relu(z2));
 *     [logits | value] = h2 . rne(Wh) + bh. Biases are fp32 and are added in fp32 before the ReLU and the
 *     rounding. Layer 2 reads the stored bf16 h1, bit for bit, and the heads the stored h2.
 *  3. Backward. dout = [dlogits | dvalue] (rows past T B without dlogits, as in fp32 mode).
 *       dz2 = rne((rne(dout) . rne(Wh)^T) * [h2 > 0])        dz1 = rne((dz2 . rne(W2)^T) * [h1 > 0])
 *       gWh = h2^T rne(dout)   gW2 = h1^T dz2   gW1 = rne(obs)^T dz1        (fp32, over row slices)
 *       gbh, gb2, gb1 = the fp32 column sums of rne(dout), dz2, dz1: the operand the weight gradient reads
 *     The masks are taken from the stored h1 / h2. The slices' slabs are summed in a fixed order and there
 *     are no float atomics: two runs give the same bits.
 *  4. Stored as bf16: h1, h2, dz1, dz2 (fi_learner_tensor reports their real byte counts, rows * hidden * 2).
 *     fp32 as before: logits, values, dlogits, dvalue, every parameter gradient, the optimiser and
 *     everything downstream of it, so every other header's block sees what it saw.
 *  5. A row's forward result depends on that row alone (fixed k order, nothing split over K), so an actor
 *     in bf16 mode returns the learner's logits and values for the same observation and parameters, bit
 *     for bit.
 *
 * Widths of the bf16 mode: 1 <= obs_dim <= 128, hidden a multiple of 32 in 32 .. 256, 2 <= num_actions <= 64.
 *
 * Place in the step: tags mlp_fwd_fused, mlp_heads_bwd, mlp_wgrad_l2, mlp_dgrad_l2, mlp_wgrad_l1 (with the
 * reduce_slabs of fp32 mode), and weights_bf16 at the end of the step, behind the optimiser and PopArt's
 * update. The gradient buckets of a communicator are handed over at the same places with the same ranges.
 * With a target network (fi_target.h) the step builds the images of theta- in front of the target forward
 * and the parameters' images again behind it (tags target_weights_bf16, target_weights_back).
 *
 * Checkpointing: the mode is configuration, not part of fi_learner_save_state's blob; a resuming process
 * calls the setter before it loads the state.
 */
#ifndef FI_MLP_H
#define FI_MLP_H

#include "fi_actor.h"
#include "fi_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fi_mlp_precision { FI_MLP_FP32 = 0, FI_MLP_BF16 = 1 };

/* Chooses the mode of an MLP learner, before its first step. FI_ERR_INVALID on an Atari handle or an
 * unknown value; FI_ERR_STATE once the handle has stepped; FI_ERR_UNSUPPORTED, with the widths in the
 * message, when bf16 is asked of a width outside the ranges above: the handle then stays in fp32.
 * Choosing bf16 frees the fp32 h1, h2, dz1, dz2 and allocates the bf16 ones and the weight images.  */
int fi_learner_set_mlp_precision(fi_learner* l, int precision);
/* The handle's mode (FI_MLP_FP32 on an Atari handle); FI_ERR_INVALID for a null handle.            */
int fi_learner_mlp_precision(const fi_learner* l);
/* The same choice on an MLP actor, before its first act call. Parameters set before or after it are
 * taken either way: the images follow every fi_actor_set_params / _dev / _ptr.                      */
int fi_actor_set_mlp_precision(fi_actor* a, int precision);

#ifdef __cplusplus
}
#endif
#endif
