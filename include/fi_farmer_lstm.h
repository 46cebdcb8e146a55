/* fi_farmer_lstm.h -- C ABI of the numeric modes of FarmerLstm's LSTM (libfi_learner.so). The LSTM of
 * fi_farmer.h computes in fp32: the input projection on the fp32 MFMA GEMM, the two recurrences on packed-fp32
 * FMAs with W_hh in registers, one workgroup per 1, 2 or 4 batch rows (csrc/farmer.hip). This header adds an
 * opt-in bf16 mode for large batches: the recurrences tiled over 32 batch rows per workgroup on
 * v_mfma_f32_32x32x16_bf16 (csrc/farmer_lstm_bf16.hip), on the convention of fi_mlp.h -- fp32 master parameters,
 * bf16 operand images rebuilt behind every write of the parameters, fp32 accumulation.
 *
 * Nothing of fi_farmer.h changes: a handle that never calls fi_farmer_set_lstm_precision enqueues the kernels it
 * enqueued before and returns the same bits. Status codes and fi_last_error() as fi_learner.h; one thread at a
 * time per handle.
 *
 * The numeric rule of FI_FARMER_LSTM_BF16 (host form in fp64: freeimpala_amd/farmer_lstm.py, lstm_bf16_reference):
 *  1. Operands. Every operand of every LSTM product is bf16, rounded to nearest even from its fp32 source: W_ih,
 *     W_hh, z, the handed-on h and the handed-on dgates. Every accumulation is fp32 in ascending k. Biases, c, dc
 *     and all activation arithmetic are fp32.
 *  2. Projection. xp = rne(z) . rne(W_ih)^T + (b_ih + b_hh), stored fp32. K = 162 is zero-padded to 176 in the
 *     images.
 *  3. Forward step. pre = xp_t + rne(h_{t-1}) . rne(W_hh)^T (the accumulator starts from xp_t);
 *     i, f, o = sigmoid(pre), g = tanh(pre), gate order i, f, g, o; c_t = f c_{t-1} + i g; h_t = o tanh(c_t);
 *     h_{-1} = c_{-1} = 0. Handed on, and stored as hprev[t+1]: rne(h_t) (hprev[0] = 0). Stored gates: rne of the
 *     activated gates, bf16; the cell update itself uses the fp32 gates. Stored c: fp32. cat[:, 0:128] receives
 *     the fp32 h_{T-1}, unrounded.
 *  4. BPTT step. dh = dcat[:, 0:128] at t = T-1, else rne(dgates_{t+1}) . rne(W_hh). In fp32, from the stored bf16
 *     gates and the fp32 c:
 *       do = dh tanh(c_t);  dc += dh o (1 - tanh^2 c_t);  di = dc g;  dg = dc i;  df = dc c_{t-1}
 *       dgates_t = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o));  dc <- dc f
 *     dG_t = rne(dgates_t), stored bf16: those same bits are the next step's operand and the weight gradients'.
 *  5. Weight gradients. gW_ih = dG^T rne(z), gW_hh = dG^T hprev, gb_ih = gb_hh = the fp32 column sums of dG, over
 *     row slices into fp32 slabs that are added in a fixed order. No float atomics: two runs give equal bits.
 *  6. Unchanged: the torso, the criterion and the optimiser stay fp32 exactly as they are, and both modes share
 *     them, the fused small-batch launches included.
 *  7. The images are rebuilt behind every write of the parameters: fi_farmer_set_params and the optimiser.
 *
 * fi_farmer_tensor reports the real byte counts: in bf16 mode "gates", "hprev" and "dG" are bf16 (B T 512 2,
 * B T 128 2, B T 512 2 bytes). It also takes the read-only names "hprev" [B T][128] (row t: h_{t-1}), "cst"
 * [B T][128] fp32, "dG" [B T][512], "xp" [B T][512] fp32 and "dcat" [B][612] fp32 (columns 0..127: the gradient
 * of h_{T-1}) in both modes, and in bf16 mode "wih_bf16" (the W_ih image) and "whh_bf16" (the W_hh image and the
 * W_hh^T image behind it); in fp32 mode those two are FI_ERR_INVALID. fi_farmer_set_profiling /
 * fi_farmer_recurrence_ms bracket the two recurrence kernels of the mode.
 */
#ifndef FI_FARMER_LSTM_H
#define FI_FARMER_LSTM_H

#include "fi_farmer.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fi_farmer_lstm_precision { FI_FARMER_LSTM_FP32 = 0, FI_FARMER_LSTM_BF16 = 1 };

/* Chooses the mode, before the handle's first step or forward; any B >= 1 and T >= 1 is taken. FI_ERR_INVALID for
 * a null handle or an unknown value; FI_ERR_STATE once the handle has stepped or run a forward;
 * FI_ERR_UNSUPPORTED when B T 512 >= 2^31 (the 32-bit offset rule): the handle then stays in fp32. Choosing bf16
 * frees the fp32 gates, hprev and dG and allocates their bf16 forms and the weight images; choosing fp32 again
 * before the first step does the reverse. Parameters set before or after the call are taken either way.         */
int fi_farmer_set_lstm_precision(fi_farmer* f, int precision);
/* The handle's mode; FI_ERR_INVALID for a null handle. */
int fi_farmer_lstm_precision(const fi_farmer* f);

#ifdef __cplusplus
}
#endif
#endif
