/* fi_farmer_act.h -- C ABI of FarmerLstm's acting branch on the MI355X (libfi_learner.so, csrc/farmer_act.hip).
 *
 * FarmerLstmModel.forward(z, x, return_value=False) of the reference is the acting rule of a DouZero-style agent:
 * the rows of the batch are the legal actions of ONE decision point, all rows carry the same history z and differ in
 * x, and the action is the argmax over the rows, or a uniformly random row with probability exp_epsilon. This handle
 * evaluates S decision points per call, each with its own number of candidate rows, with one LSTM pass per decision
 * point, an inference torso that writes no activation to HBM, and the pick made on the device.
 *
 * Status codes and fi_last_error() as fi_learner.h; one thread at a time per handle. Parameters: the fp32 blob of
 * fi_farmer.h (fi_farmer_param_count() floats, state_dict order).
 *
 * One call: S decision points, N candidate rows, host offsets[S + 1] (int32, offsets[0] = 0, non-decreasing,
 * offsets[S] = N): decision point s owns rows offsets[s] .. offsets[s + 1] - 1. z [S][T][162], x [N][484], fp32.
 *
 * The numeric rule (host form in fp64: freeimpala_amd/farmer_act.py, act_reference and pick_reference):
 *  1. LSTM. h_s is the last hidden state of z_s under the rule of fi_farmer_lstm.h (FI_FARMER_LSTM_BF16), computed
 *     by that mode's own kernels, once per decision point: h equals h_last of a bf16-mode fi_farmer of batch S on
 *     the same z, bit for bit.
 *  2. Layer-1 input. c_r = [rne(h_seg(r)) | rne(x_r)]: 612 bf16 values, zero-padded to 624 (39 k-steps of 16).
 *  3. Layers 1..5. a_l = rne(relu(a_{l-1} . rne(W_l)^T + b_l)): bf16 operands, fp32 accumulation in ascending
 *     k-steps on v_mfma_f32_32x32x16_bf16; the fp32 bias is added in the epilogue, after the last k-step; relu(v) is
 *     0 for v < 0 and v otherwise, so a NaN stays a NaN; every a_l is rounded to bf16 where it is handed on.
 *  4. Value. v_r = sum_k a5[r][k] w6[k] + b6 in fp32 from the bf16 a5 and the fp32 w6, in one fixed order (a lane's
 *     128 terms as an fma chain in ascending k, four lanes added as a tree, then b6). No atomics.
 *  5. Pick, per decision point with n_s rows. The greedy row is the one with the largest finite value, the lowest
 *     index on ties; rows whose value is not finite are never picked and are counted (fi_farmer_actor_nonfinite).
 *     (w0, w1, w2, w3) = philox4(seed, draw S + s, stream 11), draw = the handle's act calls so far. The decision
 *     point explores when w0 2^-32 < eps_s (compared exactly, in fp64) and then takes row j = (w1 n_s) >> 32; a j
 *     whose value is not finite is not taken: the greedy row stands and explored stays 0. actions[s] is the row's
 *     index inside its decision point; n_s = 0, or no finite row, gives -1 and explored 0. best_value[s] is the
 *     greedy row's value, -inf where there is none. eps = 0 never explores; eps = 1 always does.
 */
#ifndef FI_FARMER_ACT_H
#define FI_FARMER_ACT_H

#include <stddef.h>
#include <stdint.h>

#include "fi_farmer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fi_farmer_actor_config {
    int max_states;  /* most decision points of a call                                   */
    int max_rows;    /* most candidate rows of a call                                    */
    int seq_len;     /* T of z (default 10)                                              */
    int device;      /* HIP device ordinal                                               */
    uint64_t seed;   /* Philox key of the exploration draws                              */
} fi_farmer_actor_config;

typedef struct fi_farmer_actor fi_farmer_actor;

void fi_farmer_actor_config_init(fi_farmer_actor_config* cfg);
/* FI_ERR_INVALID for sizes below 1; FI_ERR_UNSUPPORTED when max_states seq_len 512 or max_rows 512 reaches 2^31. */
int fi_farmer_actor_create(const fi_farmer_actor_config* cfg, fi_farmer_actor** out);
void fi_farmer_actor_destroy(fi_farmer_actor* a);
/* The parameters from a host blob; the bf16 operand images are rebuilt behind the copy, on the handle's stream. */
int fi_farmer_actor_set_params(fi_farmer_actor* a, const float* host, size_t n);
/* The parameters from a learner on the same device: an event recorded on the learner's stream, a wait for it on the
 * actor's stream and a device-to-device copy behind it. No host wait, no host copy. */
int fi_farmer_actor_set_params_from(fi_farmer_actor* a, fi_farmer* learner);
/* One call of the rule above. inputs_on_device != 0: z and x are device pointers (x 16-byte aligned, z 8-byte), read
 * in place; else host pointers, copied in on the handle's stream. offsets, eps_per_state (nullable: then every
 * decision point uses eps), actions [S], explored [S] and values (nullable, [N]) are host pointers. Refused before
 * anything is enqueued: S < 1 or above max_states, offsets that do not start at 0 or decrease, N above max_rows, an
 * eps outside [0, 1] or NaN (FI_ERR_INVALID); a handle without parameters (FI_ERR_STATE). The LSTM, the torso and
 * the pick are enqueued back to back; the host waits once, for the results. */
int fi_farmer_actor_act(fi_farmer_actor* a, const float* z, const float* x, int inputs_on_device, const int32_t* offsets,
                        int S, float eps, const float* eps_per_state, int32_t* actions, int32_t* explored, float* values);
/* With the trace on, a call also stores a1..a5 as they are handed on: bf16 [5][N][512], N of that call. The values
 * are the same bits either way. */
int fi_farmer_actor_set_trace(fi_farmer_actor* a, int on);
/* Device pointer / bytes of "h" (fp32 [max_states][612], columns 0..127: h_s), "values" (fp32 [max_rows]),
 * "actions" (of the last call: int32 actions [S] | int32 explored [S] | fp32 best_value [S]), "trace" (bf16
 * [5][N][512], FI_ERR_STATE before the trace was ever on) and "params" (the fp32 blob). */
int fi_farmer_actor_tensor(fi_farmer_actor* a, const char* name, void** dev_ptr, size_t* bytes);
/* Rows with a non-finite value since create; waits for the handle's stream. */
int fi_farmer_actor_nonfinite(fi_farmer_actor* a, uint64_t* rows);
void* fi_farmer_actor_stream(fi_farmer_actor* a);
/* Profiling (scripts/farmer_act_bench.py): with it on, a call records HIP events around its LSTM launches (projection
 * and recurrence), its torso (row table and torso) and its pick; fi_farmer_actor_kernel_ms returns the device ms of
 * the last call's three parts, FI_ERR_STATE when that call was not profiled. */
int fi_farmer_actor_set_profiling(fi_farmer_actor* a, int on);
int fi_farmer_actor_kernel_ms(fi_farmer_actor* a, float* lstm_ms, float* torso_ms, float* pick_ms);

#ifdef __cplusplus
}
#endif
#endif
