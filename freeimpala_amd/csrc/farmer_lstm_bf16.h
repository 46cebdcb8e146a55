// farmer_lstm_bf16.h -- internal launchers of FarmerLstm's bf16 LSTM (farmer_lstm_bf16.hip; the rule
// stands in include/fi_farmer_lstm.h). farmer.hip owns the handle and calls these behind its mode switch.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fi_farmer.h"

namespace fi {
namespace farmer {

// the weight images of one parameter blob, in bf16 elements from the image's start: W_ih [512][176] and
// W_hh [512][128] as MFMA operands of 32 rows x 16 k (tile-major, k-step next, 1 KiB per fragment), and
// W_hh^T [128][512] the same way for the BPTT
constexpr size_t kLstmImgWih = 0, kLstmImgWhh = 16 * 11 * 512, kLstmImgWhhT = kLstmImgWhh + 16 * 8 * 512,
                 kLstmImgElems = kLstmImgWhhT + 4 * 32 * 512;

// row slices of the weight gradients for `rows` = B T rows: at least 8 chunks of 64 rows each, 128 at most
int lstm_bf16_splits(int rows);
// floats of the slab lstm_wgrads_bf16 needs for that many slices
size_t lstm_bf16_slab_floats(int splits);

int lstm_weights_bf16(const float* wih, const float* whh, __bf16* img, hipStream_t s);
// xp [rows][512] = rne(z) . rne(W_ih)^T + bsum
int lstm_xproj_bf16(const float* z, int rows, const __bf16* img, const float* bsum, float* xp, hipStream_t s);
// gates [B T][512] bf16, cst [B T][128] fp32, hprev [B T][128] bf16 (row t: rne(h_{t-1})), cat[:, 0:128] = h_{T-1}
int lstm_fwd_mfma(const float* xp, const __bf16* img, int B, int T, __bf16* gates, float* cst, __bf16* hprev, float* cat,
                  hipStream_t s);
// dG [B T][512] bf16 from the stored gates and c and dcat[:, 0:128]
int lstm_bwd_mfma(const __bf16* gates, const float* cst, const __bf16* img, const float* dcat, int B, int T, __bf16* dG,
                  hipStream_t s);
// gW_ih [512][162] = dG^T rne(z), gW_hh [512][128] = dG^T hprev, gb [512] = the column sums of dG
int lstm_wgrads_bf16(const __bf16* dG, const float* z, const __bf16* hprev, int rows, int splits, float* slab, float* gwih,
                     float* gwhh, float* gb, hipStream_t s);


// The launchers above as pointers: farmer_lstm_bf16.hip, which holds fi_farmer_lstm.h's C entry points, hands
// them to the handle with the mode, so farmer.hip names nothing of farmer_lstm_bf16.hip and links without it
struct LstmBf16Ops {
    decltype(&lstm_bf16_splits) splits;
    decltype(&lstm_bf16_slab_floats) slab_floats;
    decltype(&lstm_weights_bf16) weights;
    decltype(&lstm_xproj_bf16) xproj;
    decltype(&lstm_fwd_mfma) fwd;
    decltype(&lstm_bwd_mfma) bwd;
    decltype(&lstm_wgrads_bf16) wgrads;
};
// farmer.hip: fi_farmer_lstm.h's entry points behind their argument checks
int set_lstm_precision(::fi_farmer* f, int precision, const LstmBf16Ops* ops);
int lstm_precision(const ::fi_farmer* f);

}  // namespace farmer
}  // namespace fi
