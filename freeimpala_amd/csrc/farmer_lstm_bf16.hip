// farmer_lstm_bf16.hip -- FarmerLstm's LSTM in bf16 on v_mfma_f32_32x32x16_bf16 (include/fi_farmer_lstm.h, where
// the numeric rule stands): bf16 operands, fp32 accumulation, fp32 cell state and activation arithmetic.
//
// A 32x32x16 MFMA reads, per lane, the 8 consecutive k of one row (A) or one column (B): lane = 32 ((k >> 3) & 1)
// + (index & 31); one operand of 32 indices x 16 k is 64 pieces of 16 bytes (1 KiB), and the weight images hold
// such fragments tile-major, k-step next, so a wave loads one operand as one 16-byte load per lane. Accumulator
// register v of a lane is A-index (v >> 2) 8 + (lane >> 5) 4 + (v & 3), B-index lane & 31.
//
// The recurrences are batch-tiled: one 256-thread workgroup per 32 batch rows walks the sequence with its share of
// W_hh in registers (128 VGPRs per lane) and computes the TRANSPOSED product, the weights as the A operand and
// the rows' h^T (dgates^T) as the B operand. A lane's four consecutive accumulator registers are then four
// consecutive hidden units of ONE batch row: the cell update is element-wise on accumulators, no gate crosses
// LDS, and the rounded h (dgates) leave as 8-byte LDS stores that are already the next step's B operand
// (fragment ks at ks KiB, lane l at 16 l: conflict-free 16-byte reads). The LDS tile is double-buffered, so a
// step costs one barrier, and that barrier (lds_barrier) waits for LDS only: the step's global stores and the
// loads fetched one step ahead stay in flight across it. The loads of a step are issued before its stores, so the
// counted wait for them leaves the stores in flight (the comment above lstm_fwd_reg_kernel in farmer.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "farmer_lstm_bf16.h"
#include "fi_common.h"
#include "fi_farmer_lstm.h"
#include "kernels.h"

namespace fi {
namespace farmer {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int IN = 162, H = 128, G = 4 * H, CAT = H + 484;
constexpr int KSI = 11, KSH = H / 16, KSG = G / 16;  // k-steps of the padded input (176), of h and of the gates
constexpr int kTile = 32;                            // batch rows of a recurrence workgroup
constexpr int kRows = 64;                            // rows of a projection tile and of a weight-gradient chunk
constexpr int kHalf = 528;  // staged operands: LDS bytes of one 32-lane half of a fragment, 512 + 16 of padding

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ float sigm(float a) { return 1.0f / (1.0f + __expf(-a)); }
__device__ __forceinline__ int acc_row(int v, int lane) { return (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3); }

// staged operands (projection, weight gradients): byte offset of element (k, idx) and a lane's fragment
__device__ __forceinline__ int lds_at(int KS, int k, int idx) {
    return (((idx >> 5) * KS + (k >> 4)) * 2 + ((k >> 3) & 1)) * kHalf + (idx & 31) * 16 + (k & 7) * 2;
}
__device__ __forceinline__ bf16x8 lds_frag(const char* lds, int KS, int tile, int ks, int lane) {
    return *(const bf16x8*)(lds + ((tile * KS + ks) * 2 + (lane >> 5)) * kHalf + (lane & 31) * 16);
}
// 8 elements z[row][c0 .. c0 + 7] rounded, zero past column 161 (c0 even: a z row is 8-byte aligned)
__device__ __forceinline__ bf16x8 z_piece(const float* __restrict__ z, int row, int M, int c0) {
    bf16x8 o = {};
    if (row >= M) return o;
    const float* q = z + (size_t)row * IN + c0;
#pragma unroll
    for (int e = 0; e < 8; e += 2)
        if (c0 + e < IN) {
            const f32x2 v = *(const f32x2*)(q + e);
            o[e] = (__bf16)v.x;
            o[e + 1] = (__bf16)v.y;
        }
    return o;
}

// ------------------------------------------------------------------ the weight images: one 16-byte piece per thread
__global__ __launch_bounds__(256) void lstm_weights_bf16_kernel(const float* __restrict__ wih, const float* __restrict__ whh,
                                                                __bf16* __restrict__ img) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (int)(kLstmImgElems / 8)) return;
    const int seg = p < (int)(kLstmImgWhh / 8) ? 0 : p < (int)(kLstmImgWhhT / 8) ? 1 : 2;
    const int loc = p - (int)((seg == 0 ? kLstmImgWih : seg == 1 ? kLstmImgWhh : kLstmImgWhhT) / 8);
    const int KS = seg == 0 ? KSI : seg == 1 ? KSH : KSG;
    const int lane = loc & 63, t = loc >> 6, idx = (t / KS) * 32 + (lane & 31), k0 = (t % KS) * 16 + (lane >> 5) * 8;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v;
        if (seg == 0) v = k0 + e < IN ? wih[(size_t)idx * IN + k0 + e] : 0.f;  // W_ih[n][k], k padded to 176
        else if (seg == 1) v = whh[(size_t)idx * H + k0 + e];                  // W_hh[n][k]
        else v = whh[(size_t)(k0 + e) * H + idx];                              // W_hh^T[u][n]
        o[e] = (__bf16)v;
    }
    *(bf16x8*)(img + (size_t)p * 8) = o;
}

// ------------------------------------------------------------------ xp = rne(z) . rne(W_ih)^T + bsum
// 64 rows per workgroup: z is rounded on its way into LDS (A order), the image's 16 column tiles are dealt to the
// 4 waves and read straight from L2; K = 176 in 11 ascending k-steps, the bias in the epilogue
__global__ __launch_bounds__(256) void lstm_xproj_bf16_kernel(const float* __restrict__ z, int M,
                                                              const __bf16* __restrict__ img, const float* __restrict__ bsum,
                                                              float* __restrict__ xp) {
    __shared__ __attribute__((aligned(16))) char lds[2 * KSI * 2 * kHalf];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kRows;
    for (int p = tid; p < kRows * KSI * 2; p += 256) {
        const int r = p / (KSI * 2), kp = p - r * (KSI * 2);
        *(bf16x8*)(lds + lds_at(KSI, kp * 8, r)) = z_piece(z, row0 + r, M, kp * 8);
    }
    __syncthreads();
    for (int ct = wave; ct < G / 32; ct += 4) {
        f32x16 c0 = {}, c1 = {};
        const bf16x8* bp = (const bf16x8*)(img + kLstmImgWih) + (size_t)ct * KSI * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < KSI; ++ks) {
            const bf16x8 b = bp[ks * 64];
            c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(lds, KSI, 0, ks, lane), b, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(lds, KSI, 1, ks, lane), b, c1, 0, 0, 0);
        }
        const int col = ct * 32 + (lane & 31);
        const float bias = bsum[col];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r0 = row0 + acc_row(v, lane), r1 = r0 + 32;
            if (r0 < M) xp[(size_t)r0 * G + col] = c0[v] + bias;
            if (r1 < M) xp[(size_t)r1 * G + col] = c1[v] + bias;
        }
    }
}

// ------------------------------------------------------------------ forward recurrence
// Wave w owns hidden units 32 w .. 32 w + 31 of all four gates: four 32 x 32 tiles over K = 128, 32 MFMAs per
// step; its 128 x 128 slice of the W_hh image stays in registers. A lane holds, for j = 0..3, the units
// 32 w + 8 j + 4 (lane >> 5) + 0..3 of batch row lane & 31: the accumulators start from xp (fetched one step
// ahead as 16 float4), and i, f, g, o, c and h of a (row, unit) live in the same lane. Rows past B compute on
// zeros and store nothing.
__global__ __launch_bounds__(256) void lstm_fwd_mfma_kernel(const float* __restrict__ xp, const __bf16* __restrict__ img,
                                                            int B, int T, __bf16* __restrict__ gates,
                                                            float* __restrict__ cst, __bf16* __restrict__ hprev,
                                                            float* __restrict__ cat) {
    __shared__ __attribute__((aligned(16))) char hs[2][KSH * 1024];  // rne(h)^T as the B operand, double-buffered
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hl = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.x * kTile + r, ub = 32 * w + 4 * hl;
    const bool valid = row < B;
    const size_t e0 = (size_t)(valid ? row : 0) * T;  // the row's first (row, t) index
    bf16x8 wr[4][KSH];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ks = 0; ks < KSH; ++ks)
            wr[g][ks] = ((const bf16x8*)(img + kLstmImgWhh))[((g * 4 + w) * KSH + ks) * 64 + lane];
    ((f32x4*)hs[0])[tid] = f32x4{0.f, 0.f, 0.f, 0.f};  // h_{-1} = 0
    ((f32x4*)hs[0])[tid + 256] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 c[4], xn[4][4];
    auto fetch = [&](int t) {
        const float* src = xp + (e0 + t) * G + ub;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) xn[g][j] = valid ? *(const f32x4*)(src + g * H + 8 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    fetch(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid) *(bf16x4*)(hprev + e0 * H + ub + 8 * j) = bf16x4{};
    }
    lds_barrier();
    for (int t = 0; t < T; ++t) {
        const char* hr = hs[t & 1];
        char* hw = hs[(t + 1) & 1];
        f32x16 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[g][v] = xn[g][v >> 2][v & 3];
        if (t + 1 < T) fetch(t + 1);
#pragma unroll
        for (int ks = 0; ks < KSH; ++ks) {
            const bf16x8 b = *(const bf16x8*)(hr + ks * 1024 + lane * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[g][ks], b, acc[g], 0, 0, 0);
        }
        const size_t e = e0 + t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16x4 gb[4], hb;
            f32x4 hv;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = 4 * j + i;
                const float ig = sigm(acc[0][v]), fg = sigm(acc[1][v]), gg = tanhf(acc[2][v]), og = sigm(acc[3][v]);
                const float cc = fg * c[j][i] + ig * gg;
                c[j][i] = cc;
                hv[i] = og * tanhf(cc);
                hb[i] = (__bf16)hv[i];
                gb[0][i] = (__bf16)ig, gb[1][i] = (__bf16)fg, gb[2][i] = (__bf16)gg, gb[3][i] = (__bf16)og;
            }
            // units 32 w + 8 j + 4 hl + 0..3: fragment 2 w + (j >> 1), half j & 1, elements 4 hl .. 4 hl + 3
            *(bf16x4*)(hw + (2 * w + (j >> 1)) * 1024 + (j & 1) * 512 + r * 16 + hl * 8) = hb;
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) *(bf16x4*)(gates + e * G + g * H + ub + 8 * j) = gb[g];
                *(f32x4*)(cst + e * H + ub + 8 * j) = c[j];
                if (t + 1 < T) *(bf16x4*)(hprev + (e + 1) * H + ub + 8 * j) = hb;
                else *(f32x4*)(cat + (size_t)row * CAT + ub + 8 * j) = hv;
            }
        }
        lds_barrier();  // rne(h_t) visible; every wave is done reading h_{t-1}
    }
}

// ------------------------------------------------------------------ backward recurrence (BPTT)
// Same tiling, t = T-1..0. Wave w produces dh^T for its 32 units: one 32 x 32 tile over K = 512, 32 MFMAs per
// step, with its 128 x 512 slice of the W_hh^T image in registers. With the stored gates and c of its units
// (fetched one step ahead) the lane turns dh into the four dgates of its (row, unit)s; dc stays in registers.
// rne(dgates) goes to dG and, as the next step's B operand, to the double-buffered LDS tile (2 x 32 KiB).
//   do = dh tanh(c_t);  dc += dh o (1 - tanh^2 c_t);  di = dc g;  dg = dc i;  df = dc c_{t-1};
//   dgates = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o));  dc <- dc f
__global__ __launch_bounds__(256) void lstm_bwd_mfma_kernel(const __bf16* __restrict__ gates, const float* __restrict__ cst,
                                                            const __bf16* __restrict__ img, const float* __restrict__ dcat,
                                                            int B, int T, __bf16* __restrict__ dG) {
    __shared__ __attribute__((aligned(16))) char ds[2][KSG * 1024];  // rne(dgates)^T as the B operand
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hl = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.x * kTile + r, ub = 32 * w + 4 * hl;
    const bool valid = row < B;
    const size_t e0 = (size_t)(valid ? row : 0) * T;
    bf16x8 wr[KSG];
#pragma unroll
    for (int ks = 0; ks < KSG; ++ks) wr[ks] = ((const bf16x8*)(img + kLstmImgWhhT))[(w * KSG + ks) * 64 + lane];
    bf16x4 gt[4][4], gn[4][4];  // the gates of step t and of step t - 1
    f32x4 ct[4], cp[4], cn[4], dc[4];  // c_t, c_{t-1}, c_{t-2}
    auto load_c = [&](int t, f32x4 (&d)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            d[j] = valid && t >= 0 ? *(const f32x4*)(cst + (e0 + t) * H + ub + 8 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto load_g = [&](int t, bf16x4 (&d)[4][4]) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                d[g][j] = valid ? *(const bf16x4*)(gates + (e0 + t) * G + g * H + ub + 8 * j) : bf16x4{};
    };
    load_g(T - 1, gt);
    load_c(T - 1, ct);
    load_c(T - 2, cp);
#pragma unroll
    for (int j = 0; j < 4; ++j) dc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = T - 1; t >= 0; --t) {
        f32x16 dh = {};
        if (t == T - 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = valid ? *(const f32x4*)(dcat + (size_t)row * CAT + ub + 8 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) dh[4 * j + i] = v[i];
            }
        }
        if (t > 0) {
            load_g(t - 1, gn);
            load_c(t - 2, cn);
        }
        if (t < T - 1) {
            const char* dr = ds[(t + 1) & 1];
#pragma unroll
            for (int ks = 0; ks < KSG; ++ks)
                dh = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[ks], *(const bf16x8*)(dr + ks * 1024 + lane * 16), dh, 0, 0, 0);
        }
        char* dw = ds[t & 1];
        const size_t e = e0 + t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16x4 db[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ig = (float)gt[0][j][i], fg = (float)gt[1][j][i], gg = (float)gt[2][j][i], og = (float)gt[3][j][i];
                const float d = dh[4 * j + i], tc = tanhf(ct[j][i]);
                const float d_o = d * tc;
                const float dcv = dc[j][i] + d * og * (1.f - tc * tc);
                const float di = dcv * gg, dgv = dcv * ig, df = dcv * cp[j][i];
                db[0][i] = (__bf16)(di * ig * (1.f - ig));
                db[1][i] = (__bf16)(df * fg * (1.f - fg));
                db[2][i] = (__bf16)(dgv * (1.f - gg * gg));
                db[3][i] = (__bf16)(d_o * og * (1.f - og));
                dc[j][i] = dcv * fg;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // gate column 128 g + 32 w + 8 j + 4 hl + 0..3: fragment 8 g + 2 w + (j >> 1), half j & 1
                *(bf16x4*)(dw + (8 * g + 2 * w + (j >> 1)) * 1024 + (j & 1) * 512 + r * 16 + hl * 8) = db[g];
                if (valid) *(bf16x4*)(dG + e * G + g * H + ub + 8 * j) = db[g];
            }
        }
        if (t > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ct[j] = cp[j];
                cp[j] = cn[j];
#pragma unroll
                for (int g = 0; g < 4; ++g) gt[g][j] = gn[g][j];
            }
        }
        lds_barrier();  // rne(dgates_t) visible; every wave is done reading dgates_{t+1}
    }
}

// ------------------------------------------------------------------ weight gradients over row slices
// Workgroup (slice, half): gW[n][k] = sum over the slice's rows of dG[row][n] X[row][k] for the 256 gate columns
// of its half, wave w the 32 of them at 256 half + 32 w, all KT k-tiles (dG^T is the A operand, X the B operand:
// lanes run along k in the stores). Both operands have the rows as their K, so a chunk of 64 rows is transposed
// on its way into LDS (2-byte writes into padded halves). X is z (rounded on load, K padded to 192 in LDS, 162
// stored) or hprev. cs (nullable): the slice's column sums of dG, rows in ascending order.
template <bool XF32>
__global__ __launch_bounds__(512) void lstm_wgrad_bf16_kernel(const __bf16* __restrict__ dG, const void* __restrict__ X, int M,
                                                              int cps, float* __restrict__ slab, float* __restrict__ cs) {
    constexpr int C = XF32 ? IN : H, KT = XF32 ? 6 : 4;
    __shared__ __attribute__((aligned(16))) char ldsD[8 * 4 * 2 * kHalf];
    __shared__ __attribute__((aligned(16))) char ldsX[KT * 4 * 2 * kHalf];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n0 = blockIdx.y * 256;
    const int chunks = cdiv(M, kRows), c_lo = blockIdx.x * cps, c_hi = min(chunks, c_lo + cps);
    f32x16 acc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[kt] = f32x16{};
    float bsum = 0.f;
    for (int ch = c_lo; ch < c_hi; ++ch) {
        const int row0 = ch * kRows;
        __syncthreads();  // the chunk before this one has been read
        for (int p = tid; p < kRows * 32; p += 512) {
            const int cp = p >> 6, rr = p & 63, row = row0 + rr;
            bf16x8 v = {};
            if (row < M) v = *(const bf16x8*)(dG + (size_t)row * G + n0 + cp * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) *(__bf16*)(ldsD + lds_at(4, rr, cp * 8 + e)) = v[e];
        }
        for (int p = tid; p < kRows * KT * 4; p += 512) {
            const int cp = p >> 6, rr = p & 63, row = row0 + rr;
            bf16x8 v = {};
            if constexpr (XF32) v = z_piece((const float*)X, row, M, cp * 8);
            else if (row < M) v = *(const bf16x8*)((const __bf16*)X + (size_t)row * H + cp * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) *(__bf16*)(ldsX + lds_at(4, rr, cp * 8 + e)) = v[e];
        }
        __syncthreads();
        if (cs && tid < 256) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const bf16x8 v = *(const bf16x8*)(ldsD + lds_at(4, g * 8, tid));
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum += (float)v[e];
            }
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 a = lds_frag(ldsD, 4, wave, ks, lane);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, lds_frag(ldsX, 4, kt, ks, lane), acc[kt], 0, 0, 0);
        }
    }
    float* out = slab + (size_t)blockIdx.x * G * C;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int k = kt * 32 + (lane & 31);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = n0 + wave * 32 + acc_row(v, lane);
            if (k < C) out[(size_t)n * C + k] = acc[kt][v];
        }
    }
    if (cs && tid < 256) cs[(size_t)blockIdx.x * G + n0 + tid] = bsum;
}

}  // namespace

// ------------------------------------------------------------------ launchers
int lstm_bf16_splits(int rows) { return std::max(1, std::min(128, cdiv(rows, kRows) / 8)); }
size_t lstm_bf16_slab_floats(int splits) { return (size_t)splits * G * IN + (size_t)splits * G; }

int lstm_weights_bf16(const float* wih, const float* whh, __bf16* img, hipStream_t s) {
    hipLaunchKernelGGL(lstm_weights_bf16_kernel, dim3((unsigned)cdiv((int)(kLstmImgElems / 8), 256)), dim3(256), 0, s, wih, whh,
                       img);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int lstm_xproj_bf16(const float* z, int rows, const __bf16* img, const float* bsum, float* xp, hipStream_t s) {
    hipLaunchKernelGGL(lstm_xproj_bf16_kernel, dim3((unsigned)cdiv(rows, kRows)), dim3(256), 0, s, z, rows, img, bsum, xp);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int lstm_fwd_mfma(const float* xp, const __bf16* img, int B, int T, __bf16* gates, float* cst, __bf16* hprev, float* cat,
                  hipStream_t s) {
    hipLaunchKernelGGL(lstm_fwd_mfma_kernel, dim3((unsigned)cdiv(B, kTile)), dim3(256), 0, s, xp, img, B, T, gates, cst, hprev,
                       cat);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int lstm_bwd_mfma(const __bf16* gates, const float* cst, const __bf16* img, const float* dcat, int B, int T, __bf16* dG,
                  hipStream_t s) {
    hipLaunchKernelGGL(lstm_bwd_mfma_kernel, dim3((unsigned)cdiv(B, kTile)), dim3(256), 0, s, gates, cst, img, dcat, B, T, dG);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int lstm_wgrads_bf16(const __bf16* dG, const float* z, const __bf16* hprev, int rows, int splits, float* slab, float* gwih,
                     float* gwhh, float* gb, hipStream_t s) {
    const int cps = cdiv(cdiv(rows, kRows), splits);
    float* cs = slab + (size_t)splits * G * IN;
    const dim3 grid((unsigned)splits, 2), blk(512);
    hipLaunchKernelGGL(lstm_wgrad_bf16_kernel<true>, grid, blk, 0, s, dG, (const void*)z, rows, cps, slab, (float*)nullptr);
    FI_TRY(reduce_slabs(slab, splits, (size_t)G * IN, gwih, s));
    hipLaunchKernelGGL(lstm_wgrad_bf16_kernel<false>, grid, blk, 0, s, dG, (const void*)hprev, rows, cps, slab, cs);
    FI_TRY(reduce_slabs(slab, splits, (size_t)G * H, gwhh, s));
    FI_TRY(reduce_slabs(cs, splits, (size_t)G, gb, s));
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace farmer
}  // namespace fi

// ------------------------------------------------------------------ fi_farmer_lstm.h
static const fi::farmer::LstmBf16Ops kOps{fi::farmer::lstm_bf16_splits, fi::farmer::lstm_bf16_slab_floats,
                                          fi::farmer::lstm_weights_bf16, fi::farmer::lstm_xproj_bf16,
                                          fi::farmer::lstm_fwd_mfma,     fi::farmer::lstm_bwd_mfma,
                                          fi::farmer::lstm_wgrads_bf16};
extern "C" int fi_farmer_set_lstm_precision(fi_farmer* f, int precision) {
    return fi::farmer::set_lstm_precision(f, precision, &kOps);
}
extern "C" int fi_farmer_lstm_precision(const fi_farmer* f) { return fi::farmer::lstm_precision(f); }
