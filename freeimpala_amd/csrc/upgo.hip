// upgo.hip -- the learner's upgoing policy update, UPGO (include/fi_upgo.h, where the rule stands): the
// upgoing returns of a batch, the policy-gradient term on them added onto dlogits, the stats block, and
// every fi_upgo_* entry point.
//
//   upgo_scan_kernel      G_t = r_t + g_t (up_t ? G_{t+1} : V_{t+1}) down each column, AU = G - V. up_t is a
//                         comparison of inputs, so step t is the affine map X -> d_t + k_t X with
//                         input-only (k_t, d_t) and the recurrence a suffix composition of such maps: it
//                         is done across the lanes of a wave, not as a serial chain over T.
//                         A workgroup owns kTile = 16 columns (B = 4096: 256 workgroups, one per CU) and
//                         walks T in chunks of 64 steps from the top down. The (r, g, V) rows of a chunk
//                         -- 66 of them: step t needs rows t + 1 and t + 2 -- are read along b, 16 bytes
//                         per lane where B allows, and transposed into LDS, one run of 66 floats per
//                         column. Wave w takes the columns 4 w .. 4 w + 3, lane = time step: (k, d) and the
//                         cut flag come from the lane's own and its two upper neighbours' LDS entries; the
//                         four columns' scans run interleaved: shifts by 1, 2, 4, 8 inside each 16-lane row
//                         by DPP, the three row totals by v_readlane; the carry G_{t0 + 64} of the chunk
//                         above is a wave-uniform scalar. AU (and G) go back through LDS and leave along b.
//                         LDS stride 66 floats: the transposing stores of a 32-lane group (8 rows x 4
//                         pieces, bank = 8 piece + row + 2 j mod 32) and the per-column reads (consecutive
//                         lanes, consecutive floats) are both conflict-free; 64 would put the four pieces
//                         on one bank. The global loads of the chunk below are issued into registers before
//                         the scan of the current one. One u64 count of up links per workgroup.
//   upgo_grad_kernel      kl_penalty_kernel's grid, read pattern and LDS footprint (row_stream.h) over
//                         (pi, mu, dlogits): one lane per row runs pair_log_prob and policy_row_grad
//                         (policy_row.h), which leaves coeff rho AU (pi - [a]) over the pi row; add_run adds
//                         the rows onto dlogits where they lie. Per workgroup one fp64 pair (loss, sum AU)
//                         and the count of AU > 0.
//   upgo_finalize_kernel  one workgroup: the partials added in a fixed order, the 40-byte block.
// No float atomics. learner.cpp names nothing of this file: fi_upgo_enable hangs an UpgoBlock with the
// launcher on the handle (kernels.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <new>
#include <string>

#include "atari.h"  // KernelTagger, TagScope
#include "fi_common.h"
#include "fi_upgo.h"
#include "host_util.h"
#include "kernels.h"
#include "policy_row.h"
#include "row_stream.h"

namespace fi {

namespace {
static_assert(sizeof(fi_upgo_stats) == 40 && sizeof(fi_upgo_params) == 8, "fi_upgo.h fixes both sizes");

constexpr int kTile = 16;                     // columns per workgroup of the scan
constexpr int kChunk = 64;                    // time steps per chunk: one per lane
constexpr int kRows = kChunk + 2;             // staged rows per chunk: t0 .. t0 + 65
constexpr int kStride = 66;                   // floats between two columns' time runs in LDS (see above)
constexpr int kColsPerWave = kTile / kWaves;  // 4
constexpr int kScanThreads = 64 * kWaves;
static_assert(kStride >= kRows && (4 * kStride) % 32 == 8, "the transposing stores rely on 4 * stride = 8 mod 32 banks");

struct ScanArgs {
    int T, B;
    const float* __restrict__ rew;
    const float* __restrict__ disc;
    const float* __restrict__ val;
    float* au;
    float* g;                     // nullable
    uint8_t* up;                  // nullable
    unsigned long long* up_part;  // nullable: [gridDim.x]
};

// how the 256 threads move a chunk's rows between global memory and LDS: kVec (B % 4 == 0), 4 lanes per
// row of 16 columns and 16 bytes per lane; else 16 lanes per row, one float each
template <bool kVec>
struct Mover {
    static constexpr int kPer = kVec ? 4 : 1;
    static constexpr int kLanesPerRow = kTile / kPer;
    static constexpr int kRowsPerPass = kScanThreads / kLanesPerRow;
    static constexpr int kLoadPasses = (kRows + kRowsPerPass - 1) / kRowsPerPass;  // 2 or 5
    static constexpr int kStorePasses = kChunk / kRowsPerPass;                     // 1 or 4
    float v[kLoadPasses][3][kPer];                                                 // r, g, V of the chunk in flight

    // rows t0 .. t0 + 65 of the tile: r and g exist below T, V up to T; everything else reads as 0
    __device__ __forceinline__ void load(const ScanArgs& a, int t0, int b0, int tid) {
        const int c0 = (tid % kLanesPerRow) * kPer, b = b0 + c0;
#pragma unroll
        for (int p = 0; p < kLoadPasses; ++p) {
            const int row = tid / kLanesPerRow + p * kRowsPerPass, t = t0 + row;
            const bool in = row < kRows && b < a.B;  // kVec: B % 4 == 0, so a piece lies inside or outside
            const size_t e = (size_t)t * a.B + b;
#pragma unroll
            for (int j = 0; j < kPer; ++j) v[p][0][j] = v[p][1][j] = v[p][2][j] = 0.f;
            if constexpr (kVec) {
                if (in && t < a.T) {
                    const f32x4 r = *(const f32x4*)(a.rew + e), g = *(const f32x4*)(a.disc + e);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[p][0][j] = r[j], v[p][1][j] = g[j];
                }
                if (in && t <= a.T) {
                    const f32x4 x = *(const f32x4*)(a.val + e);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[p][2][j] = x[j];
                }
            } else {
                if (in && t < a.T) v[p][0][0] = a.rew[e], v[p][1][0] = a.disc[e];
                if (in && t <= a.T) v[p][2][0] = a.val[e];
            }
        }
    }
    // the transpose: column c's time run starts at c * kStride
    __device__ __forceinline__ void to_lds(float* lr, float* lg, float* lv, int tid) const {
        const int c0 = (tid % kLanesPerRow) * kPer;
#pragma unroll
        for (int p = 0; p < kLoadPasses; ++p) {
            const int row = tid / kLanesPerRow + p * kRowsPerPass;
            if (row < kRows) {
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const int o = (c0 + j) * kStride + row;
                    lr[o] = v[p][0][j], lg[o] = v[p][1][j], lv[o] = v[p][2][j];
                }
            }
        }
    }
    // the way back: rows t0 .. t0 + 63 of one output
    static __device__ __forceinline__ void store(float* out, const float* lo, int T, int B, int t0, int b0, int tid) {
        const int c0 = (tid % kLanesPerRow) * kPer, b = b0 + c0;
#pragma unroll
        for (int p = 0; p < kStorePasses; ++p) {
            const int row = tid / kLanesPerRow + p * kRowsPerPass, t = t0 + row;
            if (t < T && b < B) {
                const size_t e = (size_t)t * B + b;
                if constexpr (kVec) {
                    f32x4 x;
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = lo[(c0 + j) * kStride + row];
                    *(f32x4*)(out + e) = x;
                } else {
                    out[e] = lo[c0 * kStride + row];
                }
            }
        }
    }
};

// One step of the cross-lane suffix composition. A lane holds the map of the steps [i, i + n): X -> d when
// cut (an up_t = 0 lies in the range: the steps above do not reach it), else X -> d + k X. (k2, d2, c2) is
// the map of the n steps above; the result covers both.
__device__ __forceinline__ void compose(float& k, float& d, int& c, float k2, float d2, int c2) {
    d = c ? d : d + k * d2;
    k = k * k2;
    c |= c2;
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// row_shl:N: lane i takes lane i + N of its 16-lane row; a lane whose source lies outside the row keeps `old`,
// here the identity map
template <int N>
__device__ __forceinline__ void row_step(float& k, float& d, int& c) {
    const float k2 = dpp_f<0x100 + N>(1.f, k), d2 = dpp_f<0x100 + N>(0.f, d);
    const int c2 = __builtin_amdgcn_update_dpp(0, c, 0x100 + N, 0xf, 0xf, false);
    compose(k, d, c, k2, d2, c2);
}
__device__ __forceinline__ float lane_f(float v, int src) {  // src: a constant
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

template <bool kVec>
__device__ __forceinline__ void upgo_scan_body(const ScanArgs& a) {
    __shared__ float lr[kTile * kStride], lg[kTile * kStride], lv[kTile * kStride];  // r, g, V: [column][row of the chunk]
    __shared__ float lau[kTile * kStride], lgg[kTile * kStride];                      // AU, G on their way out
    __shared__ unsigned cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int T = a.T, B = a.B, b0 = (int)blockIdx.x * kTile;
    const int nch = (T + kChunk - 1) / kChunk;
    Mover<kVec> mv;
    mv.load(a, (nch - 1) * kChunk, b0, tid);
    float carry[kColsPerWave];  // G at the bottom step of the chunk above, wave-uniform
#pragma unroll
    for (int q = 0; q < kColsPerWave; ++q) carry[q] = 0.f;  // the top chunk is cut at T - 1 and never reads it
    unsigned nup = 0;                                       // wave-uniform
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int t0 = ch * kChunk, t = t0 + lane;
        mv.to_lds(lr, lg, lv, tid);
        __syncthreads();  // the chunk is in LDS; the stores of the chunk above have read lau / lgg
        if (ch > 0) mv.load(a, t0 - kChunk, b0, tid);  // in flight behind the scan
        float k[kColsPerWave], d[kColsPerWave], v0[kColsPerWave];
        int c[kColsPerWave];
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) {
            const int col = w * kColsPerWave + q, o = col * kStride + lane;
            const float r0 = lr[o], r1 = lr[o + 1], g0 = lg[o], g1 = lg[o + 1], x1 = lv[o + 1], x2 = lv[o + 2];
            v0[q] = lv[o];
            const bool up = t < T - 1 && b0 + col < B && r1 + g1 * x2 >= x1;  // NaN: not up
            const bool live = t < T;
            k[q] = !live ? 1.f : (up ? g0 : 0.f);
            d[q] = !live ? 0.f : (up ? r0 : r0 + g0 * x1);
            c[q] = live && !up;
            nup += (unsigned)__popcll(__ballot(up));
            if (a.up && live && b0 + col < B) a.up[(size_t)t * B + b0 + col] = up ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) row_step<1>(k[q], d[q], c[q]);
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) row_step<2>(k[q], d[q], c[q]);
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) row_step<4>(k[q], d[q], c[q]);
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) row_step<8>(k[q], d[q], c[q]);
#pragma unroll
        for (int q = 0; q < kColsPerWave; ++q) {
            // lane i holds [i, end of its row); the rows above it: lanes 16, 32, 48 hold whole rows 1, 2, 3
            float k3 = lane_f(k[q], 48), d3 = lane_f(d[q], 48);
            int c3 = __builtin_amdgcn_readlane(c[q], 48);
            float k2 = lane_f(k[q], 32), d2 = lane_f(d[q], 32);
            int c2 = __builtin_amdgcn_readlane(c[q], 32);
            float k1 = lane_f(k[q], 16), d1 = lane_f(d[q], 16);
            int c1 = __builtin_amdgcn_readlane(c[q], 16);
            compose(k2, d2, c2, k3, d3, c3);  // rows 2 .. 3
            compose(k1, d1, c1, k2, d2, c2);  // rows 1 .. 3
            const int row = lane >> 4;
            const float ka = row == 0 ? k1 : (row == 1 ? k2 : (row == 2 ? k3 : 1.f));
            const float da = row == 0 ? d1 : (row == 1 ? d2 : (row == 2 ? d3 : 0.f));
            const int ca = row == 0 ? c1 : (row == 1 ? c2 : (row == 2 ? c3 : 0));
            compose(k[q], d[q], c[q], ka, da, ca);
            const float G = c[q] ? d[q] : d[q] + k[q] * carry[q];
            carry[q] = lane_f(G, 0);
            const int o = (w * kColsPerWave + q) * kStride + lane;
            lau[o] = G - v0[q];
            lgg[o] = G;
        }
        __syncthreads();  // AU and G of the chunk are complete; lr / lg / lv have been read
        Mover<kVec>::store(a.au, lau, T, B, t0, b0, tid);
        if (a.g) Mover<kVec>::store(a.g, lgg, T, B, t0, b0, tid);
    }
    if (a.up_part) {
        if (lane == 0) cnt[w] = nup;
        __syncthreads();
        if (tid == 0) {
            unsigned long long s = 0;
            for (int i = 0; i < kWaves; ++i) s += cnt[i];
            a.up_part[blockIdx.x] = s;
        }
    }
}

struct GradArgs {
    int T, B, A;
    int ct, slices, slice_len;
    const float* __restrict__ pi;
    const float* __restrict__ mu;
    const int32_t* __restrict__ act;
    const float* __restrict__ au;
    float* dlog;
    double* part;             // [ct * slices][2]: loss, sum AU
    unsigned long long* pos;  // [ct * slices]: rows with AU > 0
    float coeff, rho_bar;
};
}  // namespace

__global__ __launch_bounds__(kScanThreads) void upgo_scan_kernel(ScanArgs a) { upgo_scan_body<true>(a); }
// any B: one float per lane and access
__global__ __launch_bounds__(kScanThreads) void upgo_scan_ragged_kernel(ScanArgs a) { upgo_scan_body<false>(a); }

__global__ __launch_bounds__(64 * kWaves) void upgo_grad_kernel(GradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    __shared__ double red[kWaves * 3];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * 2 * kCols * S;  // this wave's pi rows (the increment after the arithmetic),
    float* const lm = lp + kCols * S;                           // then its mu rows
    const uint32_t n = (uint32_t)nb * A;
    double sum[3] = {0.0, 0.0, 0.0};  // loss_u, sum AU, rows with AU > 0
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const bool mine = live && lane < nb;
        const uint32_t g0 = ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A;
        int at = 0;
        float au = 0.f;
        if (mine) {
            const size_t e = (size_t)t * B + b0 + lane;
            at = a.act[e];
            au = a.au[e];
        }
        if (live) load_run<true>(a.pi, a.mu, lp, lm, g0, n, A, S, lane);
        __syncthreads();  // the rows are in LDS
        if (mine) {
            float* __restrict__ zp = lp + (uint32_t)lane * S;
            const uint32_t ai = at < 0 ? 0u : ((uint32_t)at >= A ? A - 1u : (uint32_t)at);
            const f32x2 la = pair_log_prob(zp, lm + (uint32_t)lane * S, A, ai);  // log pi(a), log mu(a)
            const float wgt = fminf(a.rho_bar, __expf(la.x - la.y)) * au;
            policy_row_grad(zp, A, ai, -a.coeff * wgt, 0.f);  // zp <- coeff rho AU (pi - [a])
            sum[0] -= (double)wgt * (double)la.x;
            sum[1] += (double)au;
            sum[2] += au > 0.f ? 1.0 : 0.0;
        }
        __syncthreads();  // the increment rows are complete
        if (live) add_run(a.dlog, lp, g0, n, A, S, lane);
        __syncthreads();  // the rows have been read: the next round may overwrite them
    }
    block_sums<3, kWaves>(sum, red);
    if (tid < 2) a.part[(size_t)blockIdx.x * 2 + tid] = sum[tid];
    if (tid == 2) a.pos[blockIdx.x] = (unsigned long long)sum[2];
}

// One workgroup. The counts pass through doubles, exact below 2^53.
__global__ __launch_bounds__(kStatThreads) void upgo_finalize_kernel(const double* __restrict__ part,
                                                                     const unsigned long long* __restrict__ pos, int nblk,
                                                                     const unsigned long long* __restrict__ up_part, int nscan,
                                                                     uint64_t rows, fi_upgo_stats* st) {
    __shared__ double red[kWaves * 4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += kStatThreads) {
        v[0] += part[2 * (size_t)i];
        v[1] += part[2 * (size_t)i + 1];
        v[2] += (double)pos[i];
    }
    for (int i = threadIdx.x; i < nscan; i += kStatThreads) v[3] += (double)up_part[i];
    block_sums<4, kWaves>(v, red);
    if (threadIdx.x != 0) return;
    st->loss_u = v[0];
    st->sum_au = v[1];
    st->rows = rows;
    st->links_up = (uint64_t)v[3];
    st->rows_positive = (uint64_t)v[2];
}

// ------------------------------------------------------------------ the launchers
namespace {
size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// FI_ERR_INVALID, `who` opens the message
int check_params(const std::string& who, const fi_upgo_params* p) {
    FI_REQUIRE(p, who + ": null params");
    FI_REQUIRE(std::isfinite(p->coeff) && p->coeff >= 0.f, who + ": coeff " + std::to_string(p->coeff) + " must be finite and >= 0");
    FI_REQUIRE(std::isfinite(p->rho_bar) && p->rho_bar > 0.f,
               who + ": rho_bar " + std::to_string(p->rho_bar) + " must be finite and > 0");
    return FI_OK;
}

int scan_blocks(int B) { return (B + kTile - 1) / kTile; }

// workspace: AU (T * B floats) | up-link counts of the scan's workgroups | (loss, sum AU) partials | AU > 0
// counts of the grad kernel's workgroups; every part on a 256-byte boundary
struct Layout {
    size_t up_part, part, pos, total;
};
Layout layout_of(int T, int B, const TilePlan& p) {
    Layout l{};
    const size_t nblk = (size_t)p.ct * p.slices;
    l.up_part = pad256((size_t)T * B * sizeof(float));
    l.part = l.up_part + pad256((size_t)scan_blocks(B) * sizeof(unsigned long long));
    l.pos = l.part + pad256(nblk * 2 * sizeof(double));
    l.total = l.pos + pad256(nblk * sizeof(unsigned long long));
    return l;
}

int scan_launch(int T, int B, const float* rew, const float* disc, const float* val, float* au, float* g, uint8_t* up,
                unsigned long long* up_part, hipStream_t stream) {
    FI_REQUIRE(rew && disc && val && au, "upgo_returns: null argument");
    FI_REQUIRE(T >= 1 && B >= 1, "upgo_returns: T = " + std::to_string(T) + ", B = " + std::to_string(B) + " must be >= 1");
    FI_REQUIRE(((uint64_t)T + 1) * (uint64_t)B < (1ull << 31),
               "upgo_returns: (T + 1) * B = " + std::to_string(((uint64_t)T + 1) * (uint64_t)B) + " passes 2^31 - 1");
    FI_REQUIRE((uintptr_t)rew % 16 == 0 && (uintptr_t)disc % 16 == 0 && (uintptr_t)val % 16 == 0 && (uintptr_t)au % 16 == 0 &&
                   (uintptr_t)g % 16 == 0,
               "upgo_returns: rewards, discounts, values, au and g must be 16-byte aligned (16 bytes move per lane and access)");
    const ScanArgs a{T, B, rew, disc, val, au, g, up, up_part};
    if (B % 4 == 0) hipLaunchKernelGGL(upgo_scan_kernel, dim3((unsigned)scan_blocks(B)), dim3(kScanThreads), 0, stream, a);
    else hipLaunchKernelGGL(upgo_scan_ragged_kernel, dim3((unsigned)scan_blocks(B)), dim3(kScanThreads), 0, stream, a);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// rules 1 to 3: every check in front of the first launch
int term_launch(int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew, const float* disc,
                const float* val, const fi_upgo_params* prm, float* dlog, void* stats, void* ws, size_t ws_bytes,
                hipStream_t stream, KernelTagger* tg) {
    FI_TRY(check_params("upgo_term", prm));
    FI_REQUIRE(pi && mu && act && rew && disc && val && dlog && stats && ws, "upgo_term: null argument");
    TilePlan p{};
    FI_TRY(tile_plan("upgo_term", T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)mu % 16 == 0 && (uintptr_t)dlog % 16 == 0 && (uintptr_t)ws % 16 == 0,
               "upgo_term: logits, mu, dlogits and ws must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)rew % 16 == 0 && (uintptr_t)disc % 16 == 0 && (uintptr_t)val % 16 == 0,
               "upgo_term: rewards, discounts and values must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)act % 4 == 0 && (uintptr_t)stats % 8 == 0, "upgo_term: actions must be 4-byte, stats_dev 8-byte aligned");
    const Layout lay = layout_of(T, B, p);
    FI_REQUIRE(ws_bytes >= lay.total, "upgo_term: ws_bytes " + std::to_string(ws_bytes) + " < " + std::to_string(lay.total) +
                                          " = fi_upgo_workspace_bytes(" + std::to_string(T) + ", " + std::to_string(B) + ", " +
                                          std::to_string(A) + ")");
    char* w = (char*)ws;
    GradArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = p.ct, a.slices = p.slices, a.slice_len = p.slice_len;
    a.pi = pi, a.mu = mu, a.act = act, a.au = (const float*)w, a.dlog = dlog;
    a.part = (double*)(w + lay.part), a.pos = (unsigned long long*)(w + lay.pos);
    a.coeff = prm->coeff, a.rho_bar = prm->rho_bar;
    unsigned long long* const up_part = (unsigned long long*)(w + lay.up_part);
    // two padded row sets per wave, kl_penalty_kernel's footprint: more than 64 KB of dynamic LDS at A > 30
    const size_t lds = 2 * (size_t)kWaves * kCols * (A | 1) * sizeof(float), lds_most = 2 * (size_t)kWaves * kCols * 65 * 4;
    if (lds > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)upgo_grad_kernel, raised, lds_most));
    }
    {
        TagScope t(tg, "upgo_scan");
        FI_TRY(scan_launch(T, B, rew, disc, val, (float*)w, nullptr, nullptr, up_part, stream));
    }
    const int nblk = p.ct * p.slices;
    {
        TagScope t(tg, "upgo_grad");
        hipLaunchKernelGGL(upgo_grad_kernel, dim3((unsigned)nblk), dim3(64 * kWaves), lds, stream, a);
        FI_HIP_CHECK(hipGetLastError());
    }
    {
        TagScope t(tg, "upgo_finalize");
        hipLaunchKernelGGL(upgo_finalize_kernel, dim3(1), dim3(kStatThreads), 0, stream, (const double*)a.part,
                           (const unsigned long long*)a.pos, nblk, (const unsigned long long*)up_part, scan_blocks(B),
                           (uint64_t)T * (uint64_t)B, (fi_upgo_stats*)stats);
        FI_HIP_CHECK(hipGetLastError());
    }
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's block
int block_launch(const UpgoBlock* b, int T, int B, int A, const float* pi, const float* mu, const int32_t* act, const float* rew,
                 const float* disc, const float* val, float* dlog, hipStream_t stream, KernelTagger* tg) {
    return term_launch(T, B, A, pi, mu, act, rew, disc, val, &b->prm, dlog, b->state, b->ws, b->ws_bytes, stream, tg);
}

void block_free(void* p) {
    UpgoBlock* b = (UpgoBlock*)p;
    if (!b) return;
    for (void* q : {b->state, b->ws})
        if (q) (void)hipFree(q);
    delete b;
}

int block_create(const UpgoView& v, UpgoBlock** out) {
    TilePlan p{};
    if (tile_plan("upgo_enable", v.T, v.B, v.A, &p) != FI_OK)
        return fail(FI_ERR_INVALID,
                    "upgo_enable: the learner's shape is outside the kernels' (" + std::string(fi_last_error()) + ")");
    UpgoBlock* b = new (std::nothrow) UpgoBlock();
    FI_REQUIRE(b, "upgo_enable: out of host memory");
    b->launch = block_launch;
    b->ws_bytes = layout_of(v.T, v.B, p).total;
    int rc = dev_alloc(&b->state, sizeof(fi_upgo_stats), "upgo_enable: state block");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "upgo_enable: workspace");
    if (rc == FI_OK) {
        const fi_upgo_stats st{};
        hipError_t e = hipMemcpyAsync(b->state, &st, sizeof(st), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v.stream);  // st is the stack's
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "upgo_enable: initialising the block failed");
        }
    }
    if (rc != FI_OK) {
        block_free(b);
        return rc;
    }
    *out = b;
    return FI_OK;
}

// the view of a handle whose block exists
int enabled_view(fi_learner* l, const char* who, UpgoView* v) {
    FI_TRY(learner_upgo_view(l, v));
    if (!v->block)
        return fail(FI_ERR_STATE, std::string(who) + ": the UPGO term was never on on this handle (fi_upgo_enable first)");
    FI_HIP_CHECK(hipSetDevice(v->dev));
    return FI_OK;
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_upgo_enable(fi_learner* l, const fi_upgo_params* params) {
    FI_REQUIRE(l && params, "upgo_enable: null argument");
    FI_TRY(check_params("upgo_enable", params));
    UpgoView v{};
    FI_TRY(learner_upgo_view(l, &v));
    UpgoBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("upgo_enable", FI_ERR_OOM, [&] { return block_create(v, &b); }));
        learner_set_upgo_block(l, b, block_free);
    }
    b->prm = *params;  // by value into every later launch
    b->on = true;
    return FI_OK;
}

extern "C" int fi_upgo_disable(fi_learner* l) {
    FI_REQUIRE(l, "upgo_disable: null learner");
    UpgoView v{};
    FI_TRY(learner_upgo_view(l, &v));
    if (v.block) v.block->on = false;
    return FI_OK;
}

extern "C" int fi_upgo_get_state(fi_learner* l, fi_upgo_params* params, fi_upgo_stats* stats, uint32_t* enabled) {
    FI_REQUIRE(l, "upgo_get_state: null learner");
    UpgoView v{};
    FI_TRY(enabled_view(l, "upgo_get_state", &v));
    const UpgoBlock* b = v.block;
    fi_upgo_stats st{};
    FI_HIP_CHECK(hipMemcpyAsync(&st, b->state, sizeof(st), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    if (params) *params = b->prm;
    if (stats) *stats = st;
    if (enabled) *enabled = b->on ? 1u : 0u;
    return FI_OK;
}

extern "C" int fi_upgo_state_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "upgo_state_dev: null argument");
    UpgoView v{};
    FI_TRY(enabled_view(l, "upgo_state_dev", &v));
    *ptr = v.block->state;
    return FI_OK;
}

extern "C" size_t fi_upgo_workspace_bytes(int T, int B, int A) {
    TilePlan p{};
    return tile_plan("upgo_workspace_bytes", T, B, A, &p) == FI_OK ? layout_of(T, B, p).total : 0;
}

extern "C" int fi_upgo_returns_fp32(int T, int B, const float* rewards, const float* discounts, const float* values, float* au,
                                    float* g, uint8_t* up, void* stream) {
    return scan_launch(T, B, rewards, discounts, values, au, g, up, nullptr, (hipStream_t)stream);
}

extern "C" int fi_upgo_term_fp32(int T, int B, int A, const float* logits, const float* mu, const int32_t* actions,
                                 const float* rewards, const float* discounts, const float* values, const fi_upgo_params* params,
                                 float* dlogits, void* stats_dev, void* ws, size_t ws_bytes, void* stream) {
    return term_launch(T, B, A, logits, mu, actions, rewards, discounts, values, params, dlogits, stats_dev, ws, ws_bytes,
                       (hipStream_t)stream, nullptr);
}
