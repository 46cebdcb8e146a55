// mlp_bf16.hip -- the MLP policy's bf16 mode (include/fi_mlp.h): bf16 operands, fp32 accumulation on
// v_mfma_f32_32x32x16_bf16, bf16 stored activations and data gradients, fp32 everything else.
//
// One fragment layout serves every operand of every kernel here. A 32x32x16 MFMA reads, per lane, the 8
// consecutive k of one row (A) or one column (B): lane = 32 * ((k >> 3) & 1) + (index & 31). An operand
// tile of 32 indices x 16 k is therefore 64 pieces of 16 bytes, and an operand of `tiles` x KS such tiles
// is laid out tile-major, k-step next: a wave reads one MFMA operand as one 16-byte load per lane.
//   * weight images (global memory, mlp_weights_bf16_kernel): the pieces follow one another, 1 KiB per
//     (tile, k-step), so the GEMM loops below load B straight into registers from L2;
//   * LDS: the same order with 16 bytes of padding behind each 32-lane half (528 bytes), so that the
//     2-byte writes of an epilogue or of a transposing stage land in different banks.
// The forward is one launch: a workgroup of 4 waves owns 64 rows, and the rounded h1 / h2 go to global
// memory and, in A-operand order, to LDS for the next layer. K runs in ascending k-steps in every
// kernel and nothing is split over K in the forward, so a row's result depends on that row alone.
// The weight gradients are X^T dY over row slices: both operands have the rows as their K, so a chunk of
// 64 rows is transposed on its way into LDS, each wave accumulates up to 8 output tiles across the
// slice's chunks, and the slice's fp32 slab is summed by reduce_slabs in a fixed order. No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "fi_common.h"
#include "fi_mlp.h"
#include "kernels.h"

namespace fi {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRows = 64;    // rows of a forward / data-gradient tile, and of a weight-gradient chunk
constexpr int kHalf = 528;   // LDS bytes of one 32-lane half of a fragment: 512 + 16 of padding
constexpr int kFwdThreads = 256, kBwdThreads = 512;

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// the images of one parameter slab, in elements from the image's start
struct Images {
    int ks1, ksh, kso, nth, nto;  // k-steps of D, H, A + 1; 32-wide tiles of H, A + 1
    size_t w1, w2, wh, w2t, wht, total;
};
__host__ __device__ inline Images images_of(int D, int H, int A) {
    Images L;
    const int O = A + 1;
    L.ks1 = cdiv(D, 16), L.ksh = H / 16, L.kso = cdiv(O, 16), L.nth = H / 32, L.nto = cdiv(O, 32);
    L.w1 = 0;
    L.w2 = L.w1 + (size_t)L.nth * L.ks1 * 512;
    L.wh = L.w2 + (size_t)L.nth * L.ksh * 512;
    L.w2t = L.wh + (size_t)L.nto * L.ksh * 512;
    L.wht = L.w2t + (size_t)L.nth * L.ksh * 512;
    L.total = L.wht + (size_t)L.nth * L.kso * 512;
    return L;
}

__device__ __forceinline__ int lds_at(int KS, int k, int idx) {  // byte offset of element (k, idx)
    return (((idx >> 5) * KS + (k >> 4)) * 2 + ((k >> 3) & 1)) * kHalf + (idx & 31) * 16 + (k & 7) * 2;
}
__device__ __forceinline__ bf16x8 lds_frag(const char* lds, int KS, int tile, int ks, int lane) {
    return *(const bf16x8*)(lds + ((tile * KS + ks) * 2 + (lane >> 5)) * kHalf + (lane & 31) * 16);
}
__host__ __device__ inline int lds_bytes(int tiles, int KS) { return tiles * KS * 2 * kHalf; }

// ------------------------------------------------------------------ the weight images
__global__ __launch_bounds__(256) void mlp_weights_bf16_kernel(const float* __restrict__ p, int D, int H, int A,
                                                               __bf16* __restrict__ img) {
    const Images L = images_of(D, H, A);
    const int O = A + 1;
    const float* W1 = p;
    const float* W2 = W1 + (size_t)D * H + H;
    const float* Wh = W2 + (size_t)H * H + H;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < L.total; e += (size_t)gridDim.x * blockDim.x) {
        const int seg = e < L.w2 ? 0 : e < L.wh ? 1 : e < L.w2t ? 2 : e < L.wht ? 3 : 4;
        const size_t base = seg == 0 ? L.w1 : seg == 1 ? L.w2 : seg == 2 ? L.wh : seg == 3 ? L.w2t : L.wht;
        const int KS = seg == 0 ? L.ks1 : seg == 4 ? L.kso : L.ksh;
        const size_t loc = e - base;
        const int lane = (int)(loc >> 3) & 63, t = (int)(loc >> 9);
        const int k = (t % KS) * 16 + (lane >> 5) * 8 + (int)(loc & 7), n = (t / KS) * 32 + (lane & 31);
        float v = 0.f;
        if (seg == 0) v = k < D ? W1[(size_t)k * H + n] : 0.f;
        else if (seg == 1) v = W2[(size_t)k * H + n];
        else if (seg == 2) v = n < O ? Wh[(size_t)k * O + n] : 0.f;
        else if (seg == 3) v = W2[(size_t)n * H + k];
        else v = k < O ? Wh[(size_t)n * O + k] : 0.f;
        img[e] = (__bf16)v;
    }
}

// ------------------------------------------------------------------ operand sources: 8 elements (r, c0 .. c0 + 7)
struct SrcBf16 {  // (M, C) bf16, C a multiple of 8
    const __bf16* p;
    int M, C;
    __device__ __forceinline__ bf16x8 get(int r, int c0) const {
        bf16x8 o = {};
        if (r < M && c0 < C) o = *(const bf16x8*)(p + (size_t)r * C + c0);
        return o;
    }
};
struct SrcF32 {  // (M, C) fp32, any C: rounded here
    const float* p;
    int M, C;
    __device__ __forceinline__ bf16x8 get(int r, int c0) const {
        bf16x8 o = {};
        if (r >= M) return o;
        const float* q = p + (size_t)r * C;
        if ((C & 3) == 0 && c0 + 8 <= C && ((uintptr_t)p & 15) == 0) {
            const float4 a = *(const float4*)(q + c0), b = *(const float4*)(q + c0 + 4);
            o = bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = c0 + e < C ? (__bf16)q[c0 + e] : (__bf16)0.f;
        }
        return o;
    }
};
struct SrcHeads {  // the heads' upstream gradient [dlogits | dvalue], rows past T B without dlogits
    HeadsGrad g;
    __device__ __forceinline__ bf16x8 get(int r, int c0) const {
        bf16x8 o = {};
        if (r >= g.rows) return o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            float v = 0.f;
            if (c < g.A) v = r < g.TB ? g.dlog[(size_t)r * g.A + c] : 0.f;
            else if (c == g.A) v = g.dval[r];
            o[e] = (__bf16)v;
        }
        return o;
    }
};

// 64 rows x (16 KS) columns into A-operand order: the rows are the MFMA's M, the columns its K
template <class Src>
__device__ __forceinline__ void stage_rows(char* lds, int KS, const Src& src, int row0, int tid, int nthr) {
    const int per = KS * 2;
    for (int p = tid; p < kRows * per; p += nthr) {
        const int r = p / per, kp = p - r * per;
        *(bf16x8*)(lds + lds_at(KS, kp * 8, r)) = src.get(row0 + r, kp * 8);
    }
}
// 64 rows x (32 tiles) columns transposed: the rows are the MFMA's K (4 k-steps), the columns M or N.
// A wave takes 64 rows of one 8-column piece, so its 2-byte writes spread over the padded halves
template <class Src>
__device__ __forceinline__ void stage_cols(char* lds, int tiles, const Src& src, int row0, int tid, int nthr) {
    for (int p = tid; p < kRows * tiles * 4; p += nthr) {
        const int cp = p >> 6, r = p & 63;
        const bf16x8 v = src.get(row0 + r, cp * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) *(__bf16*)(lds + lds_at(4, r, cp * 8 + e)) = v[e];
    }
}

// 64 rows (A-order in LDS) times the image's column tiles ct = wave, wave + nw, ..: epi(row tile, ct, acc)
template <class Epi>
__device__ __forceinline__ void gemm_rows(const char* ldsA, int KS, const __bf16* img, int nct, int wave, int nw, int lane,
                                          Epi&& epi) {
    for (int ct = wave; ct < nct; ct += nw) {
        f32x16 c0 = {}, c1 = {};
        const bf16x8* bp = (const bf16x8*)img + (size_t)ct * KS * 64 + lane;
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 b = bp[ks * 64];
            c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(ldsA, KS, 0, ks, lane), b, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(ldsA, KS, 1, ks, lane), b, c1, 0, 0, 0);
        }
        epi(0, ct, c0);
        epi(1, ct, c1);
    }
}
// accumulator register v of a lane: row (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3), column lane & 31
__device__ __forceinline__ int acc_row(int v, int lane) { return (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3); }

// ------------------------------------------------------------------ forward
__global__ __launch_bounds__(kFwdThreads) void mlp_fwd_fused_bf16_kernel(const float* __restrict__ obs, int M, int D, int H,
                                                                         int A, const __bf16* __restrict__ img,
                                                                         const float* __restrict__ params,
                                                                         __bf16* __restrict__ h1, __bf16* __restrict__ h2,
                                                                         float* __restrict__ logits, float* __restrict__ values) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Images L = images_of(D, H, A);
    char* bufA = lds;  // the observation tile, then h2
    char* bufB = lds + lds_bytes(2, L.ks1 > L.ksh ? L.ks1 : L.ksh);  // h1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kRows;
    const float* b1 = params + (size_t)D * H;
    const float* b2 = b1 + H + (size_t)H * H;
    const float* bh = b2 + H + (size_t)H * (A + 1);

    stage_rows(bufA, L.ks1, SrcF32{obs, M, D}, row0, tid, kFwdThreads);
    __syncthreads();
    auto hidden = [&](const float* bias, __bf16* out, char* next) {
        return [=](int rt, int ct, const f32x16& c) {
            const int col = ct * 32 + (lane & 31);
            const float b = bias[col];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = rt * 32 + acc_row(v, lane);
                const __bf16 y = (__bf16)fmaxf(c[v] + b, 0.f);
                if (row0 + r < M) out[(size_t)(row0 + r) * H + col] = y;
                *(__bf16*)(next + lds_at(H / 16, col, r)) = y;
            }
        };
    };
    gemm_rows(bufA, L.ks1, img + L.w1, L.nth, wave, 4, lane, hidden(b1, h1, bufB));
    __syncthreads();
    gemm_rows(bufB, L.ksh, img + L.w2, L.nth, wave, 4, lane, hidden(b2, h2, bufA));
    __syncthreads();
    gemm_rows(bufA, L.ksh, img + L.wh, L.nto, wave, 4, lane, [=](int rt, int ct, const f32x16& c) {
        const int col = ct * 32 + (lane & 31);
        if (col > A) return;
        const float b = bh[col];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = row0 + rt * 32 + acc_row(v, lane);
            if (r >= M) continue;
            if (col < A) logits[(size_t)r * A + col] = c[v] + b;
            else values[r] = c[v] + b;
        }
    });
}

// ------------------------------------------------------------------ dz1 = (dz2 . W2^T) * [h1 > 0]
__global__ __launch_bounds__(kFwdThreads) void mlp_dgrad_bf16_kernel(const __bf16* __restrict__ dy, int M, int H,
                                                                     const __bf16* __restrict__ wT,
                                                                     const __bf16* __restrict__ act, __bf16* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kRows, KS = H / 16;
    stage_rows(lds, KS, SrcBf16{dy, M, H}, row0, tid, kFwdThreads);
    __syncthreads();
    gemm_rows(lds, KS, wT, H / 32, wave, 4, lane, [=](int rt, int ct, const f32x16& c) {
        const int col = ct * 32 + (lane & 31);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = row0 + rt * 32 + acc_row(v, lane);
            if (r >= M) continue;
            const size_t at = (size_t)r * H + col;
            dx[at] = (float)act[at] > 0.f ? (__bf16)c[v] : (__bf16)0.f;
        }
    });
}

// ------------------------------------------------------------------ weight gradients over row slices
// One slice: G (I x N) = X^T dY over the slice's chunks of 64 rows, and the column sums of dY. The
// nIt x nNt output tiles are dealt to the 8 waves in runs of tpw <= Q (tile id = it * nNt + nt).
// HEADS: X = h2 and dY = [dlogits | dvalue]; the same pass writes dz2 = (dY . Wh^T) * [h2 > 0].
template <class XS, class YS, bool HEADS, int Q>
__device__ __forceinline__ void wgrad_slice(char* lds, const XS& xs, const YS& ys, int M, int I, int N, int cps,
                                            float* __restrict__ slab, float* __restrict__ cs, const __bf16* whT, int kso,
                                            const __bf16* h2, __bf16* dz2) {
    const int nIt = cdiv(I, 32), nNt = cdiv(N, 32), total = nIt * nNt, tpw = cdiv(total, 8);
    char* ldsX = lds;
    char* ldsY = ldsX + lds_bytes(nIt, 4);
    char* ldsD = ldsY + lds_bytes(nNt, 4);  // HEADS: dY once more, in A-operand order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = cdiv(M, kRows), c_lo = blockIdx.x * cps, c_hi = min(chunks, c_lo + cps);
    f32x16 acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = f32x16{};
    float bsum = 0.f;
    for (int ch = c_lo; ch < c_hi; ++ch) {
        const int row0 = ch * kRows;
        __syncthreads();  // the chunk before this one has been read
        stage_cols(ldsX, nIt, xs, row0, tid, kBwdThreads);
        stage_cols(ldsY, nNt, ys, row0, tid, kBwdThreads);
        if constexpr (HEADS) stage_rows(ldsD, kso, ys, row0, tid, kBwdThreads);
        __syncthreads();
        if (tid < nNt * 32) {  // column tid of dY: its 64 rows in ascending order
            for (int g = 0; g < 8; ++g) {
                const bf16x8 v = *(const bf16x8*)(ldsY + lds_at(4, g * 8, tid));
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum += (float)v[e];
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int id = wave * tpw + q;
            if (q < tpw && id < total) {
                const int it = id / nNt, nt = id - it * nNt;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_frag(ldsX, 4, it, ks, lane),
                                                                    lds_frag(ldsY, 4, nt, ks, lane), acc[q], 0, 0, 0);
            }
        }
        if constexpr (HEADS) {
            const int H = I;
            gemm_rows(ldsD, kso, whT, H / 32, wave, 8, lane, [=](int rt, int ct, const f32x16& c) {
                const int col = ct * 32 + (lane & 31);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = row0 + rt * 32 + acc_row(v, lane);
                    if (r >= M) continue;
                    const size_t at = (size_t)r * H + col;
                    dz2[at] = (float)h2[at] > 0.f ? (__bf16)c[v] : (__bf16)0.f;
                }
            });
        }
    }
    float* out = slab + (size_t)blockIdx.x * I * N;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int id = wave * tpw + q;
        if (q < tpw && id < total) {
            const int it = id / nNt, nt = id - it * nNt, n = nt * 32 + (lane & 31);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = it * 32 + acc_row(v, lane);
                if (i < I && n < N) out[(size_t)i * N + n] = acc[q][v];
            }
        }
    }
    if (tid < N) cs[(size_t)blockIdx.x * N + tid] = bsum;
}

template <class XS>
__global__ __launch_bounds__(kBwdThreads) void mlp_wgrad_bf16_kernel(XS xs, SrcBf16 ys, int M, int I, int N, int cps,
                                                                     float* __restrict__ slab, float* __restrict__ cs) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    wgrad_slice<XS, SrcBf16, false, 8>(lds, xs, ys, M, I, N, cps, slab, cs, nullptr, 0, nullptr, nullptr);
}

__global__ __launch_bounds__(kBwdThreads) void mlp_heads_bwd_bf16_kernel(SrcBf16 h2, SrcHeads g, int H, int cps,
                                                                         const __bf16* __restrict__ whT, int kso,
                                                                         __bf16* __restrict__ dz2, float* __restrict__ slab,
                                                                         float* __restrict__ cs) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    wgrad_slice<SrcBf16, SrcHeads, true, 3>(lds, h2, g, g.g.rows, H, g.g.A + 1, cps, slab, cs, whT, kso, h2.p, dz2);
}

template <class K>
int allow_lds(K kernel, int bytes) {
    FI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return FI_OK;
}

}  // namespace

// ------------------------------------------------------------------ launchers
bool mlp_bf16_supported(int D, int H, int A) {
    return D >= 1 && D <= 128 && H >= 32 && H <= 256 && H % 32 == 0 && A >= 2 && A <= 64;
}
size_t mlp_bf16_image_elems(int D, int H, int A) { return images_of(D, H, A).total; }

int mlp_weights_bf16(const float* params, int D, int H, int A, __bf16* img, hipStream_t s) {
    const size_t n = images_of(D, H, A).total;
    hipLaunchKernelGGL(mlp_weights_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, params, D, H, A, img);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int mlp_fwd_fused_bf16(const float* obs, int M, int D, int H, int A, const __bf16* img, const float* params, __bf16* h1,
                       __bf16* h2, float* logits, float* values, hipStream_t s) {
    const Images L = images_of(D, H, A);
    const int bytes = lds_bytes(2, std::max(L.ks1, L.ksh)) + lds_bytes(2, L.ksh);
    FI_TRY(allow_lds(mlp_fwd_fused_bf16_kernel, bytes));
    hipLaunchKernelGGL(mlp_fwd_fused_bf16_kernel, dim3((unsigned)cdiv(M, kRows)), dim3(kFwdThreads), bytes, s, obs, M, D, H, A,
                       img, params, h1, h2, logits, values);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int mlp_dgrad_bf16(const __bf16* dz2, int M, int D, int H, int A, const __bf16* img, const __bf16* h1, __bf16* dz1,
                   hipStream_t s) {
    const int bytes = lds_bytes(2, H / 16);
    FI_TRY(allow_lds(mlp_dgrad_bf16_kernel, bytes));
    hipLaunchKernelGGL(mlp_dgrad_bf16_kernel, dim3((unsigned)cdiv(M, kRows)), dim3(kFwdThreads), bytes, s, dz2, M, H,
                       img + images_of(D, H, A).w2t, h1, dz1);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// slab: splits x (I x N) floats, cs: splits x N floats; every slice writes all of its part
int mlp_wgrad_bf16(const void* X, bool x_f32, int M, int I, const __bf16* dY, int N, int splits, float* slab, float* cs,
                   hipStream_t s) {
    const int cps = cdiv(cdiv(M, kRows), splits), bytes = lds_bytes(cdiv(I, 32) + cdiv(N, 32), 4);
    const SrcBf16 ys{dY, M, N};
    if (x_f32) {
        FI_TRY(allow_lds(mlp_wgrad_bf16_kernel<SrcF32>, bytes));
        hipLaunchKernelGGL(mlp_wgrad_bf16_kernel<SrcF32>, dim3((unsigned)splits), dim3(kBwdThreads), bytes, s,
                           SrcF32{(const float*)X, M, I}, ys, M, I, N, cps, slab, cs);
    } else {
        FI_TRY(allow_lds(mlp_wgrad_bf16_kernel<SrcBf16>, bytes));
        hipLaunchKernelGGL(mlp_wgrad_bf16_kernel<SrcBf16>, dim3((unsigned)splits), dim3(kBwdThreads), bytes, s,
                           SrcBf16{(const __bf16*)X, M, I}, ys, M, I, N, cps, slab, cs);
    }
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int mlp_heads_bwd_bf16(const HeadsGrad& g, const __bf16* h2, const __bf16* img, int D, int H, __bf16* dz2, int splits,
                       float* slab, float* cs, hipStream_t s) {
    const Images L = images_of(D, H, g.A);
    const int cps = cdiv(cdiv(g.rows, kRows), splits);
    const int bytes = lds_bytes(L.nth + L.nto, 4) + lds_bytes(2, L.kso);
    FI_TRY(allow_lds(mlp_heads_bwd_bf16_kernel, bytes));
    hipLaunchKernelGGL(mlp_heads_bwd_bf16_kernel, dim3((unsigned)splits), dim3(kBwdThreads), bytes, s,
                       SrcBf16{h2, g.rows, H}, SrcHeads{g}, H, cps, img + L.wht, L.kso, dz2, slab, cs);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

// ------------------------------------------------------------------ fi_mlp.h
static const fi::MlpBf16Ops kOps{fi::mlp_bf16_supported, fi::mlp_bf16_image_elems, fi::mlp_weights_bf16, fi::mlp_fwd_fused_bf16,
                                 fi::mlp_heads_bwd_bf16,  fi::mlp_dgrad_bf16,       fi::mlp_wgrad_bf16};
extern "C" int fi_learner_set_mlp_precision(fi_learner* l, int prec) { return fi::learner_set_mlp_precision(l, prec, &kOps); }
extern "C" int fi_learner_mlp_precision(const fi_learner* l) { return fi::learner_mlp_precision(l); }
extern "C" int fi_actor_set_mlp_precision(fi_actor* a, int prec) { return fi::actor_set_mlp_precision(a, prec, &kOps); }
