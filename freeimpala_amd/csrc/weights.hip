// weights.hip -- per-column loss weights, and the importance-sampling weights of a prioritised
// ring step that go through them (include/fi_weights.h, gfx950).
//   * scale_columns_kernel: dlogits (T, B, A) and the first T rows of dvalue times w[b] in place,
//     between V-trace and the backward (learner.cpp: run_step). A pure stream: every float is read
//     and written once, 2 * 4 * T * B * (A + 1) bytes; 16 bytes per lane and access, contiguous over
//     the wave, four loads in flight per lane before its first store; no LDS.
//   * prio_is_weights_kernel: one workgroup behind prio_columns_kernel (prio.hip) -- the window's
//     total from the chunk sums that are already there, u_c and its maximum in one strided pass over
//     the columns, the division in a second one.
// The ring's exponents (alpha, beta) live on the handle (ring_handle.h); prio.hip applies alpha in
// its refresh and hands the weights to the step. Stores are ordinary vector stores; no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fi_common.h"
#include "fi_weights.h"
#include "kernels.h"
#include "ring_handle.h"

namespace fi {

namespace {
constexpr int kPiecesPerBlock = 1024;  // 16-byte pieces a workgroup scales: 256 lanes x 4, 16 KiB
constexpr int kChunk = 1024;           // window positions per chunk sum (prio.hip)

// The floats to scale as a run of pieces of up to four floats each. Pieces [0, PL) cover dlogits,
// whole 16-byte pieces but the last (n_l floats: T * B * A need not be a multiple of 4). Behind them
// dvalue's T * B floats: a head piece of `head` floats up to its first 16-byte boundary (dvalue is
// only 4-byte aligned), `body` whole pieces and a tail piece; head and tail may be empty.
struct ScaleMap {
    float* dlog;
    float* dval;
    const float* w;
    uint32_t n_l, PL;               // dlogits: floats, pieces
    uint32_t n_v, head, body;       // dvalue: floats, head floats, whole pieces
    uint32_t A, B;
};

struct Piece {
    float* p;
    uint32_t n;         // floats of the piece that exist: 0 .. 4
    uint32_t col, r, A; // the column of its first float, that float's index inside its row of A, A (dvalue: 1)
};

__device__ __forceinline__ Piece piece_of(const ScaleMap& m, uint32_t g) {
    Piece pc;
    if (g < m.PL) {
        const uint32_t i0 = 4u * g, row = i0 / m.A;  // the column of flat float i is (i / A) mod B
        pc.p = m.dlog + i0;
        pc.n = m.n_l - i0 < 4u ? m.n_l - i0 : 4u;
        pc.col = row % m.B;
        pc.r = i0 - row * m.A;
        pc.A = m.A;
    } else {
        const uint32_t v = g - m.PL;
        uint32_t j0 = 0, n = m.head;
        if (v >= 1u && v <= m.body) {
            j0 = m.head + 4u * (v - 1u);
            n = 4u;
        } else if (v > m.body) {
            j0 = m.head + 4u * m.body;
            n = v == m.body + 1u ? m.n_v - j0 : 0u;
        }
        pc.p = m.dval + j0;
        pc.n = n;
        pc.col = j0 % m.B;
        pc.r = 0u;
        pc.A = 1u;
    }
    return pc;
}

// the weights of the piece's four floats: a piece holds floats of more than one column when A is
// not a multiple of 4 (A = 18, 3), and of four columns in dvalue
__device__ __forceinline__ void piece_weights(const Piece& pc, const float* __restrict__ w, uint32_t B, float (&wk)[4]) {
    uint32_t col = pc.col, r = pc.r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wk[k] = w[col];
        if (++r == pc.A) {
            r = 0u;
            if (++col == B) col = 0u;
        }
    }
}
}  // namespace

// ---------------------------------------------------------------- the scale
__global__ __launch_bounds__(256) void scale_columns_kernel(ScaleMap m, uint32_t pieces) {
    const uint32_t g0 = blockIdx.x * kPiecesPerBlock + threadIdx.x;
    Piece pc[4];
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t g = g0 + 256u * k;
        pc[k].n = 0u;
        if (g < pieces) pc[k] = piece_of(m, g);
        if (pc[k].n == 4u) v[k] = *(const float4*)pc[k].p;  // whole pieces are 16-byte aligned
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (pc[k].n == 0u) continue;
        float wk[4];
        piece_weights(pc[k], m.w, m.B, wk);
        if (pc[k].n == 4u) {
            *(float4*)pc[k].p = make_float4(v[k].x * wk[0], v[k].y * wk[1], v[k].z * wk[2], v[k].w * wk[3]);
        } else {  // dlogits' last piece, dvalue's head and tail: float by float
#pragma unroll
            for (uint32_t i = 0; i < 3u; ++i)
                if (i < pc[k].n) pc[k].p[i] *= wk[i];
        }
    }
}

int scale_columns_launch(float* dlogits, float* dvalue, const float* w, int T, int B, int A, hipStream_t s) {
    FI_REQUIRE(dlogits && dvalue && w, "scale_columns: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1, "scale_columns: T = " + std::to_string(T) + ", B = " + std::to_string(B) +
                                               ", A = " + std::to_string(A) + " must be >= 1");
    FI_REQUIRE((uint64_t)T * (uint64_t)B * (uint64_t)(A + 1) < (1ull << 31),
               "scale_columns: T * B * (A + 1) = " + std::to_string((uint64_t)T * (uint64_t)B * (uint64_t)(A + 1)) +
                   " passes 2^31 - 1");
    FI_REQUIRE((uintptr_t)dlogits % 16 == 0 && (uintptr_t)dvalue % 4 == 0 && (uintptr_t)w % 4 == 0,
               "scale_columns: dlogits must be 16-byte, dvalue and w 4-byte aligned");
    ScaleMap m{};
    m.dlog = dlogits;
    m.dval = dvalue;
    m.w = w;
    m.A = (uint32_t)A;
    m.B = (uint32_t)B;
    m.n_l = (uint32_t)T * (uint32_t)B * (uint32_t)A;
    m.PL = (m.n_l + 3u) / 4u;
    m.n_v = (uint32_t)T * (uint32_t)B;
    const uint32_t to_boundary = (uint32_t)((16u - (uintptr_t)dvalue % 16u) % 16u) / 4u;
    m.head = to_boundary < m.n_v ? to_boundary : m.n_v;
    m.body = (m.n_v - m.head) / 4u;
    const uint32_t pieces = m.PL + m.body + 2u;  // dvalue: head, body, tail
    hipLaunchKernelGGL(scale_columns_kernel, dim3((pieces + kPiecesPerBlock - 1) / kPiecesPerBlock), dim3(256), 0, s, m,
                       pieces);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- the importance weights
// One workgroup. Q: lane i adds the chunk sums i, i + 256, ... (at most four: capacity <= 2^20), then
// a reduction over the wave and the four waves through LDS. Pass 1: column c = i, i + 256, ...
// stores u_c and keeps the largest; the same reduction for the maximum. Pass 2: every lane divides
// the u it stored itself. Reads 8 * n_chunks + 12 * B bytes, writes 8 * B.
__global__ __launch_bounds__(256) void prio_is_weights_kernel(const uint64_t* __restrict__ entries, int B, int n_fresh,
                                                              const uint32_t* __restrict__ table, uint32_t C,
                                                              uint32_t n_valid, const uint64_t* __restrict__ sums,
                                                              uint32_t n_chunks, float beta, float* __restrict__ w_out) {
    __shared__ uint64_t q_part[4];
    __shared__ float m_part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t Q = 0;
    for (uint32_t k = threadIdx.x; k < n_chunks; k += 256u) Q += sums[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t a = __shfl_xor((uint32_t)Q, off, 64), b = __shfl_xor((uint32_t)(Q >> 32), off, 64);
        Q += (uint64_t)a | ((uint64_t)b << 32);
    }
    if (lane == 0) q_part[wave] = Q;
    __syncthreads();
    Q = q_part[0] + q_part[1] + q_part[2] + q_part[3];
    const double scale = (double)n_valid, total = (double)Q;
    float m = -1.f;  // below every u: u > 0, and lanes without a column hold no candidate
    for (int c = threadIdx.x; c < B; c += 256) {
        float u = 1.f;
        if (c >= n_fresh) {
            const uint32_t q = table[(uint32_t)(entries[c] % (uint64_t)C)];
            const double ratio = (double)q * scale / total;  // the product is below 2^51: exact
            u = powf((float)ratio, -beta);
        }
        w_out[c] = u;
        m = fmaxf(m, u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) m_part[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(m_part[0], m_part[1]), fmaxf(m_part[2], m_part[3]));
    for (int c = threadIdx.x; c < B; c += 256) w_out[c] = w_out[c] / m;
}

int prio_is_weights_launch(const uint64_t* entries, int B, int n_fresh, const uint32_t* table, int64_t C, uint64_t lo,
                           uint64_t n_valid, const uint64_t* sums, float beta, float* w_out, hipStream_t s) {
    FI_REQUIRE(entries && w_out && B >= 1, "prio_is_weights: bad arguments");
    FI_REQUIRE(beta >= 0.f && beta <= 1.f, "prio_is_weights: beta " + std::to_string(beta) + " outside [0, 1]");
    FI_REQUIRE(C >= 1 && C <= FI_PRIO_MAX_CAPACITY,
               "prio_is_weights: capacity " + std::to_string(C) + " outside 1 .. 2^20 = 1048576");
    FI_REQUIRE(n_fresh >= 0 && n_fresh <= B, "prio_is_weights: n_fresh " + std::to_string(n_fresh) + " outside 0 .. B = " +
                                                 std::to_string(B));
    FI_REQUIRE(n_valid <= (uint64_t)C && (n_fresh == B || n_valid >= 1),
               "prio_is_weights: n_valid " + std::to_string(n_valid) + " outside 1 .. capacity (lo " + std::to_string(lo) +
                   ")");
    FI_REQUIRE((uintptr_t)entries % 8 == 0 && (uintptr_t)w_out % 4 == 0,
               "prio_is_weights: entries must be 8-byte, w_out 4-byte aligned");
    uint32_t n_chunks = 0;
    if (n_fresh < B) {
        FI_REQUIRE(table && sums && (uintptr_t)table % 4 == 0 && (uintptr_t)sums % 8 == 0,
                   "prio_is_weights: table (4-byte aligned) and chunk_ws (8-byte aligned) are needed");
        n_chunks = (uint32_t)((n_valid + kChunk - 1) / kChunk);
    }
    hipLaunchKernelGGL(prio_is_weights_kernel, dim3(1), dim3(256), 0, s, entries, B, n_fresh, table, (uint32_t)C,
                       (uint32_t)n_valid, sums, n_chunks, beta, w_out);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

using namespace fi;

// ------------------------------------------------------------------ the learner's column weights
// the handle is learner.cpp's, which takes the launcher as a pointer (kernels.h)
extern "C" int fi_learner_set_column_weights(fi_learner* l, const float* w_host, int32_t n) {
    return learner_set_column_weights(l, w_host, n, scale_columns_launch);
}

extern "C" int fi_learner_clear_column_weights(fi_learner* l) { return learner_clear_column_weights(l); }

extern "C" int fi_learner_column_weights(fi_learner* l, float* dst, int32_t n) {
    return learner_column_weights(l, dst, n);
}

// ------------------------------------------------------------------ the ring's exponents
extern "C" int fi_prio_set_exponents(fi_ring* r, float alpha, float beta) {
    FI_REQUIRE(r, "prio_set_exponents: null ring");
    if (!r->prio_on) return fail(FI_ERR_STATE, "prio_set_exponents: priorities are not enabled (fi_prio_enable)");
    FI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "prio_set_exponents: alpha " + std::to_string(alpha) + " outside [0, 1]");
    FI_REQUIRE(beta >= 0.f && beta <= 1.f, "prio_set_exponents: beta " + std::to_string(beta) + " outside [0, 1]");
    r->alpha = alpha;
    r->beta = beta;
    return FI_OK;
}

extern "C" int fi_prio_exponents(const fi_ring* r, fi_prio_exponents_state* out) {
    FI_REQUIRE(r && out, "prio_exponents: null argument");
    if (!r->prio_on) return fail(FI_ERR_STATE, "prio_exponents: priorities are not enabled (fi_prio_enable)");
    *out = fi_prio_exponents_state{r->alpha, r->beta, r->is_w_valid ? 1u : 0u, 0u};
    return FI_OK;
}

extern "C" int fi_prio_last_weights(fi_ring* r, int32_t n, float* dst) {
    FI_REQUIRE(r && dst, "prio_last_weights: null argument");
    if (!r->prio_on) return fail(FI_ERR_STATE, "prio_last_weights: priorities are not enabled (fi_prio_enable)");
    FI_REQUIRE(n >= 1, "prio_last_weights: n = " + std::to_string(n) + " < 1");
    if (!r->is_w_valid) {
        for (int32_t i = 0; i < n; ++i) dst[i] = 1.f;
        return FI_OK;
    }
    FI_REQUIRE(n == r->last_n, "prio_last_weights: n = " + std::to_string(n) + " != the last step's batch " +
                                   std::to_string(r->last_n));
    FI_HIP_CHECK(hipSetDevice(r->dev));
    if (r->have_prio_done) FI_HIP_CHECK(hipEventSynchronize(r->prio_done));
    FI_HIP_CHECK(hipMemcpy(dst, r->is_w, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return FI_OK;
}

// ------------------------------------------------------------------ standalone kernels
extern "C" int fi_weights_scale_columns(float* dlogits, float* dvalue, const float* w, int32_t T, int32_t B, int32_t A,
                                        void* stream) {
    return scale_columns_launch(dlogits, dvalue, w, T, B, A, (hipStream_t)stream);
}

extern "C" int fi_prio_is_weights(const uint64_t* entries_dev, int32_t B, int32_t n_fresh, const uint32_t* table,
                                  int64_t capacity, uint64_t lo, uint64_t n_valid, const void* chunk_ws, float beta,
                                  float* w_out, void* stream) {
    return prio_is_weights_launch(entries_dev, B, n_fresh, table, capacity, lo, n_valid, (const uint64_t*)chunk_ws, beta,
                                  w_out, (hipStream_t)stream);
}
