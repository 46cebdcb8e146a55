// row_stream.h -- what the loss-side streams over the logits share (diag.hip, surrogate.hip, target.hip,
// kl.hip; the reductions also vtrace.hip). Internal, header-only. The pattern: workgroup (c, s) owns the
// 64 columns of column tile c and the time steps of slice s (tile_plan), its four waves the steps
// t .. t + 3 of a round, lane = column. The rows of one (t, tile) are one contiguous run of nb * A floats
// in global memory: load_run moves it, 16 bytes per lane and access, into the wave's padded LDS rows,
// then one lane works per row; store_run is the way back, add_run the way onto a tensor that holds
// values already (kl.hip). Row stride in LDS: A | 1 floats. ds_read_b32 is served
// in two groups of 32 lanes over 32 banks, so a stride of A floats is a 2-way conflict at A = 18 and a
// 32-way one at A = 64 in each group; an odd stride maps the 32 lanes of a group to 32 different banks.
// A workgroup's fp64 sums are reduced per wave by DPP / permlane moves (wave_reduce) and over the waves
// through LDS (block_sums), in one fixed order. A new loss-side stream starts from this header; a
// second copy of any of it goes here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fi_common.h"

namespace fi {

constexpr int kCols = 64;          // columns per workgroup: lane = column
constexpr int kWaves = 4;          // waves per workgroup of a stream: one time step each per round
constexpr int kTargetWgs = 768;    // three workgroups per CU at B = 4096: the slices of T fill the chip
constexpr int kPiecesPerLane = 5;  // 16-byte pieces a lane has in flight per tensor (A = 18: 4.5 per lane and run)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr float L2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// ---------------------------------------------------------------- reductions
// Wave-wide reduction of a double in VALU cross-lane moves: rotations 8, 4, 2, 1 inside each 16-lane
// row by DPP, then the row pairs and halves by gfx950's v_permlane16_swap / v_permlane32_swap. No trip
// through the LDS crossbar, which a shuffle takes (ds_bpermute): with some twenty doubles per wave to
// reduce, shuffles cost the two launches of the diagnostics 6 us of 46 at T = 100, B = 4096 and 8 of 23
// at T = 20, B = 256 (scripts/diag_bench.py, before and after). The order is fixed, so the result is
// deterministic; every lane ends with it.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)u, CTRL, 0xf, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int S>
__device__ __forceinline__ double xor_d(double v, int lane) {  // v of lane ^ S, S = 16 or 32
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    unsigned rlo, rhi;
    if constexpr (S == 16) {
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        rlo = (lane & 16) ? a[0] : a[1];
        rhi = (lane & 16) ? b[0] : b[1];
    } else {
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        rlo = (lane & 32) ? a[0] : a[1];
        rhi = (lane & 32) ? b[0] : b[1];
    }
    return __longlong_as_double((long long)(((unsigned long long)rhi << 32) | rlo));
}
enum { OP_SUM, OP_MAX, OP_MIN };
// op is a constant wherever a kernel's sums are combined over a wave; over the waves diag.hip lets
// thread i combine quantity i, so there it is a run-time value
__device__ __forceinline__ double combine(int op, double x, double y) {
    return op == OP_SUM ? x + y : (op == OP_MAX ? fmax(x, y) : fmin(x, y));
}
template <int OP = OP_SUM>
__device__ __forceinline__ double wave_reduce(double v, int lane) {
    v = combine(OP, v, dpp_d<0x128>(v));  // row_ror:8
    v = combine(OP, v, dpp_d<0x124>(v));  // row_ror:4
    v = combine(OP, v, dpp_d<0x122>(v));  // row_ror:2
    v = combine(OP, v, dpp_d<0x121>(v));  // row_ror:1
    v = combine(OP, v, xor_d<16>(v, lane));
    v = combine(OP, v, xor_d<32>(v, lane));
    return v;
}

// N sums of a workgroup of NW waves through LDS (red: NW * N doubles), the waves added in ascending
// order; every thread gets the results. A barrier stands in front of the writes, so red may have been
// read just before.
template <int N, int NW>
__device__ __forceinline__ void block_sums(double (&v)[N], double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_reduce(v[i], lane);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[w * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = red[i];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) s += red[w2 * N + i];
        v[i] = s;
    }
}

// ---------------------------------------------------------------- the run of one (t, tile)
// The run of nb * A floats of one (t, tile) from global memory into the wave's padded LDS rows, 16
// bytes per lane and access, consecutive lanes consecutive pieces; a head and a tail of up to 3 floats
// where the run does not start or end on a 16-byte boundary (A = 3, 18 and odd B * A occur). The
// padding costs the 16-byte LDS store (a padded row does not start on a 16-byte boundary): the pieces
// go in as four ds_write_b32, which is not what limits a kernel that moves 69 MB through HBM.
// g0 < 2^31 (tile_plan's check), so 32-bit indices do. kMu: the mu rows go with the pi rows.
template <bool kMu>
__device__ __forceinline__ void load_run(const float* __restrict__ pi, const float* __restrict__ mu, float* __restrict__ lp,
                                         float* __restrict__ lm, uint32_t g0, uint32_t n, uint32_t A, uint32_t S, int lane) {
    const uint32_t to4 = (4u - (g0 & 3u)) & 3u, head = to4 < n ? to4 : n;
    const uint32_t nbody = (n - head) >> 2, tail = n - head - 4u * nbody;
    const float* __restrict__ gp = pi + g0;
    const float* __restrict__ gm = mu + g0;
    const f32x4* __restrict__ gp4 = (const f32x4*)(gp + head);  // 16-byte aligned: (g0 + head) % 4 == 0
    const f32x4* __restrict__ gm4 = (const f32x4*)(gm + head);
    for (uint32_t k0 = 0; k0 < nbody; k0 += 64u * kPiecesPerLane) {
        f32x4 vp[kPiecesPerLane], vm[kPiecesPerLane];
#pragma unroll
        for (int u = 0; u < kPiecesPerLane; ++u) {
            const uint32_t p = k0 + 64u * u + lane;
            if (p < nbody) {
                vp[u] = __builtin_nontemporal_load(gp4 + p);
                if (kMu) vm[u] = __builtin_nontemporal_load(gm4 + p);
            }
        }
#pragma unroll
        for (int u = 0; u < kPiecesPerLane; ++u) {
            const uint32_t p = k0 + 64u * u + lane;
            if (p < nbody) {
                const uint32_t e = head + 4u * p;
                uint32_t r = e / A, cc = e - r * A;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lp[r * S + cc] = vp[u][j];
                    if (kMu) lm[r * S + cc] = vm[u][j];
                    if (++cc == A) {
                        cc = 0u;
                        ++r;
                    }
                }
            }
        }
    }
    if ((uint32_t)lane < head) {
        const uint32_t r = (uint32_t)lane / A, cc = (uint32_t)lane - r * A;
        lp[r * S + cc] = gp[lane];
        if (kMu) lm[r * S + cc] = gm[lane];
    }
    if ((uint32_t)lane < tail) {
        const uint32_t e = head + 4u * nbody + lane, r = e / A, cc = e - r * A;
        lp[r * S + cc] = gp[e];
        if (kMu) lm[r * S + cc] = gm[e];
    }
}

// the reverse: the wave's padded LDS rows leave as the run's 16-byte pieces
__device__ __forceinline__ void store_run(float* __restrict__ out, const float* __restrict__ lp, uint32_t g0, uint32_t n,
                                          uint32_t A, uint32_t S, int lane) {
    const uint32_t to4 = (4u - (g0 & 3u)) & 3u, head = to4 < n ? to4 : n;
    const uint32_t nbody = (n - head) >> 2, tail = n - head - 4u * nbody;
    float* __restrict__ go = out + g0;
    f32x4* __restrict__ go4 = (f32x4*)(go + head);
    for (uint32_t p = lane; p < nbody; p += 64u) {
        const uint32_t e = head + 4u * p;
        uint32_t r = e / A, cc = e - r * A;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = lp[r * S + cc];
            if (++cc == A) {
                cc = 0u;
                ++r;
            }
        }
        go4[p] = v;
    }
    if ((uint32_t)lane < head) {
        const uint32_t r = (uint32_t)lane / A, cc = (uint32_t)lane - r * A;
        go[lane] = lp[r * S + cc];
    }
    if ((uint32_t)lane < tail) {
        const uint32_t e = head + 4u * nbody + lane, r = e / A, cc = e - r * A;
        go[e] = lp[r * S + cc];
    }
}

// store_run's traversal onto a tensor that holds values already: out[e] += the LDS row value. The
// rows do not go through LDS a second time (kl.hip: a third padded row set does not fit a CU at A = 64):
// a lane loads up to kPiecesPerLane of its 16-byte pieces together, adds and stores them. Each element of
// the run is read once and written once, by the same lane; plain loads and stores, since out was written
// by the launch in front and is read again by the one behind.
__device__ __forceinline__ void add_run(float* __restrict__ out, const float* __restrict__ lp, uint32_t g0, uint32_t n,
                                        uint32_t A, uint32_t S, int lane) {
    const uint32_t to4 = (4u - (g0 & 3u)) & 3u, head = to4 < n ? to4 : n;
    const uint32_t nbody = (n - head) >> 2, tail = n - head - 4u * nbody;
    float* __restrict__ go = out + g0;
    f32x4* __restrict__ go4 = (f32x4*)(go + head);
    for (uint32_t k0 = 0; k0 < nbody; k0 += 64u * kPiecesPerLane) {
        f32x4 v[kPiecesPerLane];
#pragma unroll
        for (int u = 0; u < kPiecesPerLane; ++u) {
            const uint32_t p = k0 + 64u * u + lane;
            if (p < nbody) v[u] = go4[p];
        }
#pragma unroll
        for (int u = 0; u < kPiecesPerLane; ++u) {
            const uint32_t p = k0 + 64u * u + lane;
            if (p < nbody) {
                const uint32_t e = head + 4u * p;
                uint32_t r = e / A, cc = e - r * A;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[u][j] += lp[r * S + cc];
                    if (++cc == A) {
                        cc = 0u;
                        ++r;
                    }
                }
                go4[p] = v[u];
            }
        }
    }
    if ((uint32_t)lane < head) {
        const uint32_t r = (uint32_t)lane / A, cc = (uint32_t)lane - r * A;
        go[lane] += lp[r * S + cc];
    }
    if ((uint32_t)lane < tail) {
        const uint32_t e = head + 4u * nbody + lane, r = e / A, cc = e - r * A;
        go[e] += lp[r * S + cc];
    }
}

// ---------------------------------------------------------------- the grid (host)
// ct column tiles by `slices` time slices; slice s: the time steps [s * slice_len, min(T, (s + 1) *
// slice_len)). `who` opens the messages of a refused shape.
struct TilePlan {
    int ct, slices, slice_len;
};

inline int tile_plan(const std::string& who, int T, int B, int A, TilePlan* out) {
    FI_REQUIRE(T >= 1 && B >= 1, who + ": T = " + std::to_string(T) + ", B = " + std::to_string(B) + " must be >= 1");
    FI_REQUIRE(A >= 2 && A <= 64, who + ": A = " + std::to_string(A) + " outside 2 .. 64");
    FI_REQUIRE((uint64_t)T * (uint64_t)B * (uint64_t)A < (1ull << 31),
               who + ": T * B * A = " + std::to_string((uint64_t)T * (uint64_t)B * (uint64_t)A) + " passes 2^31 - 1");
    const int ct = (B + kCols - 1) / kCols;
    const int want = (kTargetWgs + ct - 1) / ct, most = (T + kWaves - 1) / kWaves;  // a slice holds a round at least
    const int s0 = want < most ? want : most;
    int len = (T + s0 - 1) / s0;
    len = (len + kWaves - 1) / kWaves * kWaves;
    *out = TilePlan{ct, (T + len - 1) / len, len};
    return FI_OK;
}

}  // namespace fi
