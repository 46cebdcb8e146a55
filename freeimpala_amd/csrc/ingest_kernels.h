// ingest_kernels.h -- the ingest kernels, once (gfx950): entries of records (records.h) -> the
// time-major SoA tensors
//   frames (T+1, B, 84, 84, 4) u8 | obs (T+1, B, D) | mu (T, B, A) | act / rew / disc (T, B).
// They are templates on where batch column b's entry lies: misc.hip instantiates them with Strided
// (one buffer, entries entry_bytes apart), gather.hip with Table (a table of B base addresses in
// device memory, so the columns of a batch may come from several buffers, in any order). A header
// and no object: a library of misc.hip without gather.hip still links.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "records.h"

namespace fi {

// ---------------------------------------------------------------- where column b's entry lies
// trivially copyable kernel arguments
struct Strided {
    const char* rec;
    size_t entry_bytes;
    __device__ __forceinline__ const char* operator()(int b) const { return rec + (size_t)b * entry_bytes; }
};
struct Table {
    const char* const* cols;
    __device__ __forceinline__ const char* operator()(int b) const { return cols[b]; }
};

// An entry may be reached through a pointer loaded from the table, and a load through such a
// pointer would be a flat one (its address space is unknown to the compiler), counted on both wait
// counters. Entries are device memory that no kernel here writes: the loads name the global address
// space, and the one with a workgroup-uniform address the constant one, which selects a scalar load.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(const char* p) {
    const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <typename T>
__device__ __forceinline__ T ld4(const char* p) {
    return *(const __attribute__((address_space(1))) T*)p;
}
__device__ __forceinline__ uint32_t ld4_uniform(const char* p) {
    return *(const __attribute__((address_space(4))) uint32_t*)p;
}

// 256-lane workgroups of a grid-stride kernel over n elements
inline int grid_for(size_t n) {
    size_t g = (n + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// ---------------------------------------------------------------- vectors: mu, the MLP observation
// out (rows, B, W) <- W floats at rec_off of record t of column b's entry
template <typename Where>
__global__ void ingest_vec_kernel(Where where, int rows, int B, int W, int rec_off, size_t rec_stride,
                                  float* __restrict__ out) {
    const size_t n = (size_t)rows * B * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t lrow = i / W;
        const int d = (int)(i - lrow * W);
        const int t = (int)(lrow / B), b = (int)(lrow - (size_t)t * B);
        out[i] = ld4<float>(where(b) + (size_t)t * rec_stride + rec_off + d * 4);
    }
}

// ---------------------------------------------------------------- action / reward / discount
// Actions outside [0, A) are counted into *bad (nullable) and stored clamped. kVersions: a lane
// also folds its records' flags words (the parameter version the acting policy held) into a min /
// max / sum, the wave reduces them by shuffles, and lane 0 issues three integer atomics per wave --
// exact in any order (versions: {min u32, max u32, sum u64}, in its neutral state before the
// launch; nullable). Without kVersions the flags word is not loaded.
template <typename Where, bool kVersions>
__global__ __launch_bounds__(256) void ingest_scalar_kernel(Where where, int T, int B, int A, int act_off,
                                                            size_t rec_stride, int32_t* act, float* rew, float* disc,
                                                            int* bad, uint32_t* versions) {
    const size_t n = (size_t)T * B;
    uint32_t vmin = 0xffffffffu, vmax = 0u;
    unsigned long long vsum = 0ull;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
        const char* r = where(b) + (size_t)t * rec_stride + act_off;
        // the header's loads before the first store: the outputs are not known to lie apart from the entries
        const int32_t a = ld4<int32_t>(r);
        const float reward = ld4<float>(r + kHdrReward), discount = ld4<float>(r + kHdrDiscount);
        const uint32_t v = kVersions ? ld4<uint32_t>(r + kHdrFlags) : 0u;
        if ((unsigned)a >= (unsigned)A && bad) atomicAdd(bad, 1);
        act[i] = a < 0 ? 0 : (a >= A ? A - 1 : a);
        rew[i] = reward;
        disc[i] = discount;
        if constexpr (kVersions) {
            vmin = min(vmin, v);
            vmax = max(vmax, v);
            vsum += v;
        }
    }
    if constexpr (kVersions) {
        if (!versions) return;  // uniform: a kernel argument
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            vmin = min(vmin, (uint32_t)__shfl_xor((int)vmin, off, 64));
            vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, off, 64));
            vsum += __shfl_xor(vsum, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(versions, vmin);
            atomicMax(versions + 1, vmax);
            atomicAdd((unsigned long long*)(versions + 2), vsum);
        }
    }
}

// ---------------------------------------------------------------- plane records -> frames
// 4 pixels of channels 0..3 (one dword each) -> 4 NHWC pixels (byte c of a pixel = channel c)
__device__ __forceinline__ uint4 interleave4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    const uint32_t ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);
    const uint32_t cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
    return make_uint4(__builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u),   // a0 b0 c0 d0
                      __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u),   // a1 b1 c1 d1
                      __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u),
                      __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u));
}

// Plane records -> the frames tensor: channel c of frame t is the plane of step t-3+c, the first
// observation of an episode filling all four channels (the frame-stack wrapper's rule, DESIGN.md
// section 3). A byte interleave of four planes into 4-byte pixels that reads every plane from HBM
// once.
//   A one-wave workgroup owns an entry b and a run of 64 16-byte plane pieces (1,024 pixels) and
// walks t forward: -3..-1 take the history block's planes, 0..T the records'. Each step a lane
// loads its 16-byte piece (the next step's is requested before this step's stores), the wave
// turns the 256 dwords through LDS so that lane j holds dwords 64k + j (k = 0..3), and the lane
// keeps the three previous steps' four dwords in registers. Output piece 64k + j of the run is
// then the byte interleave of dword 64k + j of the four channels (two levels of v_perm_b32), so
// each of the four 16-byte stores of a step is contiguous over the wave (1 KiB). b comes from
// blockIdx, so the entry base (with Table: one scalar load per workgroup) stays on the scalar
// unit; episode_start is uniform per (t, b): one scalar load and a uniform branch. 7 runs cover
// the 441 pieces (the last has 57); 7 B workgroups, no grid cap.
template <typename Where>
__global__ __launch_bounds__(64) void ingest_planes_kernel(Where where, int T, int B, uint4* __restrict__ frames) {
    __shared__ uint4 turn[2][64];  // two buffers: one barrier per step
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / kPlaneRuns, run = blockIdx.x - b * kPlaneRuns;
    const int piece = run * 64 + lane;
    const bool live = piece < kPlanePieces;  // the loads of the last run's 7 spare lanes are skipped
    const char* __restrict__ entry = where(b);
    const char* __restrict__ hist = entry + plane_history_offset(T);
    uint32_t w0[4] = {}, w1[4] = {}, w2[4] = {};  // this lane's dwords of the three previous steps
    uint4 next = make_uint4(0u, 0u, 0u, 0u);
    if (live) next = ld16(hist + piece * 16);
    for (int t = -kHistoryPlanes; t <= T; ++t) {
        const uint4 cur = next;
        if (t < T && live) {
            const char* src = t + 1 < 0 ? hist + (t + 1 + kHistoryPlanes) * kPlaneBytes
                                        : entry + (size_t)(t + 1) * kPlaneRecBytes;
            next = ld16(src + piece * 16);
        }
        uint4* x = turn[t & 1];
        x[lane] = cur;
        __syncthreads();
        const uint32_t* xd = (const uint32_t*)x;
        uint32_t n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] = xd[64 * k + lane];
        if (t >= 0) {
            if (ld4_uniform(entry + (size_t)t * kPlaneRecBytes + kPlaneRecStart) != 0u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) w0[k] = w1[k] = w2[k] = n[k];
            }
            uint4* __restrict__ dst = frames + ((size_t)t * B + b) * kFramePieces + run * 256 + lane;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (run * 256 + 64 * k + lane < kFramePieces) dst[64 * k] = interleave4(w0[k], w1[k], w2[k], n[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w0[k] = w1[k];
            w1[k] = w2[k];
            w2[k] = n[k];
        }
    }
}

// what the launchers of both files enqueue behind their own argument checks
template <typename Where>
inline void launch_ingest_vec(Where where, int rows, int B, int W, int rec_off, size_t rec_stride, float* out,
                              hipStream_t s) {
    hipLaunchKernelGGL(ingest_vec_kernel<Where>, dim3(grid_for((size_t)rows * B * W)), dim3(256), 0, s, where,
                       rows, B, W, rec_off, rec_stride, out);
}
template <typename Where, bool kVersions>
inline void launch_ingest_scalar(Where where, int T, int B, int A, int act_off, size_t rec_stride, int32_t* act,
                                 float* rew, float* disc, int* bad, uint32_t* versions, hipStream_t s) {
    hipLaunchKernelGGL((ingest_scalar_kernel<Where, kVersions>), dim3(grid_for((size_t)T * B)), dim3(256), 0,
                       s, where, T, B, A, act_off, rec_stride, act, rew, disc, bad, versions);
}
template <typename Where>
inline void launch_ingest_planes(Where where, int T, int B, uint8_t* frames, hipStream_t s) {
    hipLaunchKernelGGL(ingest_planes_kernel<Where>, dim3((unsigned)(B * kPlaneRuns)), dim3(64), 0, s, where, T, B,
                       (uint4*)frames);
}

}  // namespace fi
