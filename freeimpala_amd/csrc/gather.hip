// gather.hip -- the ingest kernels of misc.hip with one level of indirection (gfx950): batch column
// b's entry is read at cols[b], a table of B base addresses in device memory, so the columns of one
// learner batch may come from several buffers (several recording actors, include/fi_gather.h) with
// their own strides, in any order. Outputs and their layouts are the contiguous ingest's:
//   frames (T+1, B, 84, 84, 4) u8 | obs (T+1, B, D) | mu (T, B, A) | act / rew / disc (T, B).
//   * fill_columns_kernel: the table from <= 64 segments {base, stride, first column, count} that
//     arrive by value as the kernel argument (no host buffer has to outlive an asynchronous step)
//   * gather_planes_kernel: ingest_planes_kernel with entry = cols[b]
//   * gather_vec_kernel / gather_scalar_kernel: mu, the MLP observation; action / reward /
//     discount, the out-of-range action count, and the min / max / sum of the records' flags words
//     (the parameter version the acting policy held) by integer atomics: exact in any order
// Record schemas: misc.hip.
#include <algorithm>

#include "fi_common.h"
#include "interleave.h"
#include "kernels.h"

namespace fi {

namespace {
constexpr int kFramePieces = 84 * 84 * 4 / 16;                // 1,764 16-byte pieces per frame
constexpr int PLANE_REC = FI_ATARI_PLANE_RECORD_BYTES;
constexpr int kPlaneBytes = 84 * 84;
constexpr int kPlanePieces = kPlaneBytes / 16;                // 441 16-byte pieces per plane
constexpr int kPlaneRuns = (kPlanePieces + 63) / 64;          // 7 runs of 64 pieces
constexpr int PLANE_REC_MU = kPlaneBytes, PLANE_HDR_ACT = 72;  // action at 7128
constexpr int PLANE_REC_START = 7144;
constexpr int kPlaneMaxActions = 18;
constexpr int REC_OBS = 0, REC_MU = 512, HDR_ACT = 256;       // the MLP record: action at 768
constexpr int HDR_FLAGS = 12;                                 // the flags word, from the action, in both schemas
static_assert(PLANE_REC_MU + PLANE_HDR_ACT + HDR_FLAGS + 4 == PLANE_REC_START, "plane header: flags, then episode_start");
static_assert(PLANE_REC == FI_ATARI_PLANE_RECORD_ELEMENTS * FI_RECORD_BYTES, "plane record size");
static_assert(3 * kPlaneBytes <= FI_ATARI_HISTORY_BYTES, "history block");
static_assert(REC_MU + HDR_ACT + HDR_FLAGS + 4 <= FI_RECORD_BYTES, "MLP record header");

// An entry is reached through a pointer loaded from the table, and a load through such a pointer
// would be a flat one (its address space is unknown to the compiler), counted on both wait counters.
// Entries are device memory that no kernel here writes: the loads name the global address space,
// and the one with a workgroup-uniform address the constant one, which selects a scalar load.
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

int grid_for(size_t n) {
    size_t g = (n + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
}  // namespace

// cols[c] = base_k + (c - first_k) * stride_k for the segment k that holds column c; thread 0 also
// puts the version block into its neutral state {min = ~0, max = 0, sum = 0}. The table is the
// kernel argument: the search reads it with scalar loads (k is uniform).
__global__ __launch_bounds__(256) void fill_columns_kernel(SegTable tab, const char** __restrict__ cols, int B,
                                                           uint32_t* __restrict__ versions) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0 && versions) {
        versions[0] = 0xffffffffu;
        versions[1] = versions[2] = versions[3] = 0u;
    }
    if (c >= B) return;
    for (int k = 0; k < tab.n; ++k) {
        const uint32_t i = (uint32_t)(c - tab.seg[k].first);
        if (i < (uint32_t)tab.seg[k].count) {
            cols[c] = tab.seg[k].base + (size_t)i * tab.seg[k].stride;
            return;
        }
    }
}

__global__ void gather_vec_kernel(const char* const* __restrict__ cols, int rows, int B, int W, int rec_off,
                                  size_t rec_stride, float* __restrict__ out) {
    const size_t n = (size_t)rows * B * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t lrow = i / W;
        const int d = (int)(i - lrow * W);
        const int t = (int)(lrow / B), b = (int)(lrow - (size_t)t * B);
        out[i] = ld4<float>(cols[b] + (size_t)t * rec_stride + rec_off + d * 4);
    }
}

// ingest_scalar_kernel through the table, plus the flags words: a lane folds its records' words
// into a min / max / sum, the wave reduces them by shuffles, and lane 0 issues three integer atomics
// per wave (versions: {min u32, max u32, sum u64}, in its neutral state before the launch).
__global__ __launch_bounds__(256) void gather_scalar_kernel(const char* const* __restrict__ cols, int T, int B, int A,
                                                            int mu_off, int hdr_act, size_t rec_stride, int32_t* act,
                                                            float* rew, float* disc, int* bad, uint32_t* versions) {
    const size_t n = (size_t)T * B;
    uint32_t vmin = 0xffffffffu, vmax = 0u;
    unsigned long long vsum = 0ull;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
        const char* r = cols[b] + (size_t)t * rec_stride + mu_off + hdr_act;
        int32_t a = ld4<int32_t>(r);
        if ((unsigned)a >= (unsigned)A && bad) atomicAdd(bad, 1);
        act[i] = a < 0 ? 0 : (a >= A ? A - 1 : a);
        rew[i] = ld4<float>(r + 4);
        disc[i] = ld4<float>(r + 8);
        const uint32_t v = ld4<uint32_t>(r + HDR_FLAGS);
        vmin = min(vmin, v);
        vmax = max(vmax, v);
        vsum += v;
    }
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

// ingest_planes_kernel (misc.hip) with entry = cols[b]. b comes from
// blockIdx, so the table load is one scalar load per workgroup and the entry base, like the
// episode_start test below, stays on the scalar unit.
__global__ __launch_bounds__(64) void gather_planes_kernel(const char* const* __restrict__ cols, int T, int B,
                                                           uint4* __restrict__ frames) {
    __shared__ uint4 turn[2][64];  // two buffers: one barrier per step
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / kPlaneRuns, run = blockIdx.x - b * kPlaneRuns;
    const int piece = run * 64 + lane;
    const bool live = piece < kPlanePieces;  // the loads of the last run's 7 spare lanes are skipped
    const char* __restrict__ entry = cols[b];
    const char* __restrict__ hist = entry + (size_t)(T + 1) * PLANE_REC;
    uint32_t w0[4] = {}, w1[4] = {}, w2[4] = {};  // this lane's dwords of the three previous steps
    uint4 next = make_uint4(0u, 0u, 0u, 0u);
    if (live) next = ld16(hist + piece * 16);
    for (int t = -3; t <= T; ++t) {
        const uint4 cur = next;
        if (t < T && live) {
            const char* src = t + 1 < 0 ? hist + (t + 4) * kPlaneBytes : entry + (size_t)(t + 1) * PLANE_REC;
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
            if (ld4_uniform(entry + (size_t)t * PLANE_REC + PLANE_REC_START) != 0u) {
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

int fill_columns_launch(const SegTable& tab, const void** cols, int B, uint32_t* versions, hipStream_t s) {
    FI_REQUIRE(cols && B >= 1, "fill_columns: bad arguments");
    FI_REQUIRE(tab.n >= 1 && tab.n <= FI_MAX_SEGMENTS, "fill_columns: 1 <= segments <= 64");
    int next = 0;
    for (int k = 0; k < tab.n; ++k) {
        FI_REQUIRE(tab.seg[k].base && tab.seg[k].count >= 1 && tab.seg[k].first == next,
                   "fill_columns: segment " + std::to_string(k) + " does not continue the columns at " +
                       std::to_string(next));
        next += tab.seg[k].count;
    }
    FI_REQUIRE(next == B, "fill_columns: the segments hold " + std::to_string(next) + " columns, the batch " +
                              std::to_string(B));
    hipLaunchKernelGGL(fill_columns_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, tab,
                       (const char**)cols, B, versions);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int gather_records_launch(const void* const* cols, int T, int B, int A, int D, float* obs, float* mu, int32_t* act,
                          float* rew, float* disc, hipStream_t s, int* bad, uint32_t* versions) {
    FI_REQUIRE(cols && T >= 1 && B >= 1 && A >= 1 && A <= 64 && D <= 128, "gather_records: bad shape");
    FI_REQUIRE(!versions || (uintptr_t)versions % 8 == 0, "gather_records: the version block must be 8-byte aligned");
    const char* const* c = (const char* const*)cols;
    const size_t stride = FI_RECORD_BYTES;
    if (obs) {
        FI_REQUIRE(D >= 1, "gather_records: D");
        hipLaunchKernelGGL(gather_vec_kernel, dim3(grid_for((size_t)(T + 1) * B * D)), dim3(256), 0, s, c, T + 1, B, D,
                           REC_OBS, stride, obs);
    }
    if (mu)
        hipLaunchKernelGGL(gather_vec_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s, c, T, B, A, REC_MU,
                           stride, mu);
    if (act && rew && disc)
        hipLaunchKernelGGL(gather_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, c, T, B, A, REC_MU,
                           HDR_ACT, stride, act, rew, disc, bad, versions);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int gather_atari_planes_launch(const void* const* cols, int T, int B, int A, uint8_t* frames, float* mu, int32_t* act,
                               float* rew, float* disc, hipStream_t s, int* bad, uint32_t* versions) {
    FI_REQUIRE(cols && frames && mu && act && rew && disc, "gather_atari_planes: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1, "gather_atari_planes: bad shape");
    FI_REQUIRE(A <= kPlaneMaxActions, "gather_atari_planes: the plane record's header holds mu[18]: A = " +
                                          std::to_string(A) + " > 18");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff / kPlaneRuns, "gather_atari_planes: too many frames");
    FI_REQUIRE((uintptr_t)cols % 8 == 0 && (uintptr_t)frames % 16 == 0,
               "gather_atari_planes: the column table must be 8-byte, frames 16-byte aligned");
    FI_REQUIRE(!versions || (uintptr_t)versions % 8 == 0, "gather_atari_planes: the version block must be 8-byte aligned");
    const char* const* c = (const char* const*)cols;
    const size_t stride = PLANE_REC;
    hipLaunchKernelGGL(gather_planes_kernel, dim3((unsigned)(B * kPlaneRuns)), dim3(64), 0, s, c, T, B, (uint4*)frames);
    hipLaunchKernelGGL(gather_vec_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s, c, T, B, A, PLANE_REC_MU,
                       stride, mu);
    hipLaunchKernelGGL(gather_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, c, T, B, A, PLANE_REC_MU,
                       PLANE_HDR_ACT, stride, act, rew, disc, bad, versions);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// the version block's neutral state, for the standalone entry points (the learner's
// fill_columns_kernel writes it in passing)
static int versions_reset(void* versions, hipStream_t s) {
    if (!versions) return FI_OK;
    FI_HIP_CHECK(hipMemsetAsync(versions, 0xff, 4, s));
    FI_HIP_CHECK(hipMemsetAsync((char*)versions + 4, 0, 12, s));
    return FI_OK;
}

// what a learner's step from segments enqueues as its ingest (learner.cpp: learner_step_segments)
static int learner_gather_ingest(const SegTable& tab, const GatherTargets& to) {
    FI_TRY(fill_columns_launch(tab, to.cols, to.B, to.versions, to.stream));
    if (to.arch == FI_ARCH_MLP)
        return gather_records_launch(to.cols, to.T, to.B, to.A, to.D, to.obs, to.mu, to.act, to.rew, to.disc, to.stream,
                                     to.bad, to.versions);
    return gather_atari_planes_launch(to.cols, to.T, to.B, to.A, to.frames, to.mu, to.act, to.rew, to.disc, to.stream,
                                      to.bad, to.versions);
}

}  // namespace fi

extern "C" int fi_learner_step_segments_dev(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs,
                                            fi_step_stats* out) {
    return fi::learner_step_segments(l, segs, n_segs, out, true, "step_segments_dev", fi::learner_gather_ingest);
}

extern "C" int fi_learner_step_segments_dev_async(fi_learner* l, const fi_entry_segment* segs, int32_t n_segs) {
    return fi::learner_step_segments(l, segs, n_segs, nullptr, false, "step_segments_dev_async",
                                     fi::learner_gather_ingest);
}

extern "C" int fi_ingest_atari_planes_gather(const void* const* cols_dev, int T, int B, int A, uint8_t* frames,
                                             float* mu, int32_t* actions, float* rewards, float* discounts,
                                             int* bad_dev, void* versions_dev, void* stream) {
    FI_TRY(fi::versions_reset(versions_dev, (hipStream_t)stream));
    return fi::gather_atari_planes_launch(cols_dev, T, B, A, frames, mu, actions, rewards, discounts,
                                          (hipStream_t)stream, bad_dev, (uint32_t*)versions_dev);
}

extern "C" int fi_ingest_records_gather(const void* const* cols_dev, int T, int B, int A, int D, float* obs, float* mu,
                                        int32_t* actions, float* rewards, float* discounts, int* bad_dev,
                                        void* versions_dev, void* stream) {
    FI_TRY(fi::versions_reset(versions_dev, (hipStream_t)stream));
    return fi::gather_records_launch(cols_dev, T, B, A, D, obs, mu, actions, rewards, discounts, (hipStream_t)stream,
                                     bad_dev, (uint32_t*)versions_dev);
}
