// rollout.hip -- the kernels that record an actor's steps as the learner's host entries, in device
// memory (include/fi_rollout.h): the plane record of one step, the history block out of the
// stacks, the MLP record, and the scatter of the rewards and discounts that arrive from the host.
// They follow push_planes_kernel (actor.hip): one-wave workgroups, 16-byte accesses contiguous
// over the wave, a tail run of 57 pieces. Every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include <string>

#include "fi_common.h"
#include "fi_rollout.h"
#include "kernels.h"
#include "records.h"

namespace fi {

namespace {
constexpr int kStackPieces = kFramePieces;  // an actor's stack is one frame: 1,764 16-byte pieces
constexpr int kRec = kPlaneRecBytes;
// dword indices of the plane record's header fields, from its mu (records.h; the reward and the
// discount between the action and the flags are the outcome scatter's)
constexpr int kDwMu = 0, kDwAct = (kPlaneRecAct - kPlaneRecMu) / 4, kDwFlags = (kPlaneRecFlags - kPlaneRecMu) / 4,
              kDwStart = (kPlaneRecStart - kPlaneRecMu) / 4;
static_assert(kDwAct == kPlaneMaxActions && kDwStart < 64, "the header's dwords: one per lane of the last run's wave");
}  // namespace

// ---------------------------------------------------------------- one step's plane record
// rec = entries + t * 7168; entry i lies i * stride bytes further. A workgroup owns an environment
// and a run of 64 16-byte plane pieces (the last run: 57). The last run's workgroup also writes the
// header, one dword per lane: mu[lane] for lane < A, the action, the flags word, episode_start
// (read as push_planes_kernel reads it: the aligned dword that holds the byte). Without logits
// only the plane and episode_start are written (record T of an unroll). 7 N workgroups; HBM
// traffic 2 * 7,056 N bytes and the header's.
__global__ __launch_bounds__(64) void record_planes_kernel(char* __restrict__ rec, size_t stride,
                                                           const uint4* __restrict__ planes,
                                                           const uint8_t* __restrict__ start,
                                                           const float* __restrict__ logits,
                                                           const int32_t* __restrict__ actions, uint32_t flags,
                                                           int A) {
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x / kPlaneRuns, run = blockIdx.x - env * kPlaneRuns;
    const int piece = run * 64 + lane;
    char* __restrict__ r = rec + (size_t)env * stride;
    if (piece < kPlanePieces) ((uint4*)r)[piece] = planes[(size_t)env * kPlanePieces + piece];
    if (run != kPlaneRuns - 1) return;
    uint32_t* __restrict__ hdr = (uint32_t*)(r + kPlaneBytes);
    const uint8_t* __restrict__ fp = start + env;
    const uint32_t fsh = (uint32_t)((uintptr_t)fp & 3u);
    const uint32_t fword = *(const uint32_t*)(fp - fsh);
    const uint32_t first = ((fword >> (8u * fsh)) & 0xffu) != 0u ? 1u : 0u;
    if (lane == kDwStart) hdr[kDwStart] = first;
    if (!logits) return;
    if (lane < A) hdr[kDwMu + lane] = __float_as_uint(logits[(size_t)env * A + lane]);
    if (lane == kDwAct) hdr[kDwAct] = (uint32_t)actions[env];
    if (lane == kDwFlags) hdr[kDwFlags] = flags;
}

int record_planes_launch(void* entries, size_t stride, int t, const uint8_t* planes, const uint8_t* start,
                         const float* logits, const int32_t* actions, uint32_t flags, int N, int A, hipStream_t s) {
    FI_REQUIRE(entries && planes && start, "record_plane_step: null argument");
    FI_REQUIRE(!logits || actions, "record_plane_step: logits without actions");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlaneRuns, "record_plane_step: N must be >= 1");
    FI_REQUIRE(A >= 2 && A <= kPlaneMaxActions, "record_plane_step: the plane record's header holds mu[18]: 2 <= A <= 18");
    FI_REQUIRE(t >= 0, "record_plane_step: t must be >= 0");
    FI_REQUIRE((uintptr_t)entries % 16 == 0 && stride % 16 == 0 && (uintptr_t)planes % 16 == 0,
               "record_plane_step: entries, entry_stride and planes must be 16-byte aligned");
    FI_REQUIRE(stride >= ((size_t)t + 1) * kRec, "record_plane_step: entry_stride " + std::to_string(stride) +
                                                     " < (t+1)*7168 = " + std::to_string(((size_t)t + 1) * kRec));
    hipLaunchKernelGGL(record_planes_kernel, dim3((unsigned)(N * kPlaneRuns)), dim3(64), 0, s,
                       (char*)entries + (size_t)t * kRec, stride, (const uint4*)planes, start, logits, actions, flags, A);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- history block
// The inverse of the push's interleave. A workgroup owns an environment and a run of 256 stack
// pieces = 64 plane pieces per channel. Lane j loads stack pieces 64k + j (k = 0..3, each load
// contiguous over the wave); a piece is four pixels of four channel bytes, and two v_perm_b32
// pairs gather channel c of its pixels into plane dword 64k + j. The wave turns the 256 dwords of a
// channel through LDS so that lane j holds plane piece j, and stores it contiguously. Channels 0,
// 1, 2 go to hist + c * 7056; channel 3 (the newest plane) is the record's own. 7 N workgroups;
// HBM traffic (28,224 + 21,168) N bytes, on a carry-over call only.
template <int C>
__device__ __forceinline__ uint32_t gather_channel(const uint4& w) {
    constexpr uint32_t pick = ((uint32_t)(4 + C) << 8) | (uint32_t)C;  // byte C of the low word, then of the high
    const uint32_t lo = __builtin_amdgcn_perm(w.y, w.x, pick);
    const uint32_t hi = __builtin_amdgcn_perm(w.w, w.z, pick);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

__global__ __launch_bounds__(64) void extract_history_kernel(char* __restrict__ hist, size_t stride,
                                                             const uint4* __restrict__ stacks) {
    __shared__ uint4 turn[3][64];
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x / kPlaneRuns, run = blockIdx.x - env * kPlaneRuns;
    const uint4* __restrict__ st = stacks + (size_t)env * kStackPieces + run * 256 + lane;
    const int left = kStackPieces - run * 256 - lane;  // stack pieces from this lane's first to the end
    uint4 w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = make_uint4(0u, 0u, 0u, 0u);
        if (64 * k < left) w[k] = st[64 * k];
    }
    uint32_t* xd = (uint32_t*)turn;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xd[0 * 256 + 64 * k + lane] = gather_channel<0>(w[k]);
        xd[1 * 256 + 64 * k + lane] = gather_channel<1>(w[k]);
        xd[2 * 256 + 64 * k + lane] = gather_channel<2>(w[k]);
    }
    __syncthreads();
    const int piece = run * 64 + lane;
    if (piece >= kPlanePieces) return;
    char* __restrict__ h = hist + (size_t)env * stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) ((uint4*)(h + (size_t)c * kPlaneBytes))[piece] = turn[c][lane];
}

int extract_history_launch(void* entries, size_t stride, size_t hist_off, const uint8_t* stacks, int N, hipStream_t s) {
    FI_REQUIRE(entries && stacks, "extract_history: null argument");
    FI_REQUIRE(N >= 1 && N <= 0x7fffffff / kPlaneRuns, "extract_history: N must be >= 1");
    FI_REQUIRE((uintptr_t)entries % 16 == 0 && stride % 16 == 0 && hist_off % 16 == 0 && (uintptr_t)stacks % 16 == 0,
               "extract_history: entries, entry_stride, history_offset and stacks must be 16-byte aligned");
    FI_REQUIRE(stride >= hist_off + kHistoryPlanes * (size_t)kPlaneBytes,
               "extract_history: entry_stride " + std::to_string(stride) + " < history_offset + 21168 = " +
                   std::to_string(hist_off + kHistoryPlanes * (size_t)kPlaneBytes));
    hipLaunchKernelGGL(extract_history_kernel, dim3((unsigned)(N * kPlaneRuns)), dim3(64), 0, s,
                       (char*)entries + hist_off, stride, (const uint4*)stacks);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- one step's MLP record
// rec = entries + t * 1024. One wave per environment, one dword per lane and store: the D <= 128
// observation floats at byte 0, with logits also mu[lane] at 512, the action at 768 and the flags
// word at 780 (record schema: records.h). The observation rows are D floats apart, so
// for a D that is no multiple of 4 they are not 16-byte aligned: dword accesses, contiguous over
// the wave.
__global__ __launch_bounds__(64) void record_obs_kernel(char* __restrict__ rec, size_t stride,
                                                        const float* __restrict__ obs, int D,
                                                        const float* __restrict__ logits,
                                                        const int32_t* __restrict__ actions, uint32_t flags, int A) {
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x;
    uint32_t* __restrict__ r = (uint32_t*)(rec + (size_t)env * stride);
    const uint32_t* __restrict__ o = (const uint32_t*)(obs + (size_t)env * D);
    for (int i = lane; i < D; i += 64) r[i] = o[i];
    if (!logits) return;
    if (lane < A) r[kMlpRecMu / 4 + lane] = __float_as_uint(logits[(size_t)env * A + lane]);
    if (lane == 0) r[kMlpRecAct / 4] = (uint32_t)actions[env];
    if (lane == 1) r[kMlpRecFlags / 4] = flags;
}

int record_obs_launch(void* entries, size_t stride, int t, const float* obs, int D, const float* logits,
                      const int32_t* actions, uint32_t flags, int N, int A, hipStream_t s) {
    FI_REQUIRE(entries && obs, "record_obs: null argument");
    FI_REQUIRE(!logits || actions, "record_obs: logits without actions");
    FI_REQUIRE(N >= 1 && D >= 1 && D <= kMlpMaxObs && A >= 2 && A <= kMlpMaxActions && t >= 0, "record_obs: bad shape");
    FI_REQUIRE((uintptr_t)entries % 4 == 0 && stride % 4 == 0, "record_obs: entries and entry_stride must be 4-byte aligned");
    FI_REQUIRE(stride >= ((size_t)t + 1) * kMlpRecBytes, "record_obs: entry_stride < (t+1)*1024");
    hipLaunchKernelGGL(record_obs_kernel, dim3((unsigned)N), dim3(64), 0, s, (char*)entries + (size_t)t * kMlpRecBytes,
                       stride, obs, D, logits, actions, flags, A);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- rewards and discounts
// N rows of two floats, from the rewards (N) and the discounts (N): the host's staging block holds
// one behind the other, a device environment (fi_env.h) two arrays of its own; field = the byte
// offset of the reward in the record (the discount follows it).
__global__ __launch_bounds__(256) void scatter_outcome_kernel(char* __restrict__ rec, size_t stride,
                                                              const float* __restrict__ rewards,
                                                              const float* __restrict__ discounts, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float* __restrict__ f = (float*)(rec + (size_t)i * stride);
    f[0] = rewards[i];
    f[1] = discounts[i];
}

int scatter_outcome_launch(void* entries, size_t stride, size_t field, const float* rewards, const float* discounts,
                           int N, hipStream_t s) {
    FI_REQUIRE(entries && rewards && discounts && N >= 1, "rollout_outcome: bad arguments");
    FI_REQUIRE(((uintptr_t)entries + field) % 4 == 0 && stride % 4 == 0 && stride >= field + 8,
               "rollout_outcome: misaligned record");
    hipLaunchKernelGGL(scatter_outcome_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s,
                       (char*)entries + field, stride, rewards, discounts, N);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int scatter_outcome_launch(void* entries, size_t stride, size_t field, const float* out, int N, hipStream_t s) {
    FI_REQUIRE(out && N >= 1, "rollout_outcome: bad arguments");
    return scatter_outcome_launch(entries, stride, field, out, out + N, N, s);
}

}  // namespace fi

extern "C" int fi_record_plane_step(void* entries_dev, size_t entry_stride, int32_t t, const uint8_t* planes_dev,
                                    const uint8_t* episode_start_dev, const float* logits_dev,
                                    const int32_t* actions_dev, uint32_t flags, int N, int A, void* stream) {
    return fi::record_planes_launch(entries_dev, entry_stride, t, planes_dev, episode_start_dev, logits_dev,
                                    actions_dev, flags, N, A, (hipStream_t)stream);
}

extern "C" int fi_extract_history(void* entries_dev, size_t entry_stride, size_t history_offset,
                                  const uint8_t* stacks_dev, int N, void* stream) {
    return fi::extract_history_launch(entries_dev, entry_stride, history_offset, stacks_dev, N, (hipStream_t)stream);
}
