// misc.hip -- HBM-bound helper kernels of the learner step (gfx950):
//   * synthetic trajectories (Philox4x32-10, bit-identical to the oracle's generator)
//   * ingest: (B, S*1024) SharedBuffer entries -> time-major SoA tensors (MLP records, the
//     Atari records with their 84x84x4 frames, and the single-plane Atari records whose
//     4-frame stack is rebuilt here)
//   * column sums / split-K slab reduction (deterministic, fixed order)
//   * global gradient norm, Adam / SGD with global-norm clipping, fp32 -> bf16
#include <algorithm>

#include "fi_common.h"
#include "interleave.h"
#include "kernels.h"

namespace fi {

// philox4 and the stream ids (ST_*): fi_common.h, shared with actor.hip's sampler
__device__ __forceinline__ float approx_normal(uint4 u) {
    const uint32_t s = (u.x >> 8) + (u.y >> 8) + (u.z >> 8) + (u.w >> 8);
    const float x = (float)((int32_t)s - (int32_t)(1u << 25));
    return x * 0x1.bb67aep-24f;
}

__global__ void synth_normal_kernel(uint64_t seed, uint32_t stream, int rows, int B, int B_glob,
                                    int b_off, int D, float* out) {
    const size_t n = (size_t)rows * B * D;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t lrow = i / D;
        const int d = (int)(i - lrow * D);
        const int t = (int)(lrow / B), b = (int)(lrow - (size_t)t * B);
        const uint64_t row = (uint64_t)t * B_glob + (uint64_t)(b_off + b);
        out[i] = approx_normal(philox4(seed, row * D + d, stream));
    }
}

__global__ void synth_scalar_kernel(uint64_t seed, int T, int B, int B_glob, int b_off, int A,
                                    float gamma, int32_t* act, float* rew, float* disc) {
    const size_t n = (size_t)T * B;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
        const uint64_t row = (uint64_t)t * B_glob + (uint64_t)(b_off + b);
        if (act) {
            const uint4 u = philox4(seed, row, ST_ACT);
            act[i] = (int32_t)(((uint64_t)(u.x >> 8) * (uint32_t)A) >> 24);
        }
        if (rew) {
            const uint4 u = philox4(seed, row, ST_REW);
            rew[i] = (float)((int32_t)(u.x % 3u) - 1);
        }
        if (disc) {
            const uint4 u = philox4(seed, row, ST_DONE);
            disc[i] = ((u.x >> 8) < 167772u) ? 0.0f : gamma;
        }
    }
}

__global__ void synth_frames_kernel(uint64_t seed, int rows, int B, int B_glob, int b_off,
                                    uint4* frames) {
    constexpr int Q = 84 * 84 * 4 / 16;  // 16-byte pieces per frame
    const size_t n = (size_t)rows * B * Q;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t lrow = i / Q;
        const int qd = (int)(i - lrow * Q);
        const int t = (int)(lrow / B), b = (int)(lrow - (size_t)t * B);
        const uint64_t row = (uint64_t)t * B_glob + (uint64_t)(b_off + b);
        frames[i] = philox4(seed, row * Q + qd, ST_FRAME);
    }
}

static int grid_for(size_t n) {
    size_t g = (n + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

int synth_launch(uint64_t seed, int T, int B, int B_glob, int b_off, int A, int D, float gamma,
                 float* obs, float* mu, int32_t* act, float* rew, float* disc, uint8_t* frames,
                 hipStream_t s) {
    FI_REQUIRE(T >= 1 && B >= 1 && B_glob >= b_off + B && A >= 1, "synth: bad shape");
    if (obs) {
        FI_REQUIRE(D >= 1, "synth: D");
        hipLaunchKernelGGL(synth_normal_kernel, dim3(grid_for((size_t)(T + 1) * B * D)), dim3(256), 0,
                           s, seed, (uint32_t)ST_OBS, T + 1, B, B_glob, b_off, D, obs);
    }
    if (mu)
        hipLaunchKernelGGL(synth_normal_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s,
                           seed, (uint32_t)ST_MU, T, B, B_glob, b_off, A, mu);
    if (act || rew || disc)
        hipLaunchKernelGGL(synth_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, seed,
                           T, B, B_glob, b_off, A, gamma, act, rew, disc);
    if (frames)
        hipLaunchKernelGGL(synth_frames_kernel, dim3(grid_for((size_t)(T + 1) * B * 1764)), dim3(256),
                           0, s, seed, T + 1, B, B_glob, b_off, (uint4*)frames);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- ingest
// MLP record schema (one 1 KiB ELEMENT per step, reference data_structures.h:35, agent.h:62):
//   [0,512) float obs[<=128] | [512,768) float mu_logits[<=64] | 768 int32 action |
//   772 float reward | 776 float discount | 780 uint32 flags | 784.. reserved.
// Atari record schema (28 ELEMENTs = 28,672 B per step, FI_ATARI_RECORD_BYTES):
//   [0,28224) u8 frame 84x84x4 NHWC | [28224,28480) float mu_logits[<=64] | 28480 int32 action |
//   28484 float reward | 28488 float discount | 28492 uint32 flags | 28496.. reserved.
// Both headers have the same shape: mu, then action / reward / discount at +256 / +260 / +264.
// An entry holds T+1 records (record T = bootstrap observation; its header is ignored).
// Atari plane record schema (7 ELEMENTs = 7,168 B per step, FI_ATARI_PLANE_RECORD_BYTES):
//   [0,7056) u8 plane 84x84 (the newest observation) | [7056,7128) float mu_logits[<=18] |
//   7128 int32 action | 7132 float reward | 7136 float discount | 7140 uint32 flags |
//   7144 uint32 episode_start | 7148.. reserved.
// Its entry holds T+1 records and then, at (T+1)*7168, the three planes that precede record 0 in
// the actor's stack (oldest first, 3*7056 B, padded to FI_ATARI_HISTORY_BYTES).
constexpr int REC_OBS = 0, REC_MU = 512;
constexpr int HDR_ACT = 256;  // relative to the record's mu; reward and discount follow the action
constexpr int kFrameBytes = 84 * 84 * 4;
constexpr int kFramePieces = kFrameBytes / 16;  // 1,764 16-byte pieces
constexpr int ATARI_REC_MU = kFrameBytes;
static_assert(ATARI_REC_MU + HDR_ACT + 16 <= FI_ATARI_RECORD_BYTES, "Atari record header");
static_assert(FI_ATARI_RECORD_BYTES == FI_ATARI_RECORD_ELEMENTS * FI_RECORD_BYTES, "Atari record size");

__global__ void ingest_vec_kernel(const char* __restrict__ rec, int rows, int B, int W,
                                  int rec_off, size_t rec_stride, size_t entry_bytes,
                                  float* __restrict__ out) {
    const size_t n = (size_t)rows * B * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t lrow = i / W;
        const int d = (int)(i - lrow * W);
        const int t = (int)(lrow / B), b = (int)(lrow - (size_t)t * B);
        out[i] = *(const float*)(rec + (size_t)b * entry_bytes + (size_t)t * rec_stride +
                                 rec_off + d * 4);
    }
}

__global__ void ingest_scalar_kernel(const char* __restrict__ rec, int T, int B, int A,
                                     int mu_off, int hdr_act, size_t rec_stride, size_t entry_bytes,
                                     int32_t* act, float* rew, float* disc, int* bad) {
    const size_t n = (size_t)T * B;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
        const char* r = rec + (size_t)b * entry_bytes + (size_t)t * rec_stride + mu_off;
        r += hdr_act;
        int32_t a = *(const int32_t*)r;
        if ((unsigned)a >= (unsigned)A && bad) atomicAdd(bad, 1);
        act[i] = a < 0 ? 0 : (a >= A ? A - 1 : a);
        rew[i] = *(const float*)(r + 4);
        disc[i] = *(const float*)(r + 8);
    }
}

// Frames of the Atari records -> the time-major frames tensor (T+1, B, 84, 84, 4): a strided
// de-interleave of whole 28,224-byte frames. A workgroup owns a frame and grid-strides over
// frames, so the (t, b) index work is done once per frame on the scalar unit; its 256 lanes
// move the frame's 1,764 16-byte pieces, 7 per lane, every load issued before the first store.
constexpr int kIngestFullRounds = kFramePieces / 256;                  // 6 rounds of all 256 lanes
constexpr int kIngestTailLanes = kFramePieces - 256 * kIngestFullRounds;  // + 228 lanes once more

__global__ __launch_bounds__(256) void ingest_frames_kernel(const char* __restrict__ rec, int n_frames,
                                                            int B, size_t entry_bytes,
                                                            uint4* __restrict__ frames) {
    const int lane = threadIdx.x & 255;  // the launch uses 256 lanes: every piece index below is in range
    const bool tail = lane < kIngestTailLanes;
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const int t = f / B, b = f - t * B;
        const uint4* __restrict__ src =
            (const uint4*)(rec + (size_t)b * entry_bytes + (size_t)t * FI_ATARI_RECORD_BYTES) + lane;
        uint4* __restrict__ dst = frames + (size_t)f * kFramePieces + lane;
        uint4 v[kIngestFullRounds];
        uint4 vt = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < kIngestFullRounds; ++k) v[k] = src[k * 256];
        if (tail) vt = src[kIngestFullRounds * 256];
#pragma unroll
        for (int k = 0; k < kIngestFullRounds; ++k) dst[k * 256] = v[k];
        if (tail) dst[kIngestFullRounds * 256] = vt;
    }
}

int ingest_launch(const void* rec, int T, int B, int A, int D, size_t entry_bytes, float* obs,
                  float* mu, int32_t* act, float* rew, float* disc, hipStream_t s, int* bad) {
    FI_REQUIRE(rec && T >= 1 && B >= 1 && A >= 1 && A <= 64 && D <= 128, "ingest: bad shape");
    FI_REQUIRE(entry_bytes >= (size_t)(T + 1) * FI_RECORD_BYTES, "ingest: entry too small");
    const char* r = (const char*)rec;
    const size_t stride = FI_RECORD_BYTES;
    if (obs)
        hipLaunchKernelGGL(ingest_vec_kernel, dim3(grid_for((size_t)(T + 1) * B * D)), dim3(256), 0, s,
                           r, T + 1, B, D, REC_OBS, stride, entry_bytes, obs);
    if (mu)
        hipLaunchKernelGGL(ingest_vec_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s, r, T,
                           B, A, REC_MU, stride, entry_bytes, mu);
    if (act && rew && disc)
        hipLaunchKernelGGL(ingest_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, r, T,
                           B, A, REC_MU, HDR_ACT, stride, entry_bytes, act, rew, disc, bad);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// workgroups of the frame copy: 8 per CU on 256 CUs, the rest of the frames by grid stride
constexpr int kIngestFramesMaxGrid = 2048;

int ingest_atari_launch(const void* rec, int T, int B, int A, size_t entry_bytes, uint8_t* frames,
                        float* mu, int32_t* act, float* rew, float* disc, hipStream_t s, int* bad) {
    FI_REQUIRE(rec && frames && mu && act && rew && disc, "ingest_atari: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1 && A <= 64, "ingest_atari: bad shape");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff, "ingest_atari: too many frames");
    FI_REQUIRE(entry_bytes % 16 == 0, "ingest_atari: entry_bytes must be a multiple of 16");
    FI_REQUIRE(entry_bytes >= (size_t)(T + 1) * FI_ATARI_RECORD_BYTES,
               "ingest_atari: entry_bytes < " + std::to_string((size_t)(T + 1) * FI_ATARI_RECORD_BYTES) +
                   " = (T+1)*28672");
    FI_REQUIRE((uintptr_t)rec % 16 == 0 && (uintptr_t)frames % 16 == 0,
               "ingest_atari: records and frames must be 16-byte aligned");
    const char* r = (const char*)rec;
    const size_t stride = FI_ATARI_RECORD_BYTES;
    const int n_frames = (T + 1) * B;
    hipLaunchKernelGGL(ingest_frames_kernel, dim3(std::min(n_frames, kIngestFramesMaxGrid)), dim3(256), 0, s,
                       r, n_frames, B, entry_bytes, (uint4*)frames);
    hipLaunchKernelGGL(ingest_vec_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s, r, T, B, A,
                       ATARI_REC_MU, stride, entry_bytes, mu);
    hipLaunchKernelGGL(ingest_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, r, T, B, A,
                       ATARI_REC_MU, HDR_ACT, stride, entry_bytes, act, rew, disc, bad);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// Plane records -> the same frames tensor: channel c of frame t is the plane of step t-3+c, the
// first observation of an episode filling all four channels (the frame-stack wrapper's rule,
// DESIGN.md section 3). A byte interleave of four planes into 4-byte pixels that reads every
// plane from HBM once.
//   A one-wave workgroup owns an entry b and a run of 64 16-byte plane pieces (1,024 pixels) and
// walks t forward: -3..-1 take the history block's planes, 0..T the records'. Each step a lane
// loads its 16-byte piece (the next step's is requested before this step's stores), the wave
// turns the 256 dwords through LDS so that lane j holds dwords 64k + j (k = 0..3), and the lane
// keeps the three previous steps' four dwords in registers. Output piece 64k + j of the run is
// then the byte interleave of dword 64k + j of the four channels (two levels of v_perm_b32), so
// each of the four 16-byte stores of a step is contiguous over the wave (1 KiB). episode_start
// is uniform per (t, b): one scalar load and a uniform branch. 7 runs cover the 441 pieces (the
// last has 57); 7 B workgroups, no grid cap.
constexpr int PLANE_REC = FI_ATARI_PLANE_RECORD_BYTES;
constexpr int kPlaneBytes = 84 * 84;
constexpr int kPlanePieces = kPlaneBytes / 16;                // 441 16-byte pieces per plane
constexpr int kPlaneRuns = (kPlanePieces + 63) / 64;          // 7 runs of 64 pieces
constexpr int PLANE_REC_MU = kPlaneBytes, PLANE_HDR_ACT = 72;  // action at 7128, +4 reward, +8 discount
constexpr int PLANE_REC_START = 7144;
constexpr int kPlaneMaxActions = 18;
static_assert(kPlanePieces * 16 == kPlaneBytes, "a plane is a whole number of 16-byte pieces");
static_assert(PLANE_REC_MU + 4 * kPlaneMaxActions == PLANE_REC_MU + PLANE_HDR_ACT, "compact header: mu[18], action");
static_assert(PLANE_REC_START + 4 <= PLANE_REC, "plane record header");
static_assert(PLANE_REC == FI_ATARI_PLANE_RECORD_ELEMENTS * FI_RECORD_BYTES, "plane record size");
static_assert(3 * kPlaneBytes <= FI_ATARI_HISTORY_BYTES &&
                  FI_ATARI_HISTORY_BYTES == FI_ATARI_HISTORY_ELEMENTS * FI_RECORD_BYTES, "history block");

// interleave4 (4 pixels of channels 0..3 -> 4 NHWC pixels): interleave.h, shared with gather.hip

__global__ __launch_bounds__(64) void ingest_planes_kernel(const char* __restrict__ rec, int T, int B,
                                                           size_t entry_bytes, uint4* __restrict__ frames) {
    __shared__ uint4 turn[2][64];  // two buffers: one barrier per step
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / kPlaneRuns, run = blockIdx.x - b * kPlaneRuns;
    const int piece = run * 64 + lane;
    const bool live = piece < kPlanePieces;  // the loads of the last run's 7 spare lanes are skipped
    const char* __restrict__ entry = rec + (size_t)b * entry_bytes;
    const uint4* __restrict__ hist = (const uint4*)(entry + (size_t)(T + 1) * PLANE_REC);
    uint32_t w0[4] = {}, w1[4] = {}, w2[4] = {};  // this lane's dwords of the three previous steps
    uint4 next = make_uint4(0u, 0u, 0u, 0u);
    if (live) next = hist[piece];
    for (int t = -3; t <= T; ++t) {
        const uint4 cur = next;
        if (t < T && live) {
            const uint4* src = t + 1 < 0 ? hist + (t + 4) * kPlanePieces
                                         : (const uint4*)(entry + (size_t)(t + 1) * PLANE_REC);
            next = src[piece];
        }
        uint4* x = turn[t & 1];
        x[lane] = cur;
        __syncthreads();
        const uint32_t* xd = (const uint32_t*)x;
        uint32_t n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] = xd[64 * k + lane];
        if (t >= 0) {
            if (*(const uint32_t*)(entry + (size_t)t * PLANE_REC + PLANE_REC_START) != 0u) {
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

int ingest_atari_planes_launch(const void* rec, int T, int B, int A, size_t entry_bytes, uint8_t* frames,
                               float* mu, int32_t* act, float* rew, float* disc, hipStream_t s, int* bad) {
    FI_REQUIRE(rec && frames && mu && act && rew && disc, "ingest_atari_planes: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1, "ingest_atari_planes: bad shape");
    FI_REQUIRE(A <= kPlaneMaxActions, "ingest_atari_planes: the plane record's header holds mu[18]: A = " +
                                          std::to_string(A) + " > 18");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff / kPlaneRuns, "ingest_atari_planes: too many frames");
    FI_REQUIRE(entry_bytes % 16 == 0, "ingest_atari_planes: entry_bytes must be a multiple of 16");
    const size_t need = (size_t)(T + 1) * PLANE_REC + FI_ATARI_HISTORY_BYTES;
    FI_REQUIRE(entry_bytes >= need, "ingest_atari_planes: entry_bytes < " + std::to_string(need) +
                                        " = (T+1)*7168 + 21504");
    FI_REQUIRE((uintptr_t)rec % 16 == 0 && (uintptr_t)frames % 16 == 0,
               "ingest_atari_planes: records and frames must be 16-byte aligned");
    const char* r = (const char*)rec;
    const size_t stride = PLANE_REC;
    hipLaunchKernelGGL(ingest_planes_kernel, dim3((unsigned)(B * kPlaneRuns)), dim3(64), 0, s, r, T, B, entry_bytes,
                       (uint4*)frames);
    hipLaunchKernelGGL(ingest_vec_kernel, dim3(grid_for((size_t)T * B * A)), dim3(256), 0, s, r, T, B, A,
                       PLANE_REC_MU, stride, entry_bytes, mu);
    hipLaunchKernelGGL(ingest_scalar_kernel, dim3(grid_for((size_t)T * B)), dim3(256), 0, s, r, T, B, A,
                       PLANE_REC_MU, PLANE_HDR_ACT, stride, entry_bytes, act, rew, disc, bad);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- reductions
__global__ void colsum_kernel(const float* __restrict__ Y, int M, int N, int rows_per,
                              float* __restrict__ slab) {
    const int m0 = blockIdx.x * rows_per, m1 = min(M, m0 + rows_per);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int m = m0;
        for (; m + 3 < m1; m += 4) {
            s0 += Y[(size_t)m * N + n];
            s1 += Y[(size_t)(m + 1) * N + n];
            s2 += Y[(size_t)(m + 2) * N + n];
            s3 += Y[(size_t)(m + 3) * N + n];
        }
        for (; m < m1; ++m) s0 += Y[(size_t)m * N + n];
        slab[(size_t)blockIdx.x * N + n] = (s0 + s1) + (s2 + s3);
    }
}

__global__ void heads_colsum_kernel(HeadsGrad g, int rows_per, float* __restrict__ slab) {
    const int N = g.A + 1;
    const int m0 = blockIdx.x * rows_per, m1 = min(g.rows, m0 + rows_per);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float s = 0.f;
        for (int m = m0; m < m1; ++m) {
            if (n < g.A) s += m < g.TB ? g.dlog[(size_t)m * g.A + n] : 0.f;
            else s += g.dval[m];
        }
        slab[(size_t)blockIdx.x * N + n] = s;
    }
}

int colsum_partial(const float* Y, int M, int N, int splits, float* slab, hipStream_t s) {
    const int rows_per = (M + splits - 1) / splits;
    hipLaunchKernelGGL(colsum_kernel, dim3(splits), dim3(256), 0, s, Y, M, N, rows_per, slab);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int heads_colsum_partial(const HeadsGrad& g, int splits, float* slab, hipStream_t s) {
    const int rows_per = (g.rows + splits - 1) / splits;
    hipLaunchKernelGGL(heads_colsum_kernel, dim3(splits), dim3(64), 0, s, g, rows_per, slab);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// out[i] = sum_k slab[k][i] over `splits` fp32 partial slabs, in a fixed order (deterministic):
// a block owns 64 consecutive outputs (one per lane); its 4 waves take the splits k = w mod 4
// (4 independent accumulators each) and their partials are combined in wave order.
// out[i] = sum over k < splits of slab[k * stride + i], in a fixed order (deterministic)
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slab, int splits,
                                                           size_t count, size_t stride, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < count) {
        int k = w;
        for (; k + 12 < splits; k += 16) {
            a0 += slab[(size_t)k * stride + i];
            a1 += slab[(size_t)(k + 4) * stride + i];
            a2 += slab[(size_t)(k + 8) * stride + i];
            a3 += slab[(size_t)(k + 12) * stride + i];
        }
        for (; k < splits; k += 4) a0 += slab[(size_t)k * stride + i];
    }
    red[w][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (w == 0 && i < count) out[i] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// first stage for narrow slabs (few outputs, many partials): block (x, g) sums rows
// [32g, 32g + 32) of 64 outputs in a fixed order and leaves the partial in row 32g (the slab
// is scratch: every element is read and rewritten by one thread only)
constexpr int kSlabGroup = 32;
__global__ __launch_bounds__(64) void reduce_slabs_stage1(float* __restrict__ slab, int splits, size_t count) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int k0 = blockIdx.y * kSlabGroup, k1 = min(splits, k0 + kSlabGroup);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int k = k0;
    for (; k + 3 < k1; k += 4) {
        a0 += slab[(size_t)k * count + i];
        a1 += slab[(size_t)(k + 1) * count + i];
        a2 += slab[(size_t)(k + 2) * count + i];
        a3 += slab[(size_t)(k + 3) * count + i];
    }
    for (; k < k1; ++k) a0 += slab[(size_t)k * count + i];
    slab[(size_t)k0 * count + i] = (a0 + a1) + (a2 + a3);
}

int reduce_slabs(float* slab, int splits, size_t count, float* out, hipStream_t s) {
    if (splits >= 4 * kSlabGroup && count < 32768) {  // narrow: one block per 64 outputs would
        const int groups = (splits + kSlabGroup - 1) / kSlabGroup;  // walk all splits serially
        hipLaunchKernelGGL(reduce_slabs_stage1, dim3((unsigned)((count + 63) / 64), (unsigned)groups), dim3(64), 0, s,
                           slab, splits, count);
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 63) / 64)), dim3(256), 0, s, slab, groups,
                           count, (size_t)kSlabGroup * count, out);
    } else {
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 63) / 64)), dim3(256), 0, s, slab, splits,
                           count, count, out);
    }
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

__global__ void sqnorm_part_kernel(const float* __restrict__ g, size_t n, double* part) {
    __shared__ double red[4];
    double s = 0.0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        s += (double)g[i] * (double)g[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void sqnorm_final_kernel(const double* part, int nblk, double* out, const double* vt_part,
                                    int vt_nblk, double* vt_losses, int* nonfinite) {
    __shared__ double red[4][4];
    double s = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) s += part[i];
    for (int i = threadIdx.x; i < vt_nblk; i += blockDim.x) {
        l0 += vt_part[(size_t)i * 3];
        l1 += vt_part[(size_t)i * 3 + 1];
        l2 += vt_part[(size_t)i * 3 + 2];
    }
    s = wave_sum(s);
    l0 = wave_sum(l0);
    l1 = wave_sum(l1);
    l2 = wave_sum(l2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s;
        red[1][threadIdx.x >> 6] = l0;
        red[2][threadIdx.x >> 6] = l1;
        red[3][threadIdx.x >> 6] = l2;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const double* r = red[threadIdx.x];
        const double v = (r[0] + r[1]) + (r[2] + r[3]);
        if (threadIdx.x == 0) {
            *out = v;
            // squares of finite fp32 values summed in fp64 cannot overflow: a non-finite norm
            // means a NaN / Inf gradient element
            if (nonfinite)  // exponent all ones: Inf or NaN (a bit test, immune to fast-math folding)
                *nonfinite = (__double_as_longlong(v) & 0x7FF0000000000000LL) == 0x7FF0000000000000LL;
        } else if (vt_losses) vt_losses[threadIdx.x - 1] = v;
    }
}

int grad_sqnorm(const float* g, size_t n, double* part, int nblk, double* out, hipStream_t s,
                const double* vt_part, int vt_nblk, double* vt_losses, int* nonfinite) {
    hipLaunchKernelGGL(sqnorm_part_kernel, dim3(nblk), dim3(256), 0, s, g, n, part);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, s, part, nblk, out, vt_part,
                       vt_losses ? vt_nblk : 0, vt_losses, nonfinite);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- optimizer
// skip (the learner's flag words): [0] out-of-range actions in the batch (all-reduced),
// [1] non-finite gradient norm -- either leaves parameters and moments as they are. A skipped
// update is also counted in [2] and its reasons OR-ed into [3] (1 = actions, 2 = non-finite)
// until the host reads them, so a step skipped behind others still in flight (asynchronous
// submission) is reported by the next wait, not lost.
__device__ __forceinline__ bool skip_update(int* skip) {
    if (!skip || (skip[0] | skip[1]) == 0) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        skip[2] += 1;
        skip[3] |= (skip[0] != 0 ? 1 : 0) | (skip[1] != 0 ? 2 : 0);
    }
    return true;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                            float b1, float b2, float eps, double bc1, double bc2,
                            const double* sqnorm, float max_norm, int* skip) {
    if (skip_update(skip)) return;
    float scale = 1.f;
    if (max_norm > 0.f) {
        const double norm = sqrt(*sqnorm);
        if (norm > max_norm) scale = (float)((double)max_norm / (norm + 1e-6));
    }
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const double mh = mi / bc1, vh = vi / bc2;
        p[i] = (float)(p[i] - lr * mh / (sqrt(vh) + eps));
    }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, size_t n, float lr,
                           const double* sqnorm, float max_norm, int* skip) {
    if (skip_update(skip)) return;
    float scale = 1.f;
    if (max_norm > 0.f) {
        const double norm = sqrt(*sqnorm);
        if (norm > max_norm) scale = (float)((double)max_norm / (norm + 1e-6));
    }
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        p[i] -= lr * (g[i] * scale);
}

int optimizer_step(int opt, float* p, const float* g, float* m, float* v, size_t n, float lr,
                   float b1, float b2, float eps, double bc1, double bc2, const double* sqnorm,
                   float max_norm, hipStream_t s, int* skip) {
    if (opt == FI_OPT_ADAM)
        hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, g, m, v, n, lr, b1,
                           b2, eps, bc1, bc2, sqnorm, max_norm, skip);
    else
        hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, g, n, lr, sqnorm,
                           max_norm, skip);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

__global__ void to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        const __bf16 h = (__bf16)src[i];  // RNE (v_cvt_pk_bf16_f32)
        dst[i] = __builtin_bit_cast(uint16_t, h);
    }
}

int to_bf16(const float* src, uint16_t* dst, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(to_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// bf16 values in [-1, 1) from a 32-bit hash of the index (timing fills: the clock the chip
// holds depends on the operand data, so candidate algorithms are timed on random-like data)
__global__ void fill_hash_bf16_kernel(uint16_t* __restrict__ dst, size_t n, uint32_t seed) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)i * 0x9E3779B9u ^ seed;
        x ^= x >> 16;
        x *= 0x85EBCA6Bu;
        x ^= x >> 13;
        x *= 0xC2B2AE35u;
        x ^= x >> 16;
        const float v = (float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f;
        dst[i] = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
}

int fill_hash_bf16(void* dst, size_t n, uint32_t seed, hipStream_t s) {
    hipLaunchKernelGGL(fill_hash_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, (uint16_t*)dst, n, seed);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

extern "C" int fi_synth_trajectories(uint64_t seed, int T, int B, int B_glob, int b_off, int A,
                                     int D, float gamma, float* obs, float* mu, int32_t* act,
                                     float* rew, float* disc, uint8_t* frames, void* stream) {
    return fi::synth_launch(seed, T, B, B_glob, b_off, A, D, gamma, obs, mu, act, rew, disc, frames,
                            (hipStream_t)stream);
}

extern "C" int fi_ingest_records(const void* rec, int T, int B, int A, int D, size_t entry_bytes,
                                 float* obs, float* mu, int32_t* act, float* rew, float* disc,
                                 void* stream) {
    return fi::ingest_launch(rec, T, B, A, D, entry_bytes, obs, mu, act, rew, disc,
                             (hipStream_t)stream);
}

extern "C" int fi_ingest_atari_records(const void* rec, int T, int B, int A, size_t entry_bytes,
                                       uint8_t* frames, float* mu, int32_t* act, float* rew,
                                       float* disc, void* stream) {
    return fi::ingest_atari_launch(rec, T, B, A, entry_bytes, frames, mu, act, rew, disc,
                                   (hipStream_t)stream);
}

extern "C" int fi_ingest_atari_planes(const void* rec, int T, int B, int A, size_t entry_bytes,
                                      uint8_t* frames, float* mu, int32_t* act, float* rew,
                                      float* disc, void* stream) {
    return fi::ingest_atari_planes_launch(rec, T, B, A, entry_bytes, frames, mu, act, rew, disc,
                                          (hipStream_t)stream);
}
