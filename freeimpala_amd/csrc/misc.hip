// misc.hip -- HBM-bound helper kernels of the learner step (gfx950):
//   * synthetic trajectories (Philox4x32-10, bit-identical to the oracle's generator)
//   * ingest: (B, S*1024) SharedBuffer entries -> time-major SoA tensors (MLP records, the
//     Atari records with their 84x84x4 frames, and the single-plane Atari records whose
//     4-frame stack is rebuilt): the kernels of ingest_kernels.h on entries a fixed stride apart
//   * column sums / split-K slab reduction (deterministic, fixed order)
//   * global gradient norm, Adam / SGD / RMSProp with global-norm clipping, fp32 -> bf16
//   * the reward clamp in front of V-trace (include/fi_train.h)
#include <algorithm>

#include "fi_common.h"
#include "fi_train.h"
#include "ingest_kernels.h"
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

// grid_for: ingest_kernels.h
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
// Entries in one buffer, entry_bytes apart: the kernels of ingest_kernels.h with the Strided
// locator (no version block on this path: the flags word is not loaded). Record schemas: records.h.

// Frames of the stacked Atari records -> the time-major frames tensor (T+1, B, 84, 84, 4): a strided
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
            (const uint4*)(rec + (size_t)b * entry_bytes + (size_t)t * kAtariRecBytes) + lane;
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

// mu and action / reward / discount of T records, rec_stride apart, with mu at mu_off and the action at act_off
static void ingest_header(const Strided& at, int mu_off, int act_off, size_t rec_stride, const BatchTensors& to) {
    launch_ingest_vec(at, to.T, to.B, to.A, mu_off, rec_stride, to.mu, to.stream);
    launch_ingest_scalar<Strided, false>(at, to.T, to.B, to.A, act_off, rec_stride, to.act, to.rew, to.disc, to.bad,
                                         nullptr, to.stream);
}

int ingest_launch(const void* rec, size_t entry_bytes, const BatchTensors& to) {
    const int T = to.T, B = to.B;
    FI_REQUIRE(rec && T >= 1 && B >= 1 && to.A >= 1 && to.A <= kMlpMaxActions && to.D <= kMlpMaxObs, "ingest: bad shape");
    FI_REQUIRE(entry_bytes >= (size_t)(T + 1) * kMlpRecBytes, "ingest: entry too small");
    const Strided at{(const char*)rec, entry_bytes};
    if (to.obs) launch_ingest_vec(at, T + 1, B, to.D, kMlpRecObs, kMlpRecBytes, to.obs, to.stream);
    if (to.mu) launch_ingest_vec(at, T, B, to.A, kMlpRecMu, kMlpRecBytes, to.mu, to.stream);
    if (to.act && to.rew && to.disc)
        launch_ingest_scalar<Strided, false>(at, T, B, to.A, kMlpRecAct, kMlpRecBytes, to.act, to.rew, to.disc, to.bad,
                                             nullptr, to.stream);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// workgroups of the frame copy: 8 per CU on 256 CUs, the rest of the frames by grid stride
constexpr int kIngestFramesMaxGrid = 2048;

int ingest_atari_launch(const void* rec, size_t entry_bytes, const BatchTensors& to) {
    const int T = to.T, B = to.B, A = to.A;
    FI_REQUIRE(rec && to.frames && to.mu && to.act && to.rew && to.disc, "ingest_atari: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1 && A <= kMlpMaxActions, "ingest_atari: bad shape");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff, "ingest_atari: too many frames");
    FI_REQUIRE(entry_bytes % 16 == 0, "ingest_atari: entry_bytes must be a multiple of 16");
    FI_REQUIRE(entry_bytes >= (size_t)(T + 1) * kAtariRecBytes,
               "ingest_atari: entry_bytes < " + std::to_string((size_t)(T + 1) * kAtariRecBytes) +
                   " = (T+1)*28672");
    FI_REQUIRE((uintptr_t)rec % 16 == 0 && (uintptr_t)to.frames % 16 == 0,
               "ingest_atari: records and frames must be 16-byte aligned");
    const int n_frames = (T + 1) * B;
    hipLaunchKernelGGL(ingest_frames_kernel, dim3(std::min(n_frames, kIngestFramesMaxGrid)), dim3(256), 0, to.stream,
                       (const char*)rec, n_frames, B, entry_bytes, (uint4*)to.frames);
    ingest_header(Strided{(const char*)rec, entry_bytes}, kAtariRecMu, kAtariRecAct, kAtariRecBytes, to);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int ingest_atari_planes_launch(const void* rec, size_t entry_bytes, const BatchTensors& to) {
    const int T = to.T, B = to.B, A = to.A;
    FI_REQUIRE(rec && to.frames && to.mu && to.act && to.rew && to.disc, "ingest_atari_planes: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1, "ingest_atari_planes: bad shape");
    FI_REQUIRE(A <= kPlaneMaxActions, "ingest_atari_planes: the plane record's header holds mu[18]: A = " +
                                          std::to_string(A) + " > 18");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff / kPlaneRuns, "ingest_atari_planes: too many frames");
    FI_REQUIRE(entry_bytes % 16 == 0, "ingest_atari_planes: entry_bytes must be a multiple of 16");
    const size_t need = plane_history_offset(T) + kHistoryBytes;
    FI_REQUIRE(entry_bytes >= need, "ingest_atari_planes: entry_bytes < " + std::to_string(need) +
                                        " = (T+1)*7168 + 21504");
    FI_REQUIRE((uintptr_t)rec % 16 == 0 && (uintptr_t)to.frames % 16 == 0,
               "ingest_atari_planes: records and frames must be 16-byte aligned");
    const Strided at{(const char*)rec, entry_bytes};
    launch_ingest_planes(at, T, B, to.frames, to.stream);
    ingest_header(at, kPlaneRecMu, kPlaneRecAct, kPlaneRecBytes, to);
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

// RMSProp (include/fi_train.h), fp32, element by element; scale and the skip flags as adam_kernel's.
//   g' = g scale;  v = decay v + (1 - decay) g' g';  d = sqrtf(v + eps) or sqrtf(v) + eps
//   kMom: m = momentum m + g' / d, p -= lr m;  otherwise p -= lr g' / d and m is never touched
// HBM-bound: 20 bytes per element without momentum, 28 with. A lane moves 16 bytes of each stream
// per access, every load of a quad issued before its first store; the n4 whole quads go by grid
// stride and the n mod 4 elements behind them one lane each. n4 = 0 (a pointer off a 16-byte
// boundary) sends every element down the scalar loop: the same arithmetic, the same bits.
template <bool kMom, bool kEpsInSqrt>
__device__ __forceinline__ void rmsprop_one(float& p, float g, float& v, float& m, float scale, float lr, float decay,
                                            float momentum, float eps) {
    const float gs = g * scale;
    const float vi = decay * v + (1.0f - decay) * gs * gs;
    v = vi;
    const float d = kEpsInSqrt ? sqrtf(vi + eps) : sqrtf(vi) + eps;
    const float u = gs / d;
    if (kMom) {
        const float mi = momentum * m + u;
        m = mi;
        p -= lr * mi;
    } else {
        p -= lr * u;
    }
}

template <bool kMom, bool kEpsInSqrt>
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ v, float* __restrict__ m, size_t n,
                                                      size_t n4, float lr, float decay, float momentum, float eps,
                                                      const double* sqnorm, float max_norm, int* skip) {
    if (skip_update(skip)) return;
    float scale = 1.f;
    if (max_norm > 0.f) {
        const double norm = sqrt(*sqnorm);
        if (norm > max_norm) scale = (float)((double)max_norm / (norm + 1e-6));
    }
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4* __restrict__ p4 = (float4*)p;
    const float4* __restrict__ g4 = (const float4*)g;
    float4* __restrict__ v4 = (float4*)v;
    float4* __restrict__ m4 = (float4*)m;
    for (size_t i = tid; i < n4; i += stride) {
        float4 pi = p4[i], vi = v4[i], mi = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gi = g4[i];
        if (kMom) mi = m4[i];
        rmsprop_one<kMom, kEpsInSqrt>(pi.x, gi.x, vi.x, mi.x, scale, lr, decay, momentum, eps);
        rmsprop_one<kMom, kEpsInSqrt>(pi.y, gi.y, vi.y, mi.y, scale, lr, decay, momentum, eps);
        rmsprop_one<kMom, kEpsInSqrt>(pi.z, gi.z, vi.z, mi.z, scale, lr, decay, momentum, eps);
        rmsprop_one<kMom, kEpsInSqrt>(pi.w, gi.w, vi.w, mi.w, scale, lr, decay, momentum, eps);
        v4[i] = vi;
        if (kMom) m4[i] = mi;
        p4[i] = pi;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) {  // the tail, one element per lane
        float pi = p[i], vi = v[i], mi = 0.f;
        if (kMom) mi = m[i];
        rmsprop_one<kMom, kEpsInSqrt>(pi, g[i], vi, mi, scale, lr, decay, momentum, eps);
        v[i] = vi;
        if (kMom) m[i] = mi;
        p[i] = pi;
    }
}

static bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

int rmsprop_step(float* p, const float* g, float* v, float* m, size_t n, float lr, const RmsPropHp& hp,
                 const double* sqnorm, float max_norm, hipStream_t s, int* skip) {
    const bool mom = hp.momentum > 0.f;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(v) && (!mom || aligned16(m));
    const size_t n4 = vec ? n / 4 : 0;
    const dim3 grid(grid_for(vec ? n4 + (n & 3) : n)), block(256);
#define FI_RMS(MOM, EIS)                                                                                          \
    hipLaunchKernelGGL((rmsprop_kernel<MOM, EIS>), grid, block, 0, s, p, g, v, m, n, n4, lr, hp.decay, hp.momentum, \
                       hp.eps, sqnorm, max_norm, skip)
    if (mom) {
        if (hp.eps_in_sqrt) FI_RMS(true, true);
        else FI_RMS(true, false);
    } else {
        if (hp.eps_in_sqrt) FI_RMS(false, true);
        else FI_RMS(false, false);
    }
#undef FI_RMS
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// r clamped to [-c, c] in place (include/fi_train.h), by comparison: a NaN stays a NaN, -0.0 stays
// -0.0, +-Inf becomes +-c. 16 bytes per lane over the n4 whole quads, the tail one element per lane
__device__ __forceinline__ float clip_one(float r, float c) { return r > c ? c : (r < -c ? -c : r); }

__global__ __launch_bounds__(256) void clip_rewards_kernel(float* __restrict__ r, size_t n, size_t n4, float c) {
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4* __restrict__ r4 = (float4*)r;
    for (size_t i = tid; i < n4; i += stride) {
        float4 x = r4[i];
        x.x = clip_one(x.x, c);
        x.y = clip_one(x.y, c);
        x.z = clip_one(x.z, c);
        x.w = clip_one(x.w, c);
        r4[i] = x;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) r[i] = clip_one(r[i], c);
}

int clip_rewards_launch(float* r, size_t n, float c, hipStream_t s) {
    const size_t n4 = aligned16(r) ? n / 4 : 0;
    hipLaunchKernelGGL(clip_rewards_kernel, dim3(grid_for(n4 ? n4 + (n & 3) : n)), dim3(256), 0, s, r, n, n4, c);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int optimizer_step(int opt, float* p, const float* g, float* m, float* v, size_t n, float lr,
                   float b1, float b2, float eps, double bc1, double bc2, const double* sqnorm,
                   float max_norm, hipStream_t s, int* skip, const RmsPropHp* rms) {
    if (opt == FI_TRAIN_OPT_RMSPROP) {
        if (!rms) return fail(FI_ERR_INVALID, "optimizer_step: RMSProp without its hyper-parameters");
        return rmsprop_step(p, g, v, m, n, lr, *rms, sqnorm, max_norm, s, skip);
    }
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

// the standalone entry points: the tensors the caller names, no reject counter
static fi::BatchTensors tensors_of(int arch, int T, int B, int A, int D, float* obs, uint8_t* frames, float* mu,
                                   int32_t* act, float* rew, float* disc, void* stream) {
    return fi::BatchTensors{arch, T, B, A, D, obs, frames, mu, act, rew, disc, nullptr, nullptr, nullptr, (hipStream_t)stream};
}

extern "C" int fi_ingest_records(const void* rec, int T, int B, int A, int D, size_t entry_bytes,
                                 float* obs, float* mu, int32_t* act, float* rew, float* disc,
                                 void* stream) {
    return fi::ingest_launch(rec, entry_bytes, tensors_of(FI_ARCH_MLP, T, B, A, D, obs, nullptr, mu, act, rew, disc, stream));
}

extern "C" int fi_ingest_atari_records(const void* rec, int T, int B, int A, size_t entry_bytes,
                                       uint8_t* frames, float* mu, int32_t* act, float* rew,
                                       float* disc, void* stream) {
    return fi::ingest_atari_launch(rec, entry_bytes,
                                   tensors_of(FI_ARCH_ATARI, T, B, A, 0, nullptr, frames, mu, act, rew, disc, stream));
}

extern "C" int fi_ingest_atari_planes(const void* rec, int T, int B, int A, size_t entry_bytes,
                                      uint8_t* frames, float* mu, int32_t* act, float* rew,
                                      float* disc, void* stream) {
    return fi::ingest_atari_planes_launch(rec, entry_bytes,
                                          tensors_of(FI_ARCH_ATARI, T, B, A, 0, nullptr, frames, mu, act, rew, disc, stream));
}
