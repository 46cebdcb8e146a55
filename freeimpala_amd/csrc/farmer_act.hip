// farmer_act.hip -- FarmerLstm's acting branch (include/fi_farmer_act.h, where the numeric rule stands): S decision
// points with ragged candidate sets per call, one bf16 LSTM pass per decision point on the launchers of
// farmer_lstm_bf16.hip, an inference torso that keeps every activation in LDS, and the pick on the device.
//
// Operand order as farmer_lstm_bf16.hip: a 32x32x16 MFMA reads, per lane, the 8 consecutive k of one index, lane =
// 32 ((k >> 3) & 1) + (index & 31); a fragment of 32 indices x 16 k is 64 pieces of 16 bytes (1 KiB). The weight
// images hold W_l [512][K] as such fragments, tile-major, k-step next. The torso computes the TRANSPOSED product,
// W rows as the A operand and the candidate rows' activations as the B operand: accumulator register v of a lane
// is output feature (v >> 2) 8 + (lane >> 5) 4 + (v & 3) of candidate row lane & 31, so bias, ReLU and rounding are
// element-wise on the accumulators and a lane hands on runs of 4 consecutive k as one 8-byte LDS store that is
// already the next layer's B operand (row half hf, k-step ks at (hf KS + ks) KiB, lane l at 16 l: conflict-free
// 16-byte reads).
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "farmer_lstm_bf16.h"
#include "fi_common.h"
#include "fi_farmer_act.h"
#include "host_util.h"

namespace fi {
namespace farmer_act {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int IN = 162, H = 128, XW = 484, CAT = H + XW, W = 512, G = 4 * H;
constexpr int KS1 = 39, KSW = W / 16;      // k-steps of the padded layer-1 input (624) and of a hidden layer
constexpr int kRows = 64;                  // candidate rows of a torso workgroup: two 32-row halves
constexpr int kBuf0 = 2 * KS1 * 1024, kBuf1 = 2 * KSW * 1024, kLds = kBuf0 + kBuf1;  // 79,872 + 65,536 = 145,408 B
// the parameter blob of fi_farmer.h, in floats
constexpr size_t oWih = 0, oWhh = oWih + (size_t)G * IN, oBih = oWhh + (size_t)G * H, oBhh = oBih + G, oW1 = oBhh + G,
                 oB1 = oW1 + (size_t)W * CAT, oW2 = oB1 + W, kLayer = (size_t)W * W + W, oW6 = oW2 + 4 * kLayer,
                 oB6 = oW6 + W, kParams = oB6 + 1;
// the torso's images, in bf16 elements: W1 [512][624], then W2..W5 [512][512]
constexpr size_t kImg1 = (size_t)W * KS1 * 16, kImgW = (size_t)W * W, kImgElems = kImg1 + 4 * kImgW;

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline size_t w_off(int l) { return l == 0 ? oW1 : oW2 + (size_t)(l - 1) * kLayer; }
__host__ __device__ inline size_t b_off(int l) { return l == 0 ? oB1 : oW2 + (size_t)(l - 1) * kLayer + (size_t)W * W; }
__host__ __device__ inline size_t img_off(int l) { return l == 0 ? 0 : kImg1 + (size_t)(l - 1) * kImgW; }

// ------------------------------------------------------------------ the images: one 16-byte piece per thread, and
// bsum = b_ih + b_hh for the LSTM's projection behind the last piece
__global__ __launch_bounds__(256) void farmer_act_weights_kernel(const float* __restrict__ p, __bf16* __restrict__ img,
                                                                 float* __restrict__ bsum) {
    const int t = blockIdx.x * 256 + threadIdx.x, pieces = (int)(kImgElems / 8);
    if (t >= pieces) {
        const int i = t - pieces;
        if (i < G) bsum[i] = p[oBih + i] + p[oBhh + i];
        return;
    }
    const int l = t < (int)(kImg1 / 8) ? 0 : 1 + (t - (int)(kImg1 / 8)) / (int)(kImgW / 8);
    const int loc = t - (int)(img_off(l) / 8), KS = l == 0 ? KS1 : KSW, K = l == 0 ? CAT : W;
    const int lane = loc & 63, fr = loc >> 6, n = (fr / KS) * 32 + (lane & 31), k0 = (fr % KS) * 16 + (lane >> 5) * 8;
    const float* w = p + w_off(l) + (size_t)n * K;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)(k0 + e < K ? w[k0 + e] : 0.f);
    *(bf16x8*)(img + (size_t)t * 8) = o;
}

// ------------------------------------------------------------------ row r -> its decision point: the last s with
// offsets[s] <= r (empty decision points own no row), one lane per row
__global__ __launch_bounds__(256) void farmer_act_rows_kernel(const int* __restrict__ offsets, int S, int N,
                                                              int* __restrict__ rowseg) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    int lo = 0, hi = S - 1;  // offsets[lo] <= r holds throughout
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    rowseg[r] = lo;
}

// ------------------------------------------------------------------ the torso
// One layer for the workgroup's 64 rows: wave w owns output features 128 w .. 128 w + 127 (feature tiles 4 w + q) over
// both row halves, 8 accumulator tiles. Every weight fragment, 16 bytes per lane straight from the image in L2, feeds
// the MFMAs of both halves, and the next k-step's four fragments are in flight behind the current eight MFMAs. The
// bias joins in the epilogue.
template <bool TRACE>
__device__ __forceinline__ void layer(const char* __restrict__ in, int KS, const __bf16* __restrict__ img,
                                      const float* __restrict__ bias, char* __restrict__ out, int w, int lane, int row0, int N,
                                      __bf16* __restrict__ trace) {
    const int r = lane & 31, hl = lane >> 5;
    f32x16 acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = f32x16{};
    const bf16x8* wp = (const bf16x8*)img + (size_t)(4 * w) * KS * 64 + lane;
    bf16x8 wa[4], wn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wn[q] = wa[q] = wp[(size_t)q * KS * 64];
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wn[q] = wp[((size_t)q * KS + ks + 1) * 64];
        }
        const bf16x8 b0 = *(const bf16x8*)(in + ks * 1024 + lane * 16);
        const bf16x8 b1 = *(const bf16x8*)(in + (KS + ks) * 1024 + lane * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[q], b0, acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[q], b1, acc[q][1], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) wa[q] = wn[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ft = 4 * w + q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f0 = 32 * ft + 8 * j + 4 * hl;  // features f0 .. f0 + 3: the next layer's k
            const f32x4 b = *(const f32x4*)(bias + f0);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                bf16x4 y;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float s = acc[q][hf][4 * j + i] + b[i];
                    y[i] = (__bf16)(s < 0.f ? 0.f : s);  // a NaN stays a NaN
                }
                // k = f0 + i: k-step 2 ft + (j >> 1), lane half j & 1, elements 4 hl .. 4 hl + 3
                *(bf16x4*)(out + (hf * KSW + 2 * ft + (j >> 1)) * 1024 + (j & 1) * 512 + r * 16 + hl * 8) = y;
                if constexpr (TRACE) {
                    const int row = row0 + hf * 32 + r;
                    if (row < N) *(bf16x4*)(trace + (size_t)row * W + f0) = y;
                }
            }
        }
    }
}

// A 256-thread workgroup owns 64 candidate rows, whatever decision points they belong to; rows past N are staged as
// zeros and stored nowhere. c = [rne(h) | rne(x) | 0] goes into LDS in operand order: per wave step 16 rows x 4
// pieces of 4 values, so a row's 64 bytes are read together (h through the row table, x in place) and the 8-byte
// LDS stores of a step touch every bank twice. The five layers ping-pong between the two buffers with one barrier
// each; the head reads a5 from LDS: wave w takes rows 16 w .. 16 w + 15, lane l row l & 15 and the 16-byte pieces
// (l >> 4) + 4 it, it = 0..15, in ascending k, and two cross-lane additions finish a row.
template <bool TRACE>
__global__ __launch_bounds__(256) void farmer_act_torso_kernel(const float* __restrict__ x, const float* __restrict__ h,
                                                               const int* __restrict__ rowseg, int N,
                                                               const __bf16* __restrict__ img, const float* __restrict__ p,
                                                               float* __restrict__ values, __bf16* __restrict__ trace) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* buf0 = lds;
    char* buf1 = lds + kBuf0;
    const int tid = threadIdx.x, lane = tid & 63, row0 = blockIdx.x * kRows;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const int pp = lane & 3, rr = lane >> 2;
        for (int it = w; it < KS1 * 4; it += 4) {
            const int g = it >> 2, r = (it & 3) * 16 + rr, row = row0 + r, k = 16 * g + 4 * pp;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < N) {
                if (g < H / 16) v = *(const f32x4*)(h + (size_t)rowseg[row] * CAT + k);
                else if (k < CAT) v = *(const f32x4*)(x + (size_t)row * XW + (k - H));
            }
            *(bf16x4*)(buf0 + ((r >> 5) * KS1 + g) * 1024 + (pp >> 1) * 512 + (r & 31) * 16 + (pp & 1) * 8) =
                bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        }
    }
    __syncthreads();
    auto tr = [&](int l) { return TRACE ? trace + (size_t)l * N * W : (__bf16*)nullptr; };  // a_{l+1} of the trace
    layer<TRACE>(buf0, KS1, img + img_off(0), p + b_off(0), buf1, w, lane, row0, N, tr(0));
    __syncthreads();
    layer<TRACE>(buf1, KSW, img + img_off(1), p + b_off(1), buf0, w, lane, row0, N, tr(1));
    __syncthreads();
    layer<TRACE>(buf0, KSW, img + img_off(2), p + b_off(2), buf1, w, lane, row0, N, tr(2));
    __syncthreads();
    layer<TRACE>(buf1, KSW, img + img_off(3), p + b_off(3), buf0, w, lane, row0, N, tr(3));
    __syncthreads();
    layer<TRACE>(buf0, KSW, img + img_off(4), p + b_off(4), buf1, w, lane, row0, N, tr(4));
    __syncthreads();
    const int r = 16 * w + (lane & 15);
    const char* a5 = buf1 + (r >> 5) * KSW * 1024 + (r & 31) * 16;
    const float* w6 = p + oW6;
    float s = 0.f;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int q = (lane >> 4) + 4 * it;  // k = 8 q .. 8 q + 7
        const bf16x8 a = *(const bf16x8*)(a5 + (q >> 1) * 1024 + (q & 1) * 512);
        const f32x4 u0 = *(const f32x4*)(w6 + 8 * q), u1 = *(const f32x4*)(w6 + 8 * q + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf((float)a[e], u0[e], s);
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf((float)a[4 + e], u1[e], s);
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (lane < 16 && row0 + r < N) values[row0 + r] = s + p[oB6];
}

// ------------------------------------------------------------------ the pick: one wave per decision point
// out: actions [S] | explored [S] | best_value [S]
__global__ __launch_bounds__(256) void farmer_act_pick_kernel(const float* __restrict__ values, const int* __restrict__ offsets,
                                                              const float* __restrict__ eps, int S, uint64_t seed,
                                                              uint64_t draw, int* __restrict__ out,
                                                              unsigned long long* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;
    const int lo = offsets[s], n = offsets[s + 1] - lo;
    float bv = -INFINITY;
    int bi = INT_MAX, bad = 0;
    for (int i = lane; i < n; i += 64) {
        const float v = values[lo + i];
        if (!isfinite(v)) ++bad;
        else if (bi == INT_MAX || v > bv) bv = v, bi = i;  // ascending i: the lowest index of a tie stays
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
    }
    bad = wave_sum(bad);
    if (lane != 0) return;
    if (bad) atomicAdd(nonfinite, (unsigned long long)bad);
    int action = bi == INT_MAX ? -1 : bi, explored = 0;
    if (action >= 0) {
        const uint4 wd = philox4(seed, draw * (uint64_t)S + (uint64_t)s, ST_FARMER_ACT);
        if ((double)wd.x * 0x1p-32 < (double)eps[s]) {
            const int j = (int)(((uint64_t)wd.y * (uint64_t)n) >> 32);
            if (isfinite(values[lo + j])) action = j, explored = 1;
        }
    }
    out[s] = action;
    out[S + s] = explored;
    ((float*)out)[2 * S + s] = bv;
}

std::atomic<uint64_t> g_lds_plain{0}, g_lds_trace{0};

}  // namespace
}  // namespace farmer_act
}  // namespace fi

using namespace fi;
using namespace fi::farmer_act;

struct fi_farmer_actor {
    fi_farmer_actor_config cfg{};
    hipStream_t stream = nullptr;
    hipEvent_t published = nullptr;  // set_params_from: the learner's stream up to its last write of the parameters
    hipEvent_t pe[4] = {};           // profiling: around the LSTM, the torso and the pick of the last call
    bool profiling = false, profiled = false;
    float *params = nullptr, *bsum = nullptr;
    __bf16 *img = nullptr, *limg = nullptr;
    float *z = nullptr, *x = nullptr;  // staging of host inputs, allocated with the first host call
    float *xp = nullptr, *cst = nullptr, *cat = nullptr, *values = nullptr;
    __bf16 *gates = nullptr, *hprev = nullptr, *trace = nullptr;
    int *meta = nullptr, *rowseg = nullptr, *out = nullptr;  // meta: offsets [S + 1] | eps [S]
    unsigned long long* nonfinite = nullptr;
    int *h_meta = nullptr, *h_out = nullptr;  // pinned: what the call sends and what it gets back
    uint64_t draw = 0;
    int last_S = 0, last_N = 0;
    bool has_params = false, trace_on = false;
};

template <class P>
static int alloc(P** p, size_t n, const char* what) {
    return dev_alloc((void**)p, sizeof(P) * (n ? n : 1), std::string("farmer_actor_create: ") + what);
}

static int build_images(fi_farmer_actor* a) {
    hipLaunchKernelGGL(farmer_act_weights_kernel, dim3((unsigned)cdiv((int)(kImgElems / 8) + G, 256)), dim3(256), 0, a->stream,
                       a->params, a->img, a->bsum);
    FI_HIP_CHECK(hipGetLastError());
    FI_TRY(farmer::lstm_weights_bf16(a->params + oWih, a->params + oWhh, a->limg, a->stream));
    a->has_params = true;
    return FI_OK;
}

extern "C" void fi_farmer_actor_config_init(fi_farmer_actor_config* cfg) {
    if (!cfg) return;
    *cfg = fi_farmer_actor_config{};
    cfg->max_states = 256, cfg->max_rows = 4096, cfg->seq_len = 10;
}

extern "C" void fi_farmer_actor_destroy(fi_farmer_actor* a) {
    if (!a) return;
    (void)hipSetDevice(a->cfg.device);
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    for (void* p : {(void*)a->params, (void*)a->bsum, (void*)a->img, (void*)a->limg, (void*)a->z, (void*)a->x, (void*)a->xp,
                    (void*)a->cst, (void*)a->cat, (void*)a->values, (void*)a->gates, (void*)a->hprev, (void*)a->trace,
                    (void*)a->meta, (void*)a->rowseg, (void*)a->out, (void*)a->nonfinite})
        if (p) (void)hipFree(p);
    if (a->h_meta) (void)hipHostFree(a->h_meta);
    if (a->h_out) (void)hipHostFree(a->h_out);
    if (a->published) (void)hipEventDestroy(a->published);
    for (hipEvent_t e : a->pe)
        if (e) (void)hipEventDestroy(e);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

static int create(const fi_farmer_actor_config* cfg, fi_farmer_actor** out) {
    FI_REQUIRE(cfg && out, "farmer_actor_create: null argument");
    *out = nullptr;
    FI_REQUIRE(cfg->max_states >= 1 && cfg->max_rows >= 1 && cfg->seq_len >= 1, "farmer_actor_create: max_states, max_rows and seq_len start at 1");
    const size_t S = (size_t)cfg->max_states, N = (size_t)cfg->max_rows, ST = S * (size_t)cfg->seq_len;
    if (ST * G >= ((size_t)1 << 31) || N * W >= ((size_t)1 << 31))
        return fail(FI_ERR_UNSUPPORTED, "farmer_actor_create: max_states seq_len 512 and max_rows 512 stay below 2^31");
    FI_TRY(use_device(cfg->device, "farmer_actor_create"));
    fi_farmer_actor* a = new fi_farmer_actor;
    a->cfg = *cfg;
    int rc = FI_OK;
    auto step = [&](int r) { return rc == FI_OK ? (rc = r) == FI_OK : false; };
    if (hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&a->published, hipEventDisableTiming) != hipSuccess)
        rc = fail(FI_ERR_HIP, "farmer_actor_create: stream or event creation failed");
    step(alloc(&a->params, kParams, "params")) && step(alloc(&a->bsum, G, "bsum")) && step(alloc(&a->img, kImgElems, "images")) &&
        step(alloc(&a->limg, farmer::kLstmImgElems, "LSTM images")) && step(alloc(&a->xp, ST * G, "xp")) &&
        step(alloc(&a->gates, ST * G, "gates")) && step(alloc(&a->cst, ST * H, "c")) && step(alloc(&a->hprev, ST * H, "hprev")) &&
        step(alloc(&a->cat, S * CAT, "h")) && step(alloc(&a->values, N, "values")) && step(alloc(&a->meta, 2 * S + 1, "offsets")) &&
        step(alloc(&a->rowseg, N, "row table")) && step(alloc(&a->out, 3 * S, "actions")) && step(alloc(&a->nonfinite, 1, "counter"));
    if (rc == FI_OK && (hipHostMalloc((void**)&a->h_meta, (2 * S + 1) * 4) != hipSuccess ||
                        hipHostMalloc((void**)&a->h_out, 3 * S * 4) != hipSuccess))
        rc = fail(FI_ERR_OOM, "farmer_actor_create: pinned allocation failed");
    if (rc == FI_OK && hipMemset(a->nonfinite, 0, sizeof(unsigned long long)) != hipSuccess)
        rc = fail(FI_ERR_HIP, "farmer_actor_create: hipMemset failed");
    if (rc != FI_OK) {
        const std::string why = fi_last_error();
        fi_farmer_actor_destroy(a);
        return fail(rc, why);
    }
    *out = a;
    return FI_OK;
}

extern "C" int fi_farmer_actor_create(const fi_farmer_actor_config* cfg, fi_farmer_actor** out) {
    return guarded("farmer_actor_create", FI_ERR_OOM, [&] { return create(cfg, out); });
}

extern "C" int fi_farmer_actor_set_params(fi_farmer_actor* a, const float* host, size_t n) {
    FI_REQUIRE(a && host, "farmer_actor_set_params: null argument");
    FI_REQUIRE(n == kParams, "farmer_actor_set_params: the blob has " + std::to_string(kParams) + " floats");
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    FI_HIP_CHECK(hipMemcpyAsync(a->params, host, n * 4, hipMemcpyHostToDevice, a->stream));
    return build_images(a);
}

extern "C" int fi_farmer_actor_set_params_from(fi_farmer_actor* a, fi_farmer* learner) {
    FI_REQUIRE(a && learner, "farmer_actor_set_params_from: null argument");
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    void* src = nullptr;
    size_t bytes = 0, have = 0;
    FI_TRY(fi_farmer_tensor(learner, "params", &src, &bytes));
    FI_REQUIRE(bytes >= kParams * 4, "farmer_actor_set_params_from: the learner's blob is too small");
    FI_TRY(dev_bytes_behind(a->cfg.device, src, "farmer_actor_set_params_from: the learner's parameters", "actor", &have));
    FI_HIP_CHECK(hipEventRecord(a->published, (hipStream_t)fi_farmer_stream(learner)));
    FI_HIP_CHECK(hipStreamWaitEvent(a->stream, a->published, 0));
    FI_HIP_CHECK(hipMemcpyAsync(a->params, src, kParams * 4, hipMemcpyDeviceToDevice, a->stream));
    return build_images(a);
}

extern "C" int fi_farmer_actor_set_trace(fi_farmer_actor* a, int on) {
    FI_REQUIRE(a, "farmer_actor_set_trace: null handle");
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    if (on && !a->trace) FI_TRY(alloc(&a->trace, (size_t)5 * a->cfg.max_rows * W, "trace"));
    a->trace_on = on != 0;
    return FI_OK;
}

static int act(fi_farmer_actor* a, const float* z, const float* x, int on_device, const int32_t* offsets, int S, float eps,
               const float* eps_per_state, int32_t* actions, int32_t* explored, float* values) {
    const char* who = "farmer_actor_act: ";
    FI_REQUIRE(a && z && offsets && actions && explored, std::string(who) + "null argument");
    if (!a->has_params) return fail(FI_ERR_STATE, std::string(who) + "no parameters yet (fi_farmer_actor_set_params first)");
    FI_REQUIRE(S >= 1 && S <= a->cfg.max_states, who + std::to_string(S) + " decision points, the handle takes 1 .. " +
                                                      std::to_string(a->cfg.max_states));
    FI_REQUIRE(offsets[0] == 0, std::string(who) + "offsets[0] is not 0");
    for (int s = 0; s < S; ++s)
        FI_REQUIRE(offsets[s + 1] >= offsets[s], who + std::string("offsets decrease at ") + std::to_string(s + 1));
    const int N = offsets[S], T = a->cfg.seq_len;
    FI_REQUIRE(N <= a->cfg.max_rows, who + std::to_string(N) + " rows, the handle takes " + std::to_string(a->cfg.max_rows));
    FI_REQUIRE(x || N == 0, std::string(who) + "x is null");
    for (int s = 0; s < S; ++s) {
        const float e = eps_per_state ? eps_per_state[s] : eps;
        FI_REQUIRE(e >= 0.f && e <= 1.f, who + std::string("epsilon outside [0, 1]"));  // a NaN fails both comparisons
    }
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    hipStream_t st = a->stream;
    const size_t nz = (size_t)S * T * IN, nx = (size_t)N * XW;
    if (on_device) {
        FI_TRY(check_dev_span(a->cfg.device, z, nz * 4, 8, std::string(who) + "z"));
        if (N) FI_TRY(check_dev_span(a->cfg.device, x, nx * 4, 16, std::string(who) + "x"));
    } else {
        if (!a->z) FI_TRY(alloc(&a->z, (size_t)a->cfg.max_states * T * IN, "z"));
        if (!a->x) FI_TRY(alloc(&a->x, (size_t)a->cfg.max_rows * XW, "x"));
        FI_HIP_CHECK(hipMemcpyAsync(a->z, z, nz * 4, hipMemcpyHostToDevice, st));
        if (N) FI_HIP_CHECK(hipMemcpyAsync(a->x, x, nx * 4, hipMemcpyHostToDevice, st));
        z = a->z, x = a->x;
    }
    std::memcpy(a->h_meta, offsets, (size_t)(S + 1) * 4);
    float* he = (float*)(a->h_meta + S + 1);
    for (int s = 0; s < S; ++s) he[s] = eps_per_state ? eps_per_state[s] : eps;
    FI_HIP_CHECK(hipMemcpyAsync(a->meta, a->h_meta, (size_t)(2 * S + 1) * 4, hipMemcpyHostToDevice, st));

    const bool prof = a->profiling;
    if (prof) FI_HIP_CHECK(hipEventRecord(a->pe[0], st));
    FI_TRY(farmer::lstm_xproj_bf16(z, S * T, a->limg, a->bsum, a->xp, st));
    FI_TRY(farmer::lstm_fwd_mfma(a->xp, a->limg, S, T, a->gates, a->cst, a->hprev, a->cat, st));
    if (prof) FI_HIP_CHECK(hipEventRecord(a->pe[1], st));
    if (N) {
        hipLaunchKernelGGL(farmer_act_rows_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, a->meta, S, N, a->rowseg);
        const dim3 grid((unsigned)cdiv(N, kRows)), blk(256);
        if (a->trace_on) {
            FI_TRY(raise_lds((const void*)farmer_act_torso_kernel<true>, g_lds_trace, kLds));
            hipLaunchKernelGGL(farmer_act_torso_kernel<true>, grid, blk, kLds, st, x, a->cat, a->rowseg, N, a->img, a->params,
                               a->values, a->trace);
        } else {
            FI_TRY(raise_lds((const void*)farmer_act_torso_kernel<false>, g_lds_plain, kLds));
            hipLaunchKernelGGL(farmer_act_torso_kernel<false>, grid, blk, kLds, st, x, a->cat, a->rowseg, N, a->img, a->params,
                               a->values, (__bf16*)nullptr);
        }
    }
    if (prof) FI_HIP_CHECK(hipEventRecord(a->pe[2], st));
    hipLaunchKernelGGL(farmer_act_pick_kernel, dim3((unsigned)cdiv(S, 4)), dim3(256), 0, st, a->values, a->meta,
                       (const float*)(a->meta + S + 1), S, a->cfg.seed, a->draw, a->out, a->nonfinite);
    FI_HIP_CHECK(hipGetLastError());
    if (prof) FI_HIP_CHECK(hipEventRecord(a->pe[3], st));
    a->profiled = prof;
    a->draw += 1;
    a->last_S = S, a->last_N = N;
    FI_HIP_CHECK(hipMemcpyAsync(a->h_out, a->out, (size_t)3 * S * 4, hipMemcpyDeviceToHost, st));
    if (values && N) FI_HIP_CHECK(hipMemcpyAsync(values, a->values, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    FI_HIP_CHECK(hipStreamSynchronize(st));
    std::memcpy(actions, a->h_out, (size_t)S * 4);
    std::memcpy(explored, a->h_out + S, (size_t)S * 4);
    return FI_OK;
}

extern "C" int fi_farmer_actor_act(fi_farmer_actor* a, const float* z, const float* x, int inputs_on_device,
                                   const int32_t* offsets, int S, float eps, const float* eps_per_state, int32_t* actions,
                                   int32_t* explored, float* values) {
    return guarded("farmer_actor_act", FI_ERR_OOM,
                   [&] { return act(a, z, x, inputs_on_device, offsets, S, eps, eps_per_state, actions, explored, values); });
}

extern "C" int fi_farmer_actor_tensor(fi_farmer_actor* a, const char* name, void** ptr, size_t* bytes) {
    FI_REQUIRE(a && name && ptr && bytes, "farmer_actor_tensor: null argument");
    const std::string n = name;
    const size_t S = (size_t)a->cfg.max_states, N = (size_t)a->cfg.max_rows;
    if (n == "h") *ptr = a->cat, *bytes = S * CAT * 4;
    else if (n == "values") *ptr = a->values, *bytes = N * 4;
    else if (n == "actions") *ptr = a->out, *bytes = (size_t)3 * a->last_S * 4;
    else if (n == "params") *ptr = a->params, *bytes = kParams * 4;
    else if (n == "trace") {
        if (!a->trace) return fail(FI_ERR_STATE, "farmer_actor_tensor: the trace was never on");
        *ptr = a->trace, *bytes = (size_t)5 * a->last_N * W * 2;
    } else return fail(FI_ERR_INVALID, "farmer_actor_tensor: no tensor named " + n);
    return FI_OK;
}

extern "C" int fi_farmer_actor_nonfinite(fi_farmer_actor* a, uint64_t* rows) {
    FI_REQUIRE(a && rows, "farmer_actor_nonfinite: null argument");
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    unsigned long long v = 0;
    FI_HIP_CHECK(hipMemcpyAsync(&v, a->nonfinite, sizeof(v), hipMemcpyDeviceToHost, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    *rows = v;
    return FI_OK;
}

extern "C" int fi_farmer_actor_set_profiling(fi_farmer_actor* a, int on) {
    FI_REQUIRE(a, "farmer_actor_set_profiling: null handle");
    FI_HIP_CHECK(hipSetDevice(a->cfg.device));
    for (hipEvent_t& e : a->pe)
        if (on && !e) FI_HIP_CHECK(hipEventCreate(&e));
    a->profiling = on != 0;
    return FI_OK;
}

extern "C" int fi_farmer_actor_kernel_ms(fi_farmer_actor* a, float* lstm_ms, float* torso_ms, float* pick_ms) {
    FI_REQUIRE(a && lstm_ms && torso_ms && pick_ms, "farmer_actor_kernel_ms: null argument");
    if (!a->profiled) return fail(FI_ERR_STATE, "farmer_actor_kernel_ms: the last call was not profiled");
    FI_HIP_CHECK(hipEventElapsedTime(lstm_ms, a->pe[0], a->pe[1]));
    FI_HIP_CHECK(hipEventElapsedTime(torso_ms, a->pe[1], a->pe[2]));
    FI_HIP_CHECK(hipEventElapsedTime(pick_ms, a->pe[2], a->pe[3]));
    return FI_OK;
}

extern "C" void* fi_farmer_actor_stream(fi_farmer_actor* a) { return a ? (void*)a->stream : nullptr; }
