// actor.hip -- fi_actor: batched policy inference with action sampling, behind the C ABI of
// include/fi_actor.h. The other side of the loop the learner closes: N environments' observations
// in, the published policy's logits / values and one drawn action per environment out.
//
//   * push_planes_kernel: the per-environment 4-frame stacks (N, 84, 84, 4) u8 live in device
//     memory; a step sends one 84x84 plane per environment and the kernel slides it in
//   * the forward is the learner's own (atari_forward on N frames; f32_linear_fwd x2 +
//     f32_heads_fwd on N rows), unchanged, so a row's logits are the bits the learner computes
//   * sample_actions_kernel: one categorical draw (or the argmax) per row, a counter-based rule a
//     host reference reproduces (fi_actor.h)
//   * a recording handle (fi_rollout.h) also writes every step into the learner's entry format in
//     device memory, with the kernels of rollout.hip, and hands completed unrolls to a learner
//   * the act call and the outcome on device pointers (fi_env.h) enqueue the same launches on the
//     caller's memory, without the copies and without the wait
//   * an exploring handle (fi_explore.h) draws with explore.hip's kernel instead, and records the
//     behaviour logits that kernel writes in place of the policy's
// One HIP stream per handle, no global mutable state, no HIP graphs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "atari.h"
#include "fi_actor.h"
#include "fi_common.h"
#include "fi_env.h"
#include "fi_publish.h"
#include "fi_rollout.h"
#include "host_util.h"
#include "kernels.h"
#include "records.h"

namespace fi {

// ---------------------------------------------------------------- stack push
// stacks[i] (84, 84, 4) u8 <- planes[i] (84, 84) u8, in place. A pixel is one dword of the stack
// (byte c = channel c) and one byte p of the plane: the new dword is (w >> 8) | (p << 24) on a
// shift and p * 0x01010101 on an episode start, one v_perm_b32 either way (interleave4's idiom,
// ingest_kernels.h).
//   A one-wave workgroup owns an environment i and a run of 64 16-byte plane pieces (1,024
// pixels = 256 16-byte stack pieces). Lane j loads plane piece 64 run + j; the wave turns the 256
// plane dwords through LDS so that lane j holds dwords 64k + j (k = 0..3), the four pixels of
// stack piece 64k + j of the run. Every 16-byte load and store is then contiguous over the wave
// (1 KiB). The start flag is uniform per workgroup: one scalar load of the aligned dword that
// holds byte i (gfx950 has no scalar byte load; the dword holds a valid byte, so it lies in the
// array's own page) and a uniform branch -- a start does not read the stack. 7 runs cover the 441
// plane pieces: the last has 57, and 228 = 3 * 64 + 36 stack pieces (the tail lanes are skipped).
// 7 N workgroups, no grid cap. HBM traffic: (2 * 28,224 + 7,056) N bytes (a start: 28,224 fewer).
// kPlaneBytes, kPlanePieces (441), kPlaneRuns (7): records.h; a stack is a frame
constexpr int kStackBytes = kFrameBytes;
constexpr int kStackPieces = kFramePieces;  // 1,764
static_assert((size_t)kStackBytes == AtariNet::kFrameBytes, "a stack is one frame of the policy");

// pixel q of plane dword n into the top byte of stack dword w, the rest one channel down
template <int Q>
__device__ __forceinline__ uint32_t shift_in(uint32_t w, uint32_t n) {
    return __builtin_amdgcn_perm(n, w, ((uint32_t)(4 + Q) << 24) | 0x00030201u);
}
template <int Q>
__device__ __forceinline__ uint32_t fill4(uint32_t n) {
    return __builtin_amdgcn_perm(n, n, (uint32_t)Q * 0x01010101u);
}

__global__ __launch_bounds__(64) void push_planes_kernel(uint4* __restrict__ stacks, const uint4* __restrict__ planes,
                                                         const uint8_t* __restrict__ start) {
    __shared__ uint4 turn[64];
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x / kPlaneRuns, run = blockIdx.x - env * kPlaneRuns;
    const int piece = run * 64 + lane;
    uint4 p = make_uint4(0u, 0u, 0u, 0u);
    if (piece < kPlanePieces) p = planes[(size_t)env * kPlanePieces + piece];
    const uint8_t* __restrict__ fp = start + env;
    const uint32_t fsh = (uint32_t)((uintptr_t)fp & 3u);
    const uint32_t fword = *(const uint32_t*)(fp - fsh);
    const bool first = ((fword >> (8u * fsh)) & 0xffu) != 0u;
    uint4* __restrict__ st = stacks + (size_t)env * kStackPieces + run * 256 + lane;
    const int left = kStackPieces - run * 256 - lane;  // stack pieces from this lane's first to the end
    uint4 w[4];
    if (!first) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (64 * k < left) w[k] = st[64 * k];
    }
    turn[lane] = p;
    __syncthreads();
    const uint32_t* xd = (const uint32_t*)turn;
    uint32_t n[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] = xd[64 * k + lane];
    if (first) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (64 * k < left) st[64 * k] = make_uint4(fill4<0>(n[k]), fill4<1>(n[k]), fill4<2>(n[k]), fill4<3>(n[k]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (64 * k < left)
                st[64 * k] = make_uint4(shift_in<0>(w[k].x, n[k]), shift_in<1>(w[k].y, n[k]),
                                        shift_in<2>(w[k].z, n[k]), shift_in<3>(w[k].w, n[k]));
    }
}

static int push_planes_launch(uint8_t* stacks, const uint8_t* planes, const uint8_t* start, int N, hipStream_t s) {
    FI_REQUIRE(stacks && planes && start, "push_planes: null argument");
    FI_REQUIRE(N >= 1, "push_planes: N must be >= 1");
    FI_REQUIRE(N <= 0x7fffffff / kPlaneRuns, "push_planes: too many environments");
    FI_REQUIRE((uintptr_t)stacks % 16 == 0 && (uintptr_t)planes % 16 == 0,
               "push_planes: stacks and planes must be 16-byte aligned");
    hipLaunchKernelGGL(push_planes_kernel, dim3((unsigned)(N * kPlaneRuns)), dim3(64), 0, s, (uint4*)stacks,
                       (const uint4*)planes, start);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- sampling
// One lane per row, the row (A <= AMAX floats) in registers. The sums run a = 0..A-1 ascending in
// fp32, exactly as fi_actor.h states the rule, so a host reference lands on the same action except
// where u Z falls within rounding of a running sum.
template <int AMAX>
__global__ __launch_bounds__(256) void sample_actions_kernel(const float* __restrict__ logits, int N, int A, int mode,
                                                             uint64_t seed, uint64_t draw, int32_t* __restrict__ actions,
                                                             int* __restrict__ nonfinite) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* __restrict__ row = logits + (size_t)i * A;
    float l[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) l[a] = a < A ? row[a] : 0.f;
    float m = l[0];
    int am = 0;
    bool finite = true;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a < A) {
            finite = finite && (fabsf(l[a]) <= 3.402823466e+38f);  // false for NaN and for +-Inf
            if (l[a] > m) {
                m = l[a];
                am = a;
            }
        }
    int act = 0;
    if (!finite) {
        if (nonfinite) atomicAdd(nonfinite, 1);
    } else if (mode == FI_ACT_GREEDY) {
        act = am;
    } else {
        float Z = 0.f;
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
            if (a < A) {
                l[a] = expf(l[a] - m);
                Z += l[a];
            }
        const uint4 x = philox4(seed, draw * (uint64_t)N + (uint64_t)i, ST_SAMPLE);
        const float u = (float)(x.x >> 8) * 0x1p-24f;
        const float thr = u * Z;
        float c = 0.f;
        bool found = false;
        act = A - 1;
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
            if (a < A) {
                c += l[a];
                if (!found && c > thr) {
                    act = a;
                    found = true;
                }
            }
    }
    actions[i] = act;
}

static int sample_actions_launch(const float* logits, int N, int A, int mode, uint64_t seed, uint64_t draw,
                                 int32_t* actions, int* nonfinite, hipStream_t s) {
    FI_REQUIRE(logits && actions, "sample_actions: null argument");
    FI_REQUIRE(N >= 1, "sample_actions: N must be >= 1");
    FI_REQUIRE(A >= 2 && A <= 64, "sample_actions: 2 <= A <= 64");
    FI_REQUIRE(mode == FI_ACT_SAMPLE || mode == FI_ACT_GREEDY, "sample_actions: unknown mode");
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
#define FI_SAMPLE(M) \
    hipLaunchKernelGGL(sample_actions_kernel<M>, grid, block, 0, s, logits, N, A, mode, seed, draw, actions, nonfinite)
    if (A <= 8) FI_SAMPLE(8);
    else if (A <= 18) FI_SAMPLE(18);
    else if (A <= 32) FI_SAMPLE(32);
    else FI_SAMPLE(64);
#undef FI_SAMPLE
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

}  // namespace fi

using namespace fi;

// ------------------------------------------------------------------ the handle
namespace {
enum { PH_H2D = 0, PH_PUSH, PH_FWD, PH_SAMPLE, PH_D2H, PH_COUNT };
enum { IN_OBS = 0, IN_FRAMES, IN_PLANES };
constexpr size_t kAlign = 256;
size_t round_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
}  // namespace

struct fi_actor {
    fi_actor_config cfg{};
    int dev = 0;
    hipStream_t stream = nullptr;
    int N = 0, A = 0, D = 0, H = 0;
    size_t nparams = 0;
    float* params = nullptr;
    bool have_params = false;
    uint64_t version = 0;
    int mode = FI_ACT_SAMPLE;
    uint64_t seed = 0, draw = 0;
    // inputs on the device
    float* obs = nullptr;        // MLP (N, D)
    uint8_t* frames = nullptr;   // Atari: act_frames' input (N, 84, 84, 4)
    uint8_t* stacks = nullptr;   // Atari: the environments' stacks, pushed by act_planes
    uint8_t* planes = nullptr;   // Atari: (N, 7056) then the N start flags
    AtariNet* atari = nullptr;
    float* h1 = nullptr;  // MLP
    float* h2 = nullptr;
    // outputs, one device block and one D2H copy: actions | values | logits | non-finite row count
    char* out = nullptr;
    size_t off_val = 0, off_log = 0, off_bad = 0, out_bytes = 0;
    char* pin_in = nullptr;
    size_t pin_in_bytes = 0;
    char* pin_out = nullptr;
    bool profiling = false;
    hipEvent_t ev[PH_COUNT + 1] = {};
    double phase_sum[PH_COUNT] = {};
    int phase_calls = 0;
    std::vector<void*> allocs;
    // device act calls (fi_env.h), made by the first one: the event behind the last of them, the
    // count of non-finite rows they add to until fi_actor_sync reads it, and whether one was
    // enqueued since the host last waited for the stream
    hipEvent_t dev_done = nullptr;
    int* dev_bad = nullptr;
    bool dev_pending = false;
    // parameters from device memory (fi_publish.h), made by the first such call: recorded behind the copy
    hipEvent_t params_read = nullptr;
    // exploration (fi_explore.h): filled by explore.hip through actor_explore_state(), its launcher
    // included, so that this file names nothing of explore.hip and links without it
    ExploreState ex;
    // rollout recording (fi_rollout.h): two device buffers of N entries; buf[fill] takes the unroll
    // being acted, buf[ready] (or -1) holds a completed unroll until it is released
    struct {
        int T = 0;  // 0: not recording
        size_t rec = 0, entry = 0;
        char* buf[2] = {nullptr, nullptr};
        hipEvent_t ready_ev[2] = {nullptr, nullptr};
        int fill = 0;
        int t = 0;              // the record of buf[fill] the next act call writes, 0..T
        int ready = -1;
        bool need_outcome = false;  // a step was recorded and its outcome not yet supplied
        int last_buf = -1, last_t = 0;  // where the last act call's whole step went
        float* outcome = nullptr;       // device: N rewards, N discounts
        float* pin_outcome = nullptr;
    } ro;
};

static int dalloc(fi_actor* a, void** p, size_t bytes) {
    FI_TRY(dev_alloc(p, std::max<size_t>(bytes, 16), "actor"));
    a->allocs.push_back(*p);
    return FI_OK;
}

static void rollout_free(fi_actor* a) {
    for (int i = 0; i < 2; ++i) {
        if (a->ro.buf[i]) (void)hipFree(a->ro.buf[i]);
        if (a->ro.ready_ev[i]) (void)hipEventDestroy(a->ro.ready_ev[i]);
    }
    if (a->ro.outcome) (void)hipFree(a->ro.outcome);
    if (a->ro.pin_outcome) (void)hipHostFree(a->ro.pin_outcome);
    a->ro = {};
}

static void destroy(fi_actor* a) {
    if (!a) return;
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    rollout_free(a);
    atari_destroy(a->atari);
    for (void* p : a->allocs) (void)hipFree(p);
    if (a->pin_in) (void)hipHostFree(a->pin_in);
    if (a->pin_out) (void)hipHostFree(a->pin_out);
    for (auto& e : a->ev)
        if (e) (void)hipEventDestroy(e);
    if (a->dev_done) (void)hipEventDestroy(a->dev_done);
    if (a->params_read) (void)hipEventDestroy(a->params_read);
    if (a->ex.eps) (void)hipFree(a->ex.eps);
    if (a->ex.mu) (void)hipFree(a->ex.mu);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

extern "C" void fi_actor_config_init(fi_actor_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = sizeof(*c);
    c->arch = FI_ARCH_MLP;
    c->num_envs = 1;
    c->num_actions = 18;
    c->obs_dim = 128;
    c->hidden = 256;
    c->device = 0;
    c->mode = FI_ACT_SAMPLE;
    c->seed = 0;
}

static int create(const fi_actor_config* cfg, fi_actor** out) {
    FI_REQUIRE(cfg && out, "actor_create: null argument");
    *out = nullptr;
    FI_REQUIRE(cfg->struct_size == sizeof(fi_actor_config), "actor_create: struct_size mismatch");
    FI_REQUIRE(cfg->arch == FI_ARCH_MLP || cfg->arch == FI_ARCH_ATARI, "actor_create: unknown arch");
    FI_REQUIRE(cfg->num_envs >= 1, "actor_create: num_envs must be >= 1");
    FI_REQUIRE(cfg->mode == FI_ACT_SAMPLE || cfg->mode == FI_ACT_GREEDY, "actor_create: unknown mode");
    if (cfg->arch == FI_ARCH_MLP) {
        FI_REQUIRE(cfg->num_actions >= 2 && cfg->num_actions <= 64, "actor_create: 2 <= A <= 64");
        FI_REQUIRE(cfg->obs_dim >= 1 && cfg->obs_dim <= 128 && cfg->hidden >= 1 && cfg->hidden <= 4096,
                   "actor_create: MLP needs 1 <= obs_dim <= 128 (record schema), hidden <= 4096");
    } else {
        FI_REQUIRE(cfg->num_actions >= 2 && cfg->num_actions <= 18,
                   "actor_create: the Atari policy needs 2 <= A <= 18 (the full ALE action set is 18)");
    }
    FI_TRY(use_device(cfg->device, "actor_create"));

    fi_actor* a = new (std::nothrow) fi_actor();
    FI_REQUIRE(a, "actor_create: out of host memory");
    std::unique_ptr<fi_actor, void (*)(fi_actor*)> guard(a, destroy);
    a->cfg = *cfg;
    a->dev = cfg->device;
    a->N = cfg->num_envs;
    a->A = cfg->num_actions;
    a->D = cfg->obs_dim;
    a->H = cfg->hidden;
    a->mode = cfg->mode;
    a->seed = cfg->seed;
    FI_HIP_CHECK(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    for (auto& e : a->ev) FI_HIP_CHECK(hipEventCreate(&e));

    const size_t N = a->N, A = a->A;
    if (cfg->arch == FI_ARCH_MLP) {
        const size_t D = a->D, H = a->H, O = A + 1;
        a->nparams = D * H + H + H * H + H + H * O + O;
        FI_TRY(dalloc(a, (void**)&a->obs, N * D * sizeof(float)));
        FI_TRY(dalloc(a, (void**)&a->h1, N * H * sizeof(float)));
        FI_TRY(dalloc(a, (void**)&a->h2, N * H * sizeof(float)));
        a->pin_in_bytes = N * D * sizeof(float);
    } else {
        // B = N, T = 0: N frames. The net's backward buffers come with it
        a->atari = atari_create(a->N, 0, a->A);
        FI_REQUIRE(a->atari, "actor_create: Atari net allocation failed: " + std::string(fi_last_error()));
        a->nparams = atari_param_count(a->A);
        FI_TRY(dalloc(a, (void**)&a->frames, N * kStackBytes));
        FI_TRY(dalloc(a, (void**)&a->stacks, N * kStackBytes));
        FI_TRY(dalloc(a, (void**)&a->planes, N * kPlaneBytes + round_up(N)));
        FI_HIP_CHECK(hipMemsetAsync(a->stacks, 0, N * kStackBytes, a->stream));
        a->pin_in_bytes = N * kStackBytes;
    }
    FI_TRY(dalloc(a, (void**)&a->params, a->nparams * sizeof(float)));
    a->off_val = round_up(N * sizeof(int32_t));
    a->off_log = a->off_val + round_up(N * sizeof(float));
    a->off_bad = a->off_log + round_up(N * A * sizeof(float));
    a->out_bytes = a->off_bad + sizeof(int);
    FI_TRY(dalloc(a, (void**)&a->out, a->out_bytes));
    FI_HIP_CHECK(hipMemsetAsync(a->out, 0, a->out_bytes, a->stream));
    for (char** p : {&a->pin_in, &a->pin_out}) {
        const size_t bytes = p == &a->pin_in ? a->pin_in_bytes : a->out_bytes;
        const hipError_t e = hipHostMalloc((void**)p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            return fail(FI_ERR_OOM, "actor_create: hipHostMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
        }
    }
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    *out = guard.release();
    return FI_OK;
}

extern "C" int fi_actor_create(const fi_actor_config* cfg, fi_actor** out) {
    return guarded("actor_create", FI_ERR_OOM, [&] { return create(cfg, out); });
}

extern "C" void fi_actor_destroy(fi_actor* a) {
    if (!a) return;
    (void)hipSetDevice(a->dev);
    destroy(a);
}

extern "C" size_t fi_actor_param_count(const fi_actor* a) { return a ? a->nparams : 0; }
extern "C" uint64_t fi_actor_version(const fi_actor* a) { return a ? a->version : 0; }

static int set_params(fi_actor* a, const void* src, size_t bytes, uint64_t version) {
    FI_REQUIRE(a && src, "actor_set_params: null argument");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    std::vector<float> tmp;
    const float* p;
    if (bytes == a->nparams * 4) {
        p = (const float*)src;
    } else if (bytes == a->nparams * 2) {  // bf16 -> fp32: the low 16 bits are zero
        tmp.resize(a->nparams);
        const uint16_t* s = (const uint16_t*)src;
        for (size_t i = 0; i < a->nparams; ++i) {
            const uint32_t u = (uint32_t)s[i] << 16;
            std::memcpy(&tmp[i], &u, 4);
        }
        p = tmp.data();
    } else {
        return fail(FI_ERR_INVALID, "actor_set_params: " + std::to_string(bytes) + " bytes is neither the fp32 blob (" +
                                        std::to_string(a->nparams * 4) + ") nor the bf16 blob (" +
                                        std::to_string(a->nparams * 2) + ")");
    }
    FI_HIP_CHECK(hipMemcpyAsync(a->params, p, a->nparams * 4, hipMemcpyHostToDevice, a->stream));
    if (a->atari) FI_TRY(atari_sync_weights(a->atari, a->params, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    a->version = version;
    a->have_params = true;
    return FI_OK;
}

extern "C" int fi_actor_set_params(fi_actor* a, const void* blob, size_t bytes, uint64_t version) {
    return guarded("actor_set_params", FI_ERR_OOM, [&] { return set_params(a, blob, bytes, version); });
}

// fi_publish.h: the same hand-over from device memory, in stream order, with no wait
extern "C" int fi_actor_set_params_ptr(fi_actor* a, const float* params_dev, size_t count, uint64_t version,
                                       void* ready_event, void** read_event_out) {
    FI_REQUIRE(a, "actor_set_params_ptr: null actor");
    if (read_event_out) *read_event_out = nullptr;
    FI_REQUIRE(count == a->nparams, "actor_set_params_ptr: count " + std::to_string(count) +
                                        " != the handle's parameter count " + std::to_string(a->nparams));
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_TRY(check_dev_span(a->dev, params_dev, count * sizeof(float), 16, "actor_set_params_ptr: params_dev"));
    if (!a->params_read) FI_HIP_CHECK(hipEventCreateWithFlags(&a->params_read, hipEventDisableTiming));
    if (ready_event) FI_HIP_CHECK(hipStreamWaitEvent(a->stream, (hipEvent_t)ready_event, 0));
    FI_HIP_CHECK(hipMemcpyAsync(a->params, params_dev, count * sizeof(float), hipMemcpyDeviceToDevice, a->stream));
    FI_HIP_CHECK(hipEventRecord(a->params_read, a->stream));  // behind the copy: the source is free again
    if (a->atari) FI_TRY(atari_sync_weights(a->atari, a->params, a->stream));
    a->version = version;
    a->have_params = true;
    if (read_event_out) *read_event_out = (void*)a->params_read;
    return FI_OK;
}

extern "C" int fi_actor_read_params(fi_actor* a, float* dst, size_t count) {
    FI_REQUIRE(a && dst, "actor_read_params: null argument");
    FI_REQUIRE(count == a->nparams, "actor_read_params: count " + std::to_string(count) +
                                        " != the handle's parameter count " + std::to_string(a->nparams));
    if (!a->have_params) return fail(FI_ERR_STATE, "actor_read_params: no parameters yet");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_HIP_CHECK(hipMemcpyAsync(dst, a->params, count * sizeof(float), hipMemcpyDeviceToHost, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    return FI_OK;
}

extern "C" int fi_actor_set_mode(fi_actor* a, int mode) {
    FI_REQUIRE(a, "actor_set_mode: null actor");
    FI_REQUIRE(mode == FI_ACT_SAMPLE || mode == FI_ACT_GREEDY, "actor_set_mode: unknown mode");
    a->mode = mode;
    return FI_OK;
}

extern "C" int fi_actor_seed(fi_actor* a, uint64_t seed, uint64_t draw) {
    FI_REQUIRE(a, "actor_seed: null actor");
    a->seed = seed;
    a->draw = draw;
    return FI_OK;
}

// ------------------------------------------------------------------ the act call
static int mlp_forward(fi_actor* a, const float* obs, float* logits, float* values) {
    const int D = a->D, H = a->H, A = a->A;
    const float* W1 = a->params;
    const float* b1 = W1 + (size_t)D * H;
    const float* W2 = b1 + H;
    const float* b2 = W2 + (size_t)H * H;
    const float* Wh = b2 + H;
    const float* bh = Wh + (size_t)H * (A + 1);
    FI_TRY(f32_linear_fwd(obs, a->N, D, W1, b1, H, true, a->h1, a->stream));
    FI_TRY(f32_linear_fwd(a->h1, a->N, H, W2, b2, H, true, a->h2, a->stream));
    FI_TRY(f32_heads_fwd(a->h2, a->N, H, Wh, bh, A, logits, values, a->stream));
    return FI_OK;
}

// One act call's records (fi_rollout.h, the recording rule), enqueued on the handle's stream. The
// call's device tensors -- planes and flags (obs), logits, actions, the stacks -- stay as they are
// until the next act call's H2D copy, which follows in stream order. d_in / d_start: the planes
// and flags (the observations) the call ran on -- the handle's own after a host call, the caller's
// in a device call (fi_env.h).
static int record_step(fi_actor* a, int kind, bool completing, const void* d_in, const uint8_t* d_start,
                       const float* d_log, const int32_t* d_act) {
    auto& ro = a->ro;
    const uint32_t flags = (uint32_t)a->version;
    auto put = [&](int b, int t, bool whole) -> int {
        if (kind == IN_PLANES)
            return record_planes_launch(ro.buf[b], ro.entry, t, (const uint8_t*)d_in, d_start, whole ? d_log : nullptr,
                                        whole ? d_act : nullptr, flags, a->N, a->A, a->stream);
        return record_obs_launch(ro.buf[b], ro.entry, t, (const float*)d_in, a->D, whole ? d_log : nullptr,
                                 whole ? d_act : nullptr, flags, a->N, a->A, a->stream);
    };
    int b = ro.fill, t = ro.t;
    if (completing) {
        FI_TRY(put(ro.fill, ro.T, false));  // record T: the bootstrap plane and episode_start only
        b = ro.fill ^ 1;
        t = 0;
    }
    FI_TRY(put(b, t, true));
    if (t == 0 && kind == IN_PLANES)
        FI_TRY(extract_history_launch(ro.buf[b], ro.entry, (size_t)(ro.T + 1) * ro.rec, a->stacks, a->N, a->stream));
    if (completing) {
        FI_HIP_CHECK(hipEventRecord(ro.ready_ev[ro.fill], a->stream));
        ro.ready = ro.fill;
        ro.fill = b;
    }
    ro.last_buf = b;
    ro.last_t = t;
    ro.t = t + 1;
    ro.need_outcome = true;
    return FI_OK;
}

// The draw of one act call. *d_mu: what a record's mu field takes -- the policy's logits, or, while
// exploration is active in sample mode (fi_explore.h), the behaviour logits the other kernel writes.
static int sample(fi_actor* a, const float* d_log, int32_t* d_act, int* d_bad, const float** d_mu) {
    a->ex.mu_valid = a->ex.active && a->mode == FI_ACT_SAMPLE;
    if (!a->ex.mu_valid) {
        *d_mu = d_log;
        return sample_actions_launch(d_log, a->N, a->A, a->mode, a->seed, a->draw, d_act, d_bad, a->stream);
    }
    FI_REQUIRE(a->ex.launch && a->ex.eps && a->ex.mu, "act: exploration is active without its launcher and buffers");
    *d_mu = a->ex.mu;
    return a->ex.launch(d_log, a->N, a->A, a->ex.tau, a->ex.eps, a->seed, a->draw, d_act, a->ex.mu, d_bad, a->stream);
}

static void mark(fi_actor* a, int i) {
    if (a->profiling) (void)hipEventRecord(a->ev[i], a->stream);
}

// What every act call checks before anything is enqueued or pushed: the policy, the parameters and
// a recording handle's refusals (fi_rollout.h). *completing: the (T+1)-th call of the unroll being filled.
static int act_allowed(fi_actor* a, int kind, const void* in, const uint8_t* start, const std::string& nm,
                       bool* completing) {
    FI_REQUIRE(a, nm + ": null actor");
    if (kind == IN_OBS)
        FI_REQUIRE(a->cfg.arch == FI_ARCH_MLP, nm + ": an Atari handle takes frames or planes (fi_actor_act_frames, "
                                                    "fi_actor_act_planes), not an observation vector");
    else
        FI_REQUIRE(a->cfg.arch == FI_ARCH_ATARI, nm + ": an MLP handle takes observation vectors (fi_actor_act_obs)");
    FI_REQUIRE(in && (kind != IN_PLANES || start), nm + ": null input");
    if (!a->have_params)
        return fail(FI_ERR_STATE, nm + ": no parameters yet (fi_actor_set_params with the learner's published blob)");
    const bool recording = a->ro.T > 0;
    *completing = recording && a->ro.t == a->ro.T;
    if (recording) {
        FI_REQUIRE(kind != IN_FRAMES, nm + ": the handle records a rollout, and stacked records are not produced "
                                           "(fi_actor_act_planes, or fi_rollout_end first)");
        if (a->ro.need_outcome)
            return fail(FI_ERR_STATE, nm + ": the previous step's rewards and discounts were never supplied "
                                           "(fi_rollout_outcome after every act call of a recording handle)");
        if (*completing && a->ro.ready >= 0)
            return fail(FI_ERR_STATE, nm + ": this call completes an unroll, and the previous one has not been "
                                           "released: its buffer takes the next unroll's record 0 (fi_rollout_release)");
    }
    return FI_OK;
}

static int act(fi_actor* a, int kind, const void* in, const uint8_t* start, int32_t* actions, float* logits,
               float* values) {
    static const char* const names[] = {"actor_act_obs", "actor_act_frames", "actor_act_planes"};
    const std::string nm = names[kind];
    bool completing = false;
    FI_TRY(act_allowed(a, kind, in, start, nm, &completing));
    const bool recording = a->ro.T > 0;
    FI_HIP_CHECK(hipSetDevice(a->dev));
    const size_t N = a->N, A = a->A;
    void* dst = nullptr;
    size_t bytes = 0;
    if (kind == IN_OBS) {
        dst = a->obs;
        bytes = N * a->D * sizeof(float);
        std::memcpy(a->pin_in, in, bytes);
    } else if (kind == IN_FRAMES) {
        dst = a->frames;
        bytes = N * kStackBytes;
        std::memcpy(a->pin_in, in, bytes);
    } else {  // the planes, then the flags: one copy
        dst = a->planes;
        bytes = N * kPlaneBytes + N;
        std::memcpy(a->pin_in, in, N * kPlaneBytes);
        std::memcpy(a->pin_in + N * kPlaneBytes, start, N);
    }
    int32_t* d_act = (int32_t*)a->out;
    float* d_val = (float*)(a->out + a->off_val);
    float* d_log = (float*)(a->out + a->off_log);
    int* d_bad = (int*)(a->out + a->off_bad);
    mark(a, PH_H2D);
    FI_HIP_CHECK(hipMemcpyAsync(dst, a->pin_in, bytes, hipMemcpyHostToDevice, a->stream));
    mark(a, PH_PUSH);
    if (kind == IN_PLANES) FI_TRY(push_planes_launch(a->stacks, a->planes, a->planes + N * kPlaneBytes, a->N, a->stream));
    mark(a, PH_FWD);
    if (kind == IN_OBS) FI_TRY(mlp_forward(a, a->obs, d_log, d_val));
    else FI_TRY(atari_forward(a->atari, kind == IN_PLANES ? a->stacks : a->frames, d_log, d_val, a->stream));
    mark(a, PH_SAMPLE);
    FI_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), a->stream));
    const float* d_mu = nullptr;
    FI_TRY(sample(a, d_log, d_act, d_bad, &d_mu));
    mark(a, PH_D2H);
    FI_HIP_CHECK(hipMemcpyAsync(a->pin_out, a->out, a->out_bytes, hipMemcpyDeviceToHost, a->stream));
    mark(a, PH_COUNT);
    a->draw++;
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    a->dev_pending = false;
    // after the outputs' copy and the wait for it: the record kernels sit in none of the profiled
    // phases and the caller does not wait for them
    if (recording)
        FI_TRY(record_step(a, kind, completing, kind == IN_PLANES ? (const void*)a->planes : (const void*)a->obs,
                           a->planes ? a->planes + N * kPlaneBytes : nullptr, d_mu, d_act));
    if (a->profiling) {
        for (int p = 0; p < PH_COUNT; ++p) {
            float ms = 0.f;
            FI_HIP_CHECK(hipEventElapsedTime(&ms, a->ev[p], a->ev[p + 1]));
            a->phase_sum[p] += ms;
        }
        a->phase_calls++;
    }
    if (actions) std::memcpy(actions, a->pin_out, N * sizeof(int32_t));
    if (values) std::memcpy(values, a->pin_out + a->off_val, N * sizeof(float));
    if (logits) std::memcpy(logits, a->pin_out + a->off_log, N * A * sizeof(float));
    int bad = 0;
    std::memcpy(&bad, a->pin_out + a->off_bad, sizeof(int));
    if (bad != 0)
        return fail(FI_ERR_NONFINITE, nm + ": " + std::to_string(bad) + " of " + std::to_string(N) +
                                          " rows hold NaN / Inf logits (their action is 0)");
    return FI_OK;
}

extern "C" int fi_actor_act_obs(fi_actor* a, const float* obs, int32_t* actions, float* logits, float* values) {
    return act(a, IN_OBS, obs, nullptr, actions, logits, values);
}
extern "C" int fi_actor_act_frames(fi_actor* a, const uint8_t* frames, int32_t* actions, float* logits,
                                   float* values) {
    return act(a, IN_FRAMES, frames, nullptr, actions, logits, values);
}
extern "C" int fi_actor_act_planes(fi_actor* a, const uint8_t* planes, const uint8_t* episode_start, int32_t* actions,
                                   float* logits, float* values) {
    return act(a, IN_PLANES, planes, episode_start, actions, logits, values);
}

// ------------------------------------------------------------------ the act call on device pointers (fi_env.h)
// the event and the counter of the device calls, made by the first of them
static int ensure_dev_calls(fi_actor* a) {
    if (!a->dev_done) FI_HIP_CHECK(hipEventCreateWithFlags(&a->dev_done, hipEventDisableTiming));
    if (!a->dev_bad) {
        FI_TRY(dalloc(a, (void**)&a->dev_bad, sizeof(int)));
        FI_HIP_CHECK(hipMemsetAsync(a->dev_bad, 0, sizeof(int), a->stream));
    }
    return FI_OK;
}

// act() without the copies and the wait: the same launches, on the caller's pointers
static int act_dev(fi_actor* a, int kind, const void* in, const uint8_t* start, void* ready_event) {
    const std::string nm = kind == IN_OBS ? "actor_act_obs_dev" : "actor_act_planes_dev";
    bool completing = false;
    FI_TRY(act_allowed(a, kind, in, start, nm, &completing));
    FI_HIP_CHECK(hipSetDevice(a->dev));
    const size_t N = a->N;
    if (kind == IN_OBS) {
        FI_TRY(check_dev_span(a->dev, in, N * a->D * sizeof(float), 16, nm + ": obs_dev"));
    } else {
        FI_TRY(check_dev_span(a->dev, in, N * kPlaneBytes, 16, nm + ": planes_dev"));
        FI_TRY(check_dev_span(a->dev, start, N, 16, nm + ": episode_start_dev"));
    }
    FI_TRY(ensure_dev_calls(a));
    int32_t* d_act = (int32_t*)a->out;
    float* d_val = (float*)(a->out + a->off_val);
    float* d_log = (float*)(a->out + a->off_log);
    if (ready_event) FI_HIP_CHECK(hipStreamWaitEvent(a->stream, (hipEvent_t)ready_event, 0));
    a->dev_pending = true;
    if (kind == IN_PLANES) FI_TRY(push_planes_launch(a->stacks, (const uint8_t*)in, start, a->N, a->stream));
    if (kind == IN_OBS) FI_TRY(mlp_forward(a, (const float*)in, d_log, d_val));
    else FI_TRY(atari_forward(a->atari, a->stacks, d_log, d_val, a->stream));
    // dev_bad is not zeroed here: it adds up until fi_actor_sync reads it
    const float* d_mu = nullptr;
    FI_TRY(sample(a, d_log, d_act, a->dev_bad, &d_mu));
    a->draw++;
    if (a->ro.T > 0) FI_TRY(record_step(a, kind, completing, in, start, d_mu, d_act));
    FI_HIP_CHECK(hipEventRecord(a->dev_done, a->stream));
    return FI_OK;
}

extern "C" int fi_actor_act_planes_dev(fi_actor* a, const uint8_t* planes_dev, const uint8_t* episode_start_dev,
                                       void* ready_event) {
    return act_dev(a, IN_PLANES, planes_dev, episode_start_dev, ready_event);
}
extern "C" int fi_actor_act_obs_dev(fi_actor* a, const float* obs_dev, void* ready_event) {
    return act_dev(a, IN_OBS, obs_dev, nullptr, ready_event);
}

extern "C" int fi_actor_outputs_dev(fi_actor* a, const int32_t** actions_dev, const float** logits_dev,
                                    const float** values_dev, void** done_event) {
    FI_REQUIRE(a, "actor_outputs_dev: null actor");
    if (actions_dev) *actions_dev = (const int32_t*)a->out;
    if (values_dev) *values_dev = (const float*)(a->out + a->off_val);
    if (logits_dev) *logits_dev = (const float*)(a->out + a->off_log);
    if (done_event) *done_event = (void*)a->dev_done;
    return FI_OK;
}

extern "C" void* fi_actor_stream(fi_actor* a) { return a ? (void*)a->stream : nullptr; }

extern "C" int fi_actor_sync(fi_actor* a, int64_t* nonfinite_rows) {
    FI_REQUIRE(a, "actor_sync: null actor");
    if (nonfinite_rows) *nonfinite_rows = 0;
    FI_HIP_CHECK(hipSetDevice(a->dev));
    int bad = 0;
    if (a->dev_bad) FI_HIP_CHECK(hipMemcpyAsync(&bad, a->dev_bad, sizeof(int), hipMemcpyDeviceToHost, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    a->dev_pending = false;
    if (bad == 0) return FI_OK;
    FI_HIP_CHECK(hipMemsetAsync(a->dev_bad, 0, sizeof(int), a->stream));  // ahead of the next call's sampling
    if (nonfinite_rows) *nonfinite_rows = bad;
    return fail(FI_ERR_NONFINITE, "actor_sync: " + std::to_string(bad) + " rows held NaN / Inf logits in the device act "
                                      "calls since the last sync (their action is 0)");
}

extern "C" int fi_actor_reset_stacks(fi_actor* a) {
    FI_REQUIRE(a, "actor_reset_stacks: null actor");
    FI_REQUIRE(a->stacks, "actor_reset_stacks: only an Atari handle has stacks");
    if (a->ro.T > 0)
        return fail(FI_ERR_STATE, "actor_reset_stacks: the handle records a rollout, and a reset would break the "
                                  "history the learner rebuilds (start an episode with episode_start, or "
                                  "fi_rollout_end first)");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_HIP_CHECK(hipMemsetAsync(a->stacks, 0, (size_t)a->N * kStackBytes, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    return FI_OK;
}

extern "C" int fi_actor_read_stacks(fi_actor* a, uint8_t* dst, size_t bytes) {
    FI_REQUIRE(a && dst, "actor_read_stacks: null argument");
    FI_REQUIRE(a->stacks, "actor_read_stacks: only an Atari handle has stacks");
    FI_REQUIRE(bytes == (size_t)a->N * kStackBytes,
               "actor_read_stacks: bytes != num_envs * 28224 = " + std::to_string((size_t)a->N * kStackBytes));
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_HIP_CHECK(hipMemcpyAsync(dst, a->stacks, bytes, hipMemcpyDeviceToHost, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    return FI_OK;
}

extern "C" int fi_actor_set_profiling(fi_actor* a, int on) {
    FI_REQUIRE(a, "actor_set_profiling: null actor");
    a->profiling = on != 0;
    for (double& s : a->phase_sum) s = 0.0;
    a->phase_calls = 0;
    return FI_OK;
}

extern "C" int fi_actor_phase_times(fi_actor* a, float* ms, int n, int* n_calls) {
    FI_REQUIRE(a && ms && n >= 1, "actor_phase_times: bad arguments");
    for (int p = 0; p < n && p < PH_COUNT; ++p)
        ms[p] = a->phase_calls ? (float)(a->phase_sum[p] / a->phase_calls) : 0.f;
    if (n_calls) *n_calls = a->phase_calls;
    for (double& s : a->phase_sum) s = 0.0;
    a->phase_calls = 0;
    return FI_OK;
}

// ------------------------------------------------------------------ exploration (fi_explore.h)
// the handle's exploration state, for explore.hip, which owns the C entry points and the kernel
ExploreState* fi::actor_explore_state(fi_actor* a) { return a ? &a->ex : nullptr; }

// ------------------------------------------------------------------ standalone kernels
extern "C" int fi_push_planes(uint8_t* stacks_dev, const uint8_t* planes_dev, const uint8_t* episode_start_dev, int N,
                              void* stream) {
    return push_planes_launch(stacks_dev, planes_dev, episode_start_dev, N, (hipStream_t)stream);
}

extern "C" int fi_sample_actions(const float* logits_dev, int N, int A, int mode, uint64_t seed, uint64_t draw,
                                 int32_t* actions_dev, int* nonfinite_dev, void* stream) {
    return sample_actions_launch(logits_dev, N, A, mode, seed, draw, actions_dev, nonfinite_dev, (hipStream_t)stream);
}

// ------------------------------------------------------------------ rollout recording (fi_rollout.h)

static int rollout_begin(fi_actor* a, int32_t T) {
    FI_REQUIRE(a, "rollout_begin: null actor");
    FI_REQUIRE(T >= 1 && T <= (1 << 20), "rollout_begin: seq_len must be >= 1");
    if (a->ro.T > 0) return fail(FI_ERR_STATE, "rollout_begin: the handle records already (fi_rollout_end first)");
    const bool atari = a->cfg.arch == FI_ARCH_ATARI;
    FI_REQUIRE(!atari || a->A <= kPlaneMaxActions, "rollout_begin: the plane record's header holds mu[18]");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    auto& ro = a->ro;
    ro.rec = atari ? (size_t)kPlaneRecBytes : (size_t)kMlpRecBytes;
    ro.entry = (size_t)(T + 1) * ro.rec + (atari ? (size_t)kHistoryBytes : 0);
    const size_t bytes = (size_t)a->N * ro.entry;
    std::unique_ptr<fi_actor, void (*)(fi_actor*)> guard(a, rollout_free);
    for (int i = 0; i < 2; ++i) {
        FI_TRY(dev_alloc((void**)&ro.buf[i], bytes, "rollout_begin: rollout buffer " + std::to_string(i) + " of 2"));
        FI_HIP_CHECK(hipMemsetAsync(ro.buf[i], 0, bytes, a->stream));
        FI_HIP_CHECK(hipEventCreateWithFlags(&ro.ready_ev[i], hipEventDisableTiming));
    }
    const size_t ob = 2 * (size_t)a->N * sizeof(float);
    FI_TRY(dev_alloc((void**)&ro.outcome, ob, "rollout_begin: the outcome staging"));
    if (hipHostMalloc((void**)&ro.pin_outcome, ob, hipHostMallocDefault) != hipSuccess) {
        ro.pin_outcome = nullptr;
        (void)hipGetLastError();
        return fail(FI_ERR_OOM, "rollout_begin: the outcome staging (" + std::to_string(ob) + " bytes) cannot be allocated");
    }
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    ro.T = T;
    ro.fill = 0;
    ro.t = 0;
    ro.ready = -1;
    ro.need_outcome = false;
    ro.last_buf = -1;
    guard.release();
    return FI_OK;
}

extern "C" int fi_rollout_begin(fi_actor* a, int32_t seq_len) {
    return guarded("rollout_begin", FI_ERR_OOM, [&] { return rollout_begin(a, seq_len); });
}

extern "C" int fi_rollout_outcome(fi_actor* a, const float* rewards, const float* discounts) {
    FI_REQUIRE(a && rewards && discounts, "rollout_outcome: null argument");
    auto& ro = a->ro;
    if (ro.T == 0) return fail(FI_ERR_STATE, "rollout_outcome: the handle does not record (fi_rollout_begin)");
    if (!ro.need_outcome)
        return fail(FI_ERR_STATE, "rollout_outcome: no act call since the last outcome: every step takes one");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    // the pinned block is free: the act call between two outcomes has waited for the stream (a
    // device act call has not: wait here)
    if (a->dev_pending) {
        FI_HIP_CHECK(hipStreamSynchronize(a->stream));
        a->dev_pending = false;
    }
    const size_t N = a->N;
    std::memcpy(ro.pin_outcome, rewards, N * sizeof(float));
    std::memcpy(ro.pin_outcome + N, discounts, N * sizeof(float));
    FI_HIP_CHECK(hipMemcpyAsync(ro.outcome, ro.pin_outcome, 2 * N * sizeof(float), hipMemcpyHostToDevice, a->stream));
    const bool atari = a->cfg.arch == FI_ARCH_ATARI;
    const size_t field = (size_t)ro.last_t * ro.rec + (atari ? kPlaneRecReward : kMlpRecReward);
    FI_TRY(scatter_outcome_launch(ro.buf[ro.last_buf], ro.entry, field, ro.outcome, a->N, a->stream));
    ro.need_outcome = false;
    return FI_OK;
}

// fi_env.h: the same state machine, the scatter straight from the caller's device arrays
extern "C" int fi_rollout_outcome_dev(fi_actor* a, const float* rewards_dev, const float* discounts_dev,
                                      void* ready_event) {
    FI_REQUIRE(a, "rollout_outcome_dev: null actor");
    auto& ro = a->ro;
    if (ro.T == 0) return fail(FI_ERR_STATE, "rollout_outcome_dev: the handle does not record (fi_rollout_begin)");
    if (!ro.need_outcome)
        return fail(FI_ERR_STATE, "rollout_outcome_dev: no act call since the last outcome: every step takes one");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    const size_t bytes = (size_t)a->N * sizeof(float);
    FI_TRY(check_dev_span(a->dev, rewards_dev, bytes, 16, "rollout_outcome_dev: rewards_dev"));
    FI_TRY(check_dev_span(a->dev, discounts_dev, bytes, 16, "rollout_outcome_dev: discounts_dev"));
    FI_TRY(ensure_dev_calls(a));
    if (ready_event) FI_HIP_CHECK(hipStreamWaitEvent(a->stream, (hipEvent_t)ready_event, 0));
    a->dev_pending = true;
    const bool atari = a->cfg.arch == FI_ARCH_ATARI;
    const size_t field = (size_t)ro.last_t * ro.rec + (atari ? kPlaneRecReward : kMlpRecReward);
    FI_TRY(scatter_outcome_launch(ro.buf[ro.last_buf], ro.entry, field, rewards_dev, discounts_dev, a->N, a->stream));
    ro.need_outcome = false;
    FI_HIP_CHECK(hipEventRecord(a->dev_done, a->stream));
    return FI_OK;
}

extern "C" int fi_rollout_ready(const fi_actor* a) { return a && a->ro.T > 0 && a->ro.ready >= 0 ? 1 : 0; }
extern "C" size_t fi_rollout_entry_bytes(const fi_actor* a) { return a && a->ro.T > 0 ? a->ro.entry : 0; }

static int no_unroll(const fi_actor* a, const char* who) {
    if (a->ro.T == 0) return fail(FI_ERR_STATE, std::string(who) + ": the handle does not record (fi_rollout_begin)");
    return fail(FI_ERR_STATE, std::string(who) + ": no completed unroll waits (record " + std::to_string(a->ro.t) +
                                  " of " + std::to_string(a->ro.T + 1) + " is next)");
}

extern "C" int fi_rollout_acquire(fi_actor* a, const void** entries_dev, size_t* entry_stride, void** ready_event) {
    FI_REQUIRE(a, "rollout_acquire: null actor");
    if (a->ro.T == 0 || a->ro.ready < 0) return no_unroll(a, "rollout_acquire");
    if (entries_dev) *entries_dev = a->ro.buf[a->ro.ready];
    if (entry_stride) *entry_stride = a->ro.entry;
    if (ready_event) *ready_event = (void*)a->ro.ready_ev[a->ro.ready];
    return FI_OK;
}

extern "C" int fi_rollout_release(fi_actor* a, void* consumed_event) {
    FI_REQUIRE(a, "rollout_release: null actor");
    if (a->ro.T == 0 || a->ro.ready < 0) return no_unroll(a, "rollout_release");
    FI_HIP_CHECK(hipSetDevice(a->dev));
    // everything the stream does from here on, the next write to that buffer included, follows the event
    if (consumed_event) FI_HIP_CHECK(hipStreamWaitEvent(a->stream, (hipEvent_t)consumed_event, 0));
    a->ro.ready = -1;
    return FI_OK;
}

extern "C" int fi_rollout_read(fi_actor* a, void* host_dst, size_t bytes) {
    FI_REQUIRE(a && host_dst, "rollout_read: null argument");
    if (a->ro.T == 0 || a->ro.ready < 0) return no_unroll(a, "rollout_read");
    const size_t want = (size_t)a->N * a->ro.entry;
    FI_REQUIRE(bytes == want, "rollout_read: bytes != num_envs * entry bytes = " + std::to_string(want));
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_HIP_CHECK(hipMemcpyAsync(host_dst, a->ro.buf[a->ro.ready], bytes, hipMemcpyDeviceToHost, a->stream));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    return FI_OK;
}

extern "C" int fi_rollout_end(fi_actor* a) {
    FI_REQUIRE(a, "rollout_end: null actor");
    if (a->ro.T == 0) return FI_OK;
    FI_HIP_CHECK(hipSetDevice(a->dev));
    FI_HIP_CHECK(hipStreamSynchronize(a->stream));
    rollout_free(a);
    return FI_OK;
}

// what fi_ring_push_rollout (ring.hip) compares with the ring, and fi_env_rollout (env.hip) with the environment
int fi::actor_info(const fi_actor* a, ActorInfo* out) {
    FI_REQUIRE(a && out, "actor_info: null argument");
    *out = ActorInfo{a->dev, a->N, a->cfg.arch, a->ro.T > 0, a->stream, a->A, a->D, a->H};
    return FI_OK;
}

// What a step from an actor's unroll refuses of the actor (`who`: the call and the subject, "the
// actor" or "actor k"): it records, and its device, policy and unroll length are the learner's;
// whole_batch: its environments are the learner's batch.
static int actor_fits(const fi_actor* a, const LearnerInfo& li, const std::string& who, bool whole_batch) {
    if (a->ro.T == 0) return fail(FI_ERR_STATE, who + " does not record (fi_rollout_begin)");
    auto differs = [&](const char* what, int actor, int learner) {
        return fail(FI_ERR_INVALID, who + "'s " + what + " " + std::to_string(actor) + " != the learner's " +
                                        std::to_string(learner));
    };
    if (a->dev != li.dev) return differs("device", a->dev, li.dev);
    if (a->cfg.arch != li.arch) return differs("arch", a->cfg.arch, li.arch);
    if (a->A != li.A) return differs("num_actions", a->A, li.A);
    if (li.arch == FI_ARCH_MLP && a->D != li.D) return differs("obs_dim", a->D, li.D);
    if (whole_batch && a->N != li.B) return differs("num_envs", a->N, li.B);
    if (a->ro.T != li.T) return differs("rollout seq_len", a->ro.T, li.T);
    return FI_OK;
}

// acquire, step, release. It lives here, not in learner.cpp, because it holds both handles: the
// learner is driven through its C ABI, and learner.cpp stays free of the actor.
extern "C" int fi_learner_step_rollout(fi_learner* l, fi_actor* a, fi_step_stats* out) {
    FI_REQUIRE(l && a, "step_rollout: null argument");
    LearnerInfo li{};
    FI_TRY(learner_info(l, &li));
    FI_TRY(actor_fits(a, li, "step_rollout: the actor", true));
    FI_TRY(require_dev_entries(li.dev_entries_ok, "step_rollout"));
    const void* entries = nullptr;
    size_t stride = 0;
    void* ready = nullptr;
    FI_TRY(fi_rollout_acquire(a, &entries, &stride, &ready));
    const int rc = fi_learner_step_entries_dev(l, entries, stride, ready, out);
    // Any other status: refused or broken before or at the enqueue, the unroll stays. Otherwise the
    // step ran (and was waited for), whatever it then reported: the ingest has read the buffer, and
    // it goes back.
    if (!step_taken(rc)) return rc;
    return finish_taken(rc, [&] { return fi_rollout_release(a, fi_learner_entries_consumed_event(l)); });
}

// ------------------------------------------------------------------ several actors, one batch (fi_gather.h)
// Every actor is checked and found ready before the first is acquired, so a refusal leaves every
// unroll waiting; the learner side (segments, column table, gathering ingest) is learner.cpp's.
static int step_rollouts(fi_learner* l, fi_actor* const* actors, int32_t n, fi_step_stats* out, bool wait,
                         const char* who) {
    const std::string nm = who;
    FI_REQUIRE(l && actors, nm + ": null argument");
    FI_REQUIRE(n >= 1 && n <= FI_MAX_SEGMENTS,
               nm + ": " + std::to_string(n) + " actors, 1 .. " + std::to_string(FI_MAX_SEGMENTS) + " are taken");
    LearnerInfo li{};
    FI_TRY(learner_info(l, &li));
    int64_t envs = 0;
    for (int k = 0; k < n; ++k) {
        const fi_actor* a = actors[k];
        const std::string ak = nm + ": actor " + std::to_string(k);
        FI_REQUIRE(a, ak + " is null");
        for (int j = 0; j < k; ++j) FI_REQUIRE(actors[j] != a, ak + " is actor " + std::to_string(j) + " again");
        FI_TRY(actor_fits(a, li, ak, false));
        envs += a->N;
    }
    FI_REQUIRE(envs == li.B, nm + ": the actors' num_envs sum to " + std::to_string(envs) + " != the learner's batch " +
                                 std::to_string(li.B));
    FI_TRY(require_dev_entries(li.dev_entries_ok, nm));
    for (int k = 0; k < n; ++k)
        if (actors[k]->ro.ready < 0)
            return fail(FI_ERR_STATE, nm + ": actor " + std::to_string(k) + " has no completed unroll (record " +
                                          std::to_string(actors[k]->ro.t) + " of " +
                                          std::to_string(actors[k]->ro.T + 1) + " is next); none was acquired");
    fi_entry_segment segs[FI_MAX_SEGMENTS];
    for (int k = 0; k < n; ++k) {
        segs[k].num_entries = actors[k]->N;
        FI_TRY(fi_rollout_acquire(actors[k], &segs[k].entries_dev, &segs[k].entry_stride, &segs[k].ready_event));
    }
    const int rc = wait ? fi_learner_step_segments_dev(l, segs, n, out) : fi_learner_step_segments_dev_async(l, segs, n);
    // as fi_learner_step_rollout; asynchronously the unrolls go back when the step was enqueued -- the
    // consumed event is recorded behind the ingest either way; after any other status they all stay
    if (!step_taken(rc)) return rc;
    return finish_taken(rc, [&]() -> int {
        for (int k = 0; k < n; ++k) FI_TRY(fi_rollout_release(actors[k], fi_learner_entries_consumed_event(l)));
        return FI_OK;
    });
}

extern "C" int fi_learner_step_rollouts(fi_learner* l, fi_actor* const* actors, int32_t n_actors, fi_step_stats* out) {
    return step_rollouts(l, actors, n_actors, out, true, "step_rollouts");
}

extern "C" int fi_learner_step_rollouts_async(fi_learner* l, fi_actor* const* actors, int32_t n_actors) {
    return step_rollouts(l, actors, n_actors, nullptr, false, "step_rollouts_async");
}
