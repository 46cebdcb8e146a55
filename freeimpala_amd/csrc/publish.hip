// publish.hip -- parameter publication on the device, behind the C ABI of include/fi_publish.h:
// the learner's parameters reach its actors through stream order alone.
//
//   * publish_params_kernel: params -> a snapshot slot in the published form (fp32 as it is, or
//     rounded to bf16 and widened), 16 bytes per lane and access, a scalar tail, a grid stride; one
//     lane writes the slot's header {exact version, n}
//   * the publication block of a learner: two slots, their events, the reader events and a host
//     record under a mutex. It hangs on the learner handle as an opaque pointer (kernels.h), so
//     learner.cpp names nothing of this file
//   * fi_actor_set_params_dev: the newest slot into an actor through fi_actor_set_params_ptr
//     (actor.hip), and a reader event against the slot on the actor's stream
// No global mutable state, no HIP graphs.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <string>

#include "fi_common.h"
#include "fi_publish.h"
#include "host_util.h"
#include "kernels.h"

namespace fi {

// f2bf of learner.cpp and the widening of fi_actor_set_params in one: the upper 16 bits rounded to
// nearest even, the lower 16 zero. All exponent bits set: the upper half stays, with bit 6 set when
// a lower bit was (a NaN whose payload sat in the lower half alone would otherwise become an Inf).
// No carry leaves the word: the largest u that takes the sum is 0xff7fffff.
__device__ __forceinline__ uint32_t round_bf16_bits(uint32_t u) {
    if ((u & 0x7f800000u) == 0x7f800000u) return (u & 0xffff0000u) | ((u & 0xffffu) ? 0x400000u : 0u);
    return (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
}

template <bool kBf16>
__device__ __forceinline__ float publish_one(float x) {
    if (!kBf16) return x;
    return __uint_as_float(round_bf16_bits(__float_as_uint(x)));
}

// dst[i] = published(src[i]), i < n. n4 = n / 4 whole quads, one float4 per lane and access; the
// n mod 4 elements behind them one per lane. header (nullable): {tag - *skipped, n}, by lane 0 of
// workgroup 0. src and dst never alias (a slot is its own allocation).
template <bool kBf16>
__global__ __launch_bounds__(256) void publish_params_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                             size_t n, size_t n4, uint64_t* __restrict__ header,
                                                             uint64_t tag, const int* __restrict__ skipped) {
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const float4* __restrict__ s4 = (const float4*)src;
    float4* __restrict__ d4 = (float4*)dst;
    for (size_t i = tid; i < n4; i += stride) {
        float4 v = s4[i];
        v.x = publish_one<kBf16>(v.x);
        v.y = publish_one<kBf16>(v.y);
        v.z = publish_one<kBf16>(v.z);
        v.w = publish_one<kBf16>(v.w);
        d4[i] = v;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) dst[i] = publish_one<kBf16>(src[i]);
    if (header && tid == 0) {
        header[0] = tag - (uint64_t)(skipped ? *skipped : 0);
        header[1] = (uint64_t)n;
    }
}

static int publish_launch(float* dst, const float* src, size_t n, int dtype, uint64_t* header, uint64_t tag,
                          const int* skipped, hipStream_t s) {
    FI_REQUIRE(dtype == FI_PUBLISH_FP32 || dtype == FI_PUBLISH_BF16, "publish: unknown dtype " + std::to_string(dtype));
    FI_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 15) == 0,
               "publish: dst and src must be 16-byte aligned (16 bytes move per lane and access)");
    if (n == 0 && !header) return FI_OK;
    const size_t n4 = n / 4;
    // one quad per lane up to 2,048 workgroups (8 per CU), which covers the Atari policy's 1.69 M
    // parameters (1,655 workgroups); the grid stride takes the rest. At least one workgroup
    size_t wgs = (n4 + (n & 3) + 255) / 256;
    wgs = wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs);
    const dim3 grid((unsigned)wgs), block(256);
    if (dtype == FI_PUBLISH_BF16)
        hipLaunchKernelGGL(publish_params_kernel<true>, grid, block, 0, s, dst, src, n, n4, header, tag, skipped);
    else
        hipLaunchKernelGGL(publish_params_kernel<false>, grid, block, 0, s, dst, src, n, n4, header, tag, skipped);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ------------------------------------------------------------------ the publication block
namespace {
constexpr size_t kHeaderBytes = 16;

struct Reader {
    const fi_actor* who = nullptr;
    hipEvent_t ev = nullptr;  // made on first use, kept for the block's life
};

struct PublishBlock {
    std::mutex mu;
    // constants of the learner, so that an actor's thread reads the block alone
    int dev = 0, arch = 0, A = 0, D = 0, H = 0, dtype = 0;
    size_t nparams = 0;
    char* slot[2] = {nullptr, nullptr};  // header, then nparams floats
    hipEvent_t ready[2] = {nullptr, nullptr};
    Reader readers[2][FI_PUBLISH_MAX_READERS];
    int n_readers[2] = {0, 0};  // recorded against the slot since the last publication into it
    uint64_t count = 0;         // publications enqueued
    uint64_t tag[2] = {0, 0};
};

float* snapshot(const PublishBlock* b, int s) { return (float*)(b->slot[s] + kHeaderBytes); }

void block_free(void* p) {
    PublishBlock* b = (PublishBlock*)p;
    if (!b) return;
    for (int s = 0; s < 2; ++s) {
        // an actor's copy from the slot may still run: the slot goes when its readers are through
        for (Reader& r : b->readers[s])
            if (r.ev) {
                (void)hipEventSynchronize(r.ev);
                (void)hipEventDestroy(r.ev);
            }
        if (b->ready[s]) (void)hipEventDestroy(b->ready[s]);
        if (b->slot[s]) (void)hipFree(b->slot[s]);
    }
    delete b;
}

int block_create(const PublishView& v, PublishBlock** out) {
    PublishBlock* b = new (std::nothrow) PublishBlock();
    FI_REQUIRE(b, "publish_params: out of host memory");
    b->dev = v.dev, b->arch = v.arch, b->A = v.A, b->D = v.D, b->H = v.H, b->dtype = v.dtype;
    b->nparams = v.nparams;
    const size_t bytes = kHeaderBytes + v.nparams * sizeof(float);
    for (int s = 0; s < 2; ++s) {
        const int rc = dev_alloc((void**)&b->slot[s], bytes, "publish_params: snapshot slot " + std::to_string(s) + " of 2");
        if (rc != FI_OK) {
            block_free(b);
            return rc;
        }
        if (hipEventCreateWithFlags(&b->ready[s], hipEventDisableTiming) != hipSuccess) {
            b->ready[s] = nullptr;
            (void)hipGetLastError();
            block_free(b);
            return fail(FI_ERR_HIP, "publish_params: hipEventCreate failed");
        }
    }
    *out = b;
    return FI_OK;
}

int no_publication(const char* who) {
    return fail(FI_ERR_STATE, std::string(who) + ": the learner has published nothing yet (0 publications; "
                                                 "fi_publish_params first)");
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_publish_params(fi_learner* l, uint64_t* tag) {
    PublishView v{};
    FI_TRY(learner_publish_view(l, &v));
    FI_HIP_CHECK(hipSetDevice(v.dev));
    PublishBlock* b = (PublishBlock*)v.block;
    if (!b) {
        FI_TRY(block_create(v, &b));
        learner_set_publish_block(l, b, block_free);
    }
    std::lock_guard<std::mutex> lock(b->mu);
    const int s = (int)(b->count & 1);
    for (int i = 0; i < b->n_readers[s]; ++i) FI_HIP_CHECK(hipStreamWaitEvent(v.stream, b->readers[s][i].ev, 0));
    b->n_readers[s] = 0;  // the waits are enqueued: whoever reads the slot from here on reads the new snapshot
    FI_TRY(publish_launch(snapshot(b, s), v.params, v.nparams, v.dtype, (uint64_t*)b->slot[s], v.version, v.skipped,
                          v.stream));
    FI_HIP_CHECK(hipEventRecord(b->ready[s], v.stream));
    b->tag[s] = v.version;
    b->count++;
    if (tag) *tag = v.version;
    return FI_OK;
}

extern "C" int fi_publish_read(fi_learner* l, float* dst, size_t count, uint64_t* version) {
    PublishView v{};
    FI_TRY(learner_publish_view(l, &v));
    FI_REQUIRE(dst, "publish_read: null destination");
    FI_REQUIRE(count == v.nparams, "publish_read: count " + std::to_string(count) + " != the learner's parameter count " +
                                       std::to_string(v.nparams));
    PublishBlock* b = (PublishBlock*)v.block;
    if (!b) return no_publication("publish_read");
    int s;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (b->count == 0) return no_publication("publish_read");
        s = (int)((b->count - 1) & 1);
    }
    FI_HIP_CHECK(hipSetDevice(v.dev));
    FI_HIP_CHECK(hipEventSynchronize(b->ready[s]));
    FI_HIP_CHECK(hipMemcpy(dst, snapshot(b, s), count * sizeof(float), hipMemcpyDeviceToHost));
    if (version) {
        uint64_t h[2] = {0, 0};
        FI_HIP_CHECK(hipMemcpy(h, b->slot[s], sizeof(h), hipMemcpyDeviceToHost));
        *version = h[0];
    }
    return FI_OK;
}

extern "C" int fi_publish_get_state(fi_learner* l, fi_publish_state* out) {
    PublishView v{};
    FI_TRY(learner_publish_view(l, &v));
    FI_REQUIRE(out, "publish_get_state: null argument");
    *out = fi_publish_state{};
    out->dtype = (uint32_t)v.dtype;
    PublishBlock* b = (PublishBlock*)v.block;
    if (!b) return FI_OK;
    int s;
    {
        std::lock_guard<std::mutex> lock(b->mu);
        if (b->count == 0) return FI_OK;
        s = (int)((b->count - 1) & 1);
        out->publications = b->count;
        out->tag = b->tag[s];
        out->slot = (uint32_t)s;
        out->readers[0] = (uint32_t)b->n_readers[0];
        out->readers[1] = (uint32_t)b->n_readers[1];
    }
    FI_HIP_CHECK(hipSetDevice(v.dev));
    FI_HIP_CHECK(hipEventSynchronize(b->ready[s]));
    uint64_t h[2] = {0, 0};
    FI_HIP_CHECK(hipMemcpy(h, b->slot[s], sizeof(h), hipMemcpyDeviceToHost));
    out->version = h[0];
    return FI_OK;
}

extern "C" void* fi_publish_event(fi_learner* l) {
    PublishBlock* b = (PublishBlock*)learner_publish_block(l);
    if (!b) return nullptr;
    std::lock_guard<std::mutex> lock(b->mu);
    return b->count ? (void*)b->ready[(b->count - 1) & 1] : nullptr;
}

// Runs on the actor's thread, possibly while another thread drives the learner: of the learner it
// reads the block pointer (an atomic load) and then the block under its mutex, nothing else.
extern "C" int fi_actor_set_params_dev(fi_actor* a, fi_learner* l) {
    FI_REQUIRE(a && l, "actor_set_params_dev: null argument");
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    PublishBlock* b = (PublishBlock*)learner_publish_block(l);
    if (!b) return no_publication("actor_set_params_dev");
    auto differs = [&](const char* what, long long actor, long long learner) {
        return fail(FI_ERR_INVALID, std::string("actor_set_params_dev: the actor's ") + what + " " + std::to_string(actor) +
                                        " != the learner's " + std::to_string(learner));
    };
    if (ai.dev != b->dev) return differs("device", ai.dev, b->dev);
    if (ai.arch != b->arch) return differs("arch", ai.arch, b->arch);
    if (ai.A != b->A) return differs("num_actions", ai.A, b->A);
    if (b->arch == FI_ARCH_MLP && ai.D != b->D) return differs("obs_dim", ai.D, b->D);
    if (b->arch == FI_ARCH_MLP && ai.H != b->H) return differs("hidden", ai.H, b->H);
    const size_t have = fi_actor_param_count(a);
    if (have != b->nparams) return differs("parameter count", (long long)have, (long long)b->nparams);
    FI_HIP_CHECK(hipSetDevice(b->dev));

    std::lock_guard<std::mutex> lock(b->mu);
    if (b->count == 0) return no_publication("actor_set_params_dev");
    const int s = (int)((b->count - 1) & 1);
    int r = 0;
    while (r < b->n_readers[s] && b->readers[s][r].who != a) ++r;
    if (r == FI_PUBLISH_MAX_READERS)
        return fail(FI_ERR_STATE, "actor_set_params_dev: slot " + std::to_string(s) + " has " +
                                      std::to_string(FI_PUBLISH_MAX_READERS) + " distinct readers since publication " +
                                      std::to_string(b->count - 1) + " went into it, and takes no more (this would be "
                                      "reader " + std::to_string(FI_PUBLISH_MAX_READERS + 1) + ")");
    Reader& rd = b->readers[s][r];
    if (!rd.ev) FI_HIP_CHECK(hipEventCreateWithFlags(&rd.ev, hipEventDisableTiming));
    FI_TRY(fi_actor_set_params_ptr(a, snapshot(b, s), b->nparams, b->tag[s], (void*)b->ready[s], nullptr));
    // behind the copy on the actor's stream (the operand images are rebuilt from the actor's own
    // copy, so the slot is free a few launches early at worst: an event behind them is still correct)
    FI_HIP_CHECK(hipEventRecord(rd.ev, ai.stream));
    rd.who = a;
    if (r == b->n_readers[s]) b->n_readers[s] = r + 1;
    return FI_OK;
}

extern "C" int fi_publish_copy(float* dst_dev, const float* src_dev, size_t n, int dtype, void* stream) {
    FI_REQUIRE(dst_dev && src_dev, "publish_copy: null pointer");
    return publish_launch(dst_dev, src_dev, n, dtype, nullptr, 0, nullptr, (hipStream_t)stream);
}
