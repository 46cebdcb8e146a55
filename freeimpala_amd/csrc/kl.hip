// kl.hip -- the learner's adaptive KL penalty (include/fi_kl.h, where the rule stands): c KL(q || pi) on a
// reference policy q of the very batch, the coefficient c in a device block, and every fi_kl_* entry point.
//
//   kl_penalty_kernel   surrogate_loss_kernel's grid and read pattern (row_stream.h) over (pi, q, dlogits):
//                       the pi and q rows of one (t, tile) arrive together in padded LDS rows
//                       (load_run<true>), target_loss_kernel's footprint; one lane per row runs
//                       pair_kl_grad (policy_row.h), which leaves c (pi - q) over the pi row; add_run then
//                       adds the rows onto dlogits where it lies in global memory, read once and written
//                       once -- a third row set does not fit a CU's LDS at A = 64. c = (float)coeff is read
//                       from the block, so a step uses what the previous step's finalize left without a
//                       host round trip. One fp64 partial per workgroup.
//   kl_finalize_kernel  one workgroup: the partials added in a fixed order; rows, kl_sum, mean_kl; then,
//                       unless the optimiser skipped, updates and the adaptation of the coefficient.
// No float atomics. learner.cpp names nothing of this file: fi_kl_enable hangs a KlBlock with the two
// launchers on the handle (kernels.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <new>
#include <string>

#include "fi_common.h"
#include "fi_kl.h"
#include "host_util.h"
#include "kernels.h"
#include "policy_row.h"
#include "row_stream.h"

namespace fi {

namespace {
static_assert(sizeof(fi_kl_stats) == 48 && sizeof(fi_kl_params) == 32, "fi_kl.h fixes both sizes");

struct KlArgs {
    int T, B, A;
    int ct, slices, slice_len;
    const float* __restrict__ pi;
    const float* __restrict__ q;
    float* dlog;
    const fi_kl_stats* state;  // coeff is read
    double* part;              // [ct * slices]
};
}  // namespace

__global__ __launch_bounds__(64 * kWaves) void kl_penalty_kernel(KlArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    __shared__ double red[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int c = (int)blockIdx.x % a.ct, s = (int)blockIdx.x / a.ct;
    const int T = a.T, B = a.B;
    const uint32_t A = (uint32_t)a.A, S = A | 1u;
    const int b0 = c * kCols, nb = min(kCols, B - b0);
    const int t_lo = s * a.slice_len, t_hi = min(T, t_lo + a.slice_len);
    float* const lp = (float*)ssm + (size_t)w * 2 * kCols * S;  // this wave's pi rows (c (pi - q) after the arithmetic),
    float* const lq = lp + kCols * S;                           // then its q rows
    const uint32_t n = (uint32_t)nb * A;
    const float coeff = (float)a.state->coeff;  // uniform over the grid
    double sum[1] = {0.0};
    for (int t0 = t_lo; t0 < t_hi; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_hi;  // wave-uniform
        const uint32_t g0 = ((uint32_t)t * (uint32_t)B + (uint32_t)b0) * A;
        if (live) load_run<true>(a.pi, a.q, lp, lq, g0, n, A, S, lane);
        __syncthreads();  // the rows are in LDS
        if (live && lane < nb) sum[0] += (double)pair_kl_grad(lp + (uint32_t)lane * S, lq + (uint32_t)lane * S, A, coeff);
        __syncthreads();  // the gradient rows are complete
        if (live) add_run(a.dlog, lp, g0, n, A, S, lane);
        __syncthreads();  // the rows have been read: the next round may overwrite them
    }
    block_sums<1, kWaves>(sum, red);
    if (tid == 0) a.part[blockIdx.x] = sum[0];
}

// One workgroup. skip (nullable): the optimiser's flag words.
__global__ __launch_bounds__(kStatThreads) void kl_finalize_kernel(const double* __restrict__ part, int nblk, uint64_t rows,
                                                                   fi_kl_params p, fi_kl_stats* st,
                                                                   const int* __restrict__ skip) {
    __shared__ double red[kWaves];
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < nblk; i += kStatThreads) v[0] += part[i];
    block_sums<1, kWaves>(v, red);
    if (threadIdx.x != 0) return;
    const double mean = v[0] / (double)rows;
    st->rows = rows;
    st->kl_sum = v[0];
    st->mean_kl = mean;
    if (skip && (skip[0] | skip[1]) != 0) return;  // the update was skipped: the coefficient and the counts stay
    st->updates = st->updates + 1;
    if (!p.adapt || !(fabs(mean) < __builtin_inf())) return;  // NaN or Inf: no adaptation
    const double target = (double)p.kl_target, band = (double)p.band, factor = (double)p.factor;
    if (mean > band * target) {
        st->coeff = fmin(st->coeff * factor, (double)p.coeff_max);
        st->raised = st->raised + 1;
    } else if (mean < target / band) {
        st->coeff = fmax(st->coeff / factor, (double)p.coeff_min);
        st->lowered = st->lowered + 1;
    }
}

// ------------------------------------------------------------------ the launchers
namespace {
size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// FI_ERR_INVALID, `who` opens the message
int check_params(const std::string& who, const fi_kl_params* p) {
    FI_REQUIRE(p, who + ": null params");
    FI_REQUIRE(p->reference == FI_KL_REF_BEHAVIOUR || p->reference == FI_KL_REF_TARGET,
               who + ": reference " + std::to_string(p->reference) + " is neither behaviour (0) nor target (1)");
    FI_REQUIRE(p->adapt <= 1u, who + ": adapt " + std::to_string(p->adapt) + " must be 0 or 1");
    FI_REQUIRE(std::isfinite(p->coeff) && p->coeff >= 0.f, who + ": coeff " + std::to_string(p->coeff) + " must be finite and >= 0");
    FI_REQUIRE(std::isfinite(p->kl_target) && p->kl_target > 0.f,
               who + ": kl_target " + std::to_string(p->kl_target) + " must be finite and > 0");
    FI_REQUIRE(std::isfinite(p->band) && p->band > 1.f, who + ": band " + std::to_string(p->band) + " must be finite and > 1");
    FI_REQUIRE(std::isfinite(p->factor) && p->factor > 1.f, who + ": factor " + std::to_string(p->factor) + " must be finite and > 1");
    FI_REQUIRE(std::isfinite(p->coeff_min) && std::isfinite(p->coeff_max) && p->coeff_min > 0.f && p->coeff_min <= p->coeff_max,
               who + ": bounds coeff_min " + std::to_string(p->coeff_min) + ", coeff_max " + std::to_string(p->coeff_max) +
                   " must be finite with 0 < coeff_min <= coeff_max");
    return FI_OK;
}

int check_coeff(const std::string& who, double c) {
    FI_REQUIRE(std::isfinite(c) && c >= 0.0, who + ": coeff " + std::to_string(c) + " must be finite and >= 0");
    return FI_OK;
}

size_t workspace_of(const TilePlan& p) { return pad256((size_t)p.ct * p.slices * sizeof(double)); }

int penalty_launch(int T, int B, int A, const float* pi, const float* q, float* dlog, const void* state, void* ws,
                   size_t ws_bytes, hipStream_t stream) {
    FI_REQUIRE(pi && q && dlog && state && ws, "kl_penalty: null argument");
    TilePlan p{};
    FI_TRY(tile_plan("kl_penalty", T, B, A, &p));
    FI_REQUIRE((uintptr_t)pi % 16 == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)dlog % 16 == 0,
               "kl_penalty: pi, q and dlogits must be 16-byte aligned (16 bytes move per lane and access)");
    FI_REQUIRE((uintptr_t)state % 8 == 0 && (uintptr_t)ws % 8 == 0, "kl_penalty: the state block and ws must be 8-byte aligned");
    FI_REQUIRE(ws_bytes >= workspace_of(p), "kl_penalty: ws_bytes " + std::to_string(ws_bytes) + " < " +
                                                std::to_string(workspace_of(p)) + " = fi_kl_workspace_bytes(" +
                                                std::to_string(T) + ", " + std::to_string(B) + ", " + std::to_string(A) + ")");
    // two padded row sets per wave, target_loss_kernel's footprint: more than 64 KB of dynamic LDS at A > 30
    const size_t lds = 2 * (size_t)kWaves * kCols * (A | 1) * sizeof(float), lds_most = 2 * (size_t)kWaves * kCols * 65 * 4;
    if (lds > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        FI_TRY(raise_lds((const void*)kl_penalty_kernel, raised, lds_most));
    }
    KlArgs a{};
    a.T = T, a.B = B, a.A = A;
    a.ct = p.ct, a.slices = p.slices, a.slice_len = p.slice_len;
    a.pi = pi, a.q = q, a.dlog = dlog;
    a.state = (const fi_kl_stats*)state;
    a.part = (double*)ws;
    hipLaunchKernelGGL(kl_penalty_kernel, dim3((unsigned)(p.ct * p.slices)), dim3(64 * kWaves), lds, stream, a);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int finalize_launch(int T, int B, int A, const fi_kl_params* prm, void* state, const void* ws, size_t ws_bytes, const int* skip,
                    hipStream_t stream) {
    FI_TRY(check_params("kl_finalize", prm));
    FI_REQUIRE(state && ws, "kl_finalize: null argument");
    TilePlan p{};
    FI_TRY(tile_plan("kl_finalize", T, B, A, &p));
    FI_REQUIRE((uintptr_t)state % 8 == 0 && (uintptr_t)ws % 8 == 0, "kl_finalize: the state block and ws must be 8-byte aligned");
    FI_REQUIRE((uintptr_t)skip % 4 == 0, "kl_finalize: skip must be 4-byte aligned");
    FI_REQUIRE(ws_bytes >= workspace_of(p), "kl_finalize: ws_bytes " + std::to_string(ws_bytes) + " < " +
                                                std::to_string(workspace_of(p)) + " = fi_kl_workspace_bytes(" +
                                                std::to_string(T) + ", " + std::to_string(B) + ", " + std::to_string(A) + ")");
    hipLaunchKernelGGL(kl_finalize_kernel, dim3(1), dim3(kStatThreads), 0, stream, (const double*)ws, p.ct * p.slices,
                       (uint64_t)T * (uint64_t)B, *prm, (fi_kl_stats*)state, skip);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ------------------------------------------------------------------ the learner's block
int block_penalty(const KlBlock* b, int T, int B, int A, const float* pi, const float* q, float* dlog, hipStream_t stream) {
    return penalty_launch(T, B, A, pi, q, dlog, b->state, b->ws, b->ws_bytes, stream);
}

int block_adapt(const KlBlock* b, int T, int B, int A, const int* skip, hipStream_t stream) {
    return finalize_launch(T, B, A, &b->prm, b->state, b->ws, b->ws_bytes, skip, stream);
}

void block_free(void* p) {
    KlBlock* b = (KlBlock*)p;
    if (!b) return;
    for (void* q : {b->state, b->ws})
        if (q) (void)hipFree(q);
    delete b;
}

int block_create(const KlView& v, double coeff, KlBlock** out) {
    TilePlan p{};
    if (tile_plan("kl_enable", v.T, v.B, v.A, &p) != FI_OK)
        return fail(FI_ERR_INVALID,
                    "kl_enable: the learner's shape is outside the kernels' (" + std::string(fi_last_error()) + ")");
    KlBlock* b = new (std::nothrow) KlBlock();
    FI_REQUIRE(b, "kl_enable: out of host memory");
    b->penalty = block_penalty;
    b->adapt = block_adapt;
    b->ws_bytes = workspace_of(p);
    int rc = dev_alloc(&b->state, sizeof(fi_kl_stats), "kl_enable: state block");
    if (rc == FI_OK) rc = dev_alloc(&b->ws, b->ws_bytes, "kl_enable: workspace");
    if (rc == FI_OK) {
        fi_kl_stats st{};
        st.coeff = coeff;
        hipError_t e = hipMemcpyAsync(b->state, &st, sizeof(st), hipMemcpyHostToDevice, v.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v.stream);  // st is the stack's
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(FI_ERR_HIP, "kl_enable: initialising the block failed");
        }
    }
    if (rc != FI_OK) {
        block_free(b);
        return rc;
    }
    *out = b;
    return FI_OK;
}

// the view of a handle whose block exists
int enabled_view(fi_learner* l, const char* who, KlView* v) {
    FI_TRY(learner_kl_view(l, v));
    if (!v->block)
        return fail(FI_ERR_STATE, std::string(who) + ": the KL penalty was never on on this handle (fi_kl_enable first)");
    FI_HIP_CHECK(hipSetDevice(v->dev));
    return FI_OK;
}
}  // namespace

}  // namespace fi

using namespace fi;

extern "C" int fi_kl_enable(fi_learner* l, const fi_kl_params* params) {
    FI_REQUIRE(l && params, "kl_enable: null argument");
    FI_TRY(check_params("kl_enable", params));
    KlView v{};
    FI_TRY(learner_kl_view(l, &v));
    if (params->reference == FI_KL_REF_TARGET && !v.has_target)
        return fail(FI_ERR_STATE, "kl_enable: reference target on a handle without a target network (fi_target_enable first)");
    if (params->adapt && v.nranks > 1)
        return fail(FI_ERR_STATE, "kl_enable: the handle is attached to a communicator of " + std::to_string(v.nranks) +
                                      " ranks; each rank would adapt to its own shard's mean KL and the coefficients would part"
                                      " (adapt = 0 is accepted)");
    KlBlock* b = v.block;
    if (!b) {
        FI_HIP_CHECK(hipSetDevice(v.dev));
        FI_TRY(guarded("kl_enable", FI_ERR_OOM, [&] { return block_create(v, (double)params->coeff, &b); }));
        learner_set_kl_block(l, b, block_free);
    }
    b->prm = *params;  // by value into every later launch; the block's coeff is kept
    b->on = true;
    return FI_OK;
}

extern "C" int fi_kl_disable(fi_learner* l) {
    FI_REQUIRE(l, "kl_disable: null learner");
    KlView v{};
    FI_TRY(learner_kl_view(l, &v));
    if (v.block) v.block->on = false;
    return FI_OK;
}

extern "C" int fi_kl_set_coeff(fi_learner* l, double c) {
    FI_REQUIRE(l, "kl_set_coeff: null learner");
    FI_TRY(check_coeff("kl_set_coeff", c));
    KlView v{};
    FI_TRY(enabled_view(l, "kl_set_coeff", &v));
    // behind every enqueued step; the rest of the block is kept
    FI_HIP_CHECK(hipMemcpyAsync(v.block->state, &c, sizeof(c), hipMemcpyHostToDevice, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    return FI_OK;
}

extern "C" int fi_kl_get_state(fi_learner* l, fi_kl_params* params, fi_kl_stats* stats, uint32_t* enabled) {
    FI_REQUIRE(l, "kl_get_state: null learner");
    KlView v{};
    FI_TRY(enabled_view(l, "kl_get_state", &v));
    const KlBlock* b = v.block;
    fi_kl_stats st{};
    FI_HIP_CHECK(hipMemcpyAsync(&st, b->state, sizeof(st), hipMemcpyDeviceToHost, v.stream));
    FI_HIP_CHECK(hipStreamSynchronize(v.stream));
    if (params) *params = b->prm;
    if (stats) *stats = st;
    if (enabled) *enabled = b->on ? 1u : 0u;
    return FI_OK;
}

extern "C" int fi_kl_state_dev(fi_learner* l, const void** ptr) {
    FI_REQUIRE(l && ptr, "kl_state_dev: null argument");
    KlView v{};
    FI_TRY(enabled_view(l, "kl_state_dev", &v));
    *ptr = v.block->state;
    return FI_OK;
}

extern "C" size_t fi_kl_workspace_bytes(int T, int B, int A) {
    TilePlan p{};
    return tile_plan("kl_workspace_bytes", T, B, A, &p) == FI_OK ? workspace_of(p) : 0;
}

extern "C" int fi_kl_penalty_fp32(int T, int B, int A, const float* pi, const float* q, float* dlogits, const void* state_dev,
                                  void* ws, size_t ws_bytes, void* stream) {
    return penalty_launch(T, B, A, pi, q, dlogits, state_dev, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int fi_kl_finalize(int T, int B, int A, const fi_kl_params* params, void* state_dev, const void* ws, size_t ws_bytes,
                              const int* skip, void* stream) {
    return finalize_launch(T, B, A, params, state_dev, ws, ws_bytes, skip, (hipStream_t)stream);
}
