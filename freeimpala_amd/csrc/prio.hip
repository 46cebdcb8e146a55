// prio.hip -- prioritised replay for the device entry ring (include/fi_prio.h, gfx950): a table of
// one u32 priority per slot, the draw in proportion to it, and the refresh from the learner's own
// step.
//   * prio_init_kernel: q_init into a run of slots that may wrap
//   * prio_chunk_sums_kernel: the u64 sums of the window's chunks of 1,024 positions
//   * prio_columns_kernel: takes ring_columns_kernel's place -- one wave per column; a replayed
//     column scans the chunk sums, then the 1,024 priorities of the chunk its number falls into
//   * prio_from_td_kernel: a column's priority from vs and values, quantised
//   * prio_from_td_alpha_kernel: the same with the exponent alpha on it (fi_weights.h)
//   * prio_clear_kernel / prio_max_kernel: the refresh's two passes
// The rule (fi_prio.h) is integer arithmetic from the quantised priorities on: q >= 1, capacity
// <= 2^20, so every sum is below 2^51 and exact in u64, and (x * Q) >> 64 with a 64-bit x picks
// r < Q. As in ring.hip every number arrives by value as a kernel argument, stores are ordinary
// vector stores, and the only atomic is the integer maximum of the refresh (a vector atomic, as
// the version fold of gather.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "fi_common.h"
#include "fi_prio.h"
#include "fi_weights.h"
#include "host_util.h"
#include "kernels.h"
#include "ring_handle.h"

namespace fi {

namespace {
constexpr int kChunk = 1024;      // window positions per chunk: 256 lanes x 4, or one wave x 16
constexpr int kMaxChunks = 1024;  // capacity <= 2^20
constexpr int kPerLane = 16;
constexpr int64_t kPrioMaxCapacity = FI_PRIO_MAX_CAPACITY;
constexpr uint32_t kQMax = FI_PRIO_Q_MAX;

// the window of one draw: position j < n_valid is entry lo + j in slot (lo_slot + j) mod C
struct Window {
    const uint32_t* table;
    uint32_t C, lo_slot, n_valid;
};

__device__ __forceinline__ uint32_t window_q(const Window& w, uint32_t j) {
    uint32_t slot = w.lo_slot + j;  // both below 2^20
    if (slot >= w.C) slot -= w.C;
    return j < w.n_valid ? w.table[slot] : 0u;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t a = __shfl((uint32_t)v, lane, 64), b = __shfl((uint32_t)(v >> 32), lane, 64);
    return (uint64_t)a | ((uint64_t)b << 32);
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t a = __shfl_up((uint32_t)v, d, 64), b = __shfl_up((uint32_t)(v >> 32), d, 64);
    return (uint64_t)a | ((uint64_t)b << 32);
}

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = shfl_up64(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// Lane L holds the kPerLane consecutive values v[] of a run of 64 * kPerLane; `r` is below their
// total. Returns, to every lane, the first index of the run whose inclusive sum exceeds r, and in
// *before the sum of the values in front of it.
__device__ __forceinline__ uint32_t wave_search(const uint64_t (&v)[kPerLane], uint64_t r, int lane, uint64_t* before) {
    uint64_t mine = 0;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) mine += v[i];
    const uint64_t incl = wave_scan(mine, lane);
    const uint64_t hit = __ballot(incl > r);
    // r < total, so the last lane's bit is set; should table and sums ever disagree, the last lane
    // still names a position inside the run
    const int src = hit ? __ffsll((unsigned long long)hit) - 1 : 63;
    uint64_t run = incl - mine;
    uint32_t idx = kPerLane - 1;
    bool found = false;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        if (!found && run + v[i] > r) {
            idx = (uint32_t)i;
            found = true;
        }
        if (!found) run += v[i];
    }
    if (!found) run -= v[kPerLane - 1];  // the sum in front of the last value
    *before = shfl64(run, src);
    return (uint32_t)src * kPerLane + __shfl(idx, src, 64);
}
}  // namespace

// ---------------------------------------------------------------- the q_init fill
// slots (first_slot + i) mod C, i < count <= C: one lane per slot, contiguous over the wave
__global__ __launch_bounds__(256) void prio_init_kernel(uint32_t* __restrict__ table, uint32_t C, uint32_t first_slot,
                                                        uint32_t count, uint32_t q) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint32_t slot = first_slot + i;
    if (slot >= C) slot -= C;
    table[slot] = q;
}

static int prio_init_launch(uint32_t* table, int64_t C, uint64_t first_entry, uint64_t count, uint32_t q, hipStream_t s) {
    if (count == 0) return FI_OK;
    FI_REQUIRE(table && C >= 1 && C <= kPrioMaxCapacity && count <= (uint64_t)C, "prio_init: bad arguments");
    hipLaunchKernelGGL(prio_init_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, table, (uint32_t)C,
                       (uint32_t)(first_entry % (uint64_t)C), (uint32_t)count, q);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- the chunk sums
// Workgroup k sums the positions [1024 k, 1024 k + 1024) of the window: four loads per lane, each
// contiguous over the wave, a wave reduction and four partial sums through LDS. Reads 4 * n_valid
// bytes, writes 8 per chunk.
__global__ __launch_bounds__(256) void prio_chunk_sums_kernel(Window w, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[4];
    const uint32_t j0 = blockIdx.x * kChunk + threadIdx.x;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += window_q(w, j0 + 256 * k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += shfl64(s, (int)(threadIdx.x & 63) ^ off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// ---------------------------------------------------------------- the draw
// One wave per column, four to a workgroup. A fresh column (c < n_fresh) is entry tail + c. A
// replayed one: lane L holds the chunk sums 16 L .. 16 L + 15 (absent chunks count 0), the wave
// scan gives Q and, for r = (x * Q) >> 64, the chunk and what remains of r inside it; then lane L
// holds that chunk's priorities 16 L .. 16 L + 15 and the same search gives the position. Lane 0
// stores the column's address and entry index; column 0 also resets the version block.
__global__ __launch_bounds__(256) void prio_columns_kernel(RingBatch rb, Window w, const uint64_t* __restrict__ sums,
                                                           uint32_t n_chunks, const char** __restrict__ cols, int B,
                                                           uint32_t* __restrict__ versions) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave_id();
    if (c == 0 && lane == 0 && versions) {
        versions[0] = 0xffffffffu;
        versions[1] = versions[2] = versions[3] = 0u;
    }
    if (c >= B) return;
    uint64_t e = rb.tail + (uint64_t)c;
    if (c >= rb.n_fresh) {
        const uint4 ph = philox4(rb.seed, rb.draw * (uint64_t)B + (uint64_t)c, ST_PRIO);
        const uint64_t x = ((uint64_t)ph.x << 32) | (uint64_t)ph.y;
        uint64_t v[kPerLane];
        uint64_t mine = 0;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) {
            const uint32_t k = (uint32_t)lane * kPerLane + i;
            v[i] = k < n_chunks ? sums[k] : 0ull;
            mine += v[i];
        }
        const uint64_t Q = shfl64(wave_scan(mine, lane), 63);
        const uint64_t r = __umul64hi(x, Q);
        uint64_t before = 0;
        uint32_t chunk = wave_search(v, r, lane, &before);
        if (chunk >= n_chunks) chunk = n_chunks - 1;
        const uint64_t rem = r - before;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i) v[i] = window_q(w, chunk * kChunk + (uint32_t)lane * kPerLane + i);
        uint32_t j = chunk * kChunk + wave_search(v, rem, lane, &before);
        if (j >= w.n_valid) j = w.n_valid - 1;
        e = rb.lo + (uint64_t)j;
    }
    if (lane != 0) return;
    const uint32_t slot = (uint32_t)(e % (uint64_t)rb.C);
    cols[c] = rb.base + (size_t)slot * rb.entry_bytes;
    if (rb.entries_out) rb.entries_out[c] = e;
}

static int prio_columns_launch(const RingBatch& rb, const uint32_t* table, uint64_t* sums, const void** cols, int B,
                               uint32_t* versions, hipStream_t s) {
    FI_REQUIRE(cols && rb.base && B >= 1, "prio_fill_columns: bad arguments");
    FI_REQUIRE((uintptr_t)cols % 8 == 0 && (uintptr_t)rb.entries_out % 8 == 0 && (uintptr_t)versions % 8 == 0,
               "prio_fill_columns: cols, entries_out and versions must be 8-byte aligned");
    FI_REQUIRE(rb.C >= 1 && rb.C <= (uint32_t)kPrioMaxCapacity,
               "prio_fill_columns: capacity " + std::to_string(rb.C) + " outside 1 .. 2^20 = 1048576");
    FI_REQUIRE(rb.n_fresh >= 0 && rb.n_fresh <= B, "prio_fill_columns: n_fresh " + std::to_string(rb.n_fresh) +
                                                       " outside 0 .. B = " + std::to_string(B));
    FI_REQUIRE(rb.lo + rb.n_valid == rb.tail && rb.n_valid <= rb.C,
               "prio_fill_columns: lo " + std::to_string(rb.lo) + " + n_valid " + std::to_string(rb.n_valid) +
                   " must be tail " + std::to_string(rb.tail) + " and n_valid <= capacity");
    FI_REQUIRE(rb.n_fresh == B || rb.n_valid >= 1, "prio_fill_columns: replayed columns need n_valid >= 1");
    Window w{table, rb.C, (uint32_t)(rb.lo % (uint64_t)rb.C), (uint32_t)rb.n_valid};
    uint32_t n_chunks = 0;
    if (rb.n_fresh < B) {
        FI_REQUIRE(table && sums && (uintptr_t)table % 4 == 0 && (uintptr_t)sums % 8 == 0,
                   "prio_fill_columns: table (4-byte aligned) and chunk_ws (8-byte aligned) are needed");
        n_chunks = (w.n_valid + kChunk - 1) / kChunk;  // <= 1024
        hipLaunchKernelGGL(prio_chunk_sums_kernel, dim3(n_chunks), dim3(256), 0, s, w, sums);
    }
    hipLaunchKernelGGL(prio_columns_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, rb, w, (const uint64_t*)sums,
                       n_chunks, (const char**)cols, B, versions);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- a column's priority
__device__ __forceinline__ uint32_t quantize(float p) {
    if (!(p < 32768.f)) return kQMax;  // NaN, Inf, >= 32768
    const uint32_t q = (uint32_t)rintf(p * 65536.f);
    return q < 1u ? 1u : q;
}

// One lane per column; the loads of one t are contiguous over the wave, the tensors being (T, B).
// The sum runs over t ascending. A NaN difference makes sum and maximum NaN. Reads 8 T B bytes.
__device__ __forceinline__ float td_priority(const float* __restrict__ vs, const float* __restrict__ values, int T, int B,
                                             int b, float eta) {
    float sum = 0.f, mx = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t i = (size_t)t * B + b;
        const float d = fabsf(vs[i] - values[i]);
        sum += d;
        mx = (d > mx || d != d) ? d : mx;
    }
    return eta * mx + (1.f - eta) * (sum / (float)T);
}

__global__ __launch_bounds__(256) void prio_from_td_kernel(const float* __restrict__ vs, const float* __restrict__ values,
                                                           int T, int B, float eta, uint32_t* __restrict__ q_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    q_out[b] = quantize(td_priority(vs, values, T, B, b, eta));
}

// The table holds p^alpha (fi_weights.h); launched for alpha != 1 only. powf(NaN, 0) is 1, so NaN is
// taken out first.
__global__ __launch_bounds__(256) void prio_from_td_alpha_kernel(const float* __restrict__ vs,
                                                                 const float* __restrict__ values, int T, int B, float eta,
                                                                 float alpha, uint32_t* __restrict__ q_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float p = td_priority(vs, values, T, B, b, eta);
    q_out[b] = p != p ? kQMax : quantize(powf(p, alpha));
}

// alpha == 1: fi_prio.h's kernel, as before fi_weights.h
static int prio_from_td_launch(const float* vs, const float* values, int T, int B, float eta, uint32_t* q_out,
                               hipStream_t s, float alpha = 1.f) {
    FI_REQUIRE(vs && values && q_out, "prio_from_td: null argument");
    FI_REQUIRE(T >= 1 && B >= 1, "prio_from_td: T = " + std::to_string(T) + ", B = " + std::to_string(B) + " must be >= 1");
    FI_REQUIRE(eta >= 0.f && eta <= 1.f, "prio_from_td: eta " + std::to_string(eta) + " outside [0, 1]");
    FI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "prio_from_td: alpha " + std::to_string(alpha) + " outside [0, 1]");
    const dim3 grid((unsigned)((B + 255) / 256));
    if (alpha == 1.f) hipLaunchKernelGGL(prio_from_td_kernel, grid, dim3(256), 0, s, vs, values, T, B, eta, q_out);
    else hipLaunchKernelGGL(prio_from_td_alpha_kernel, grid, dim3(256), 0, s, vs, values, T, B, eta, alpha, q_out);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- the refresh
// Two launches, so every 0 is stored before the first maximum: a slot that several columns name
// ends as the largest of their priorities (all >= 1) whatever the order, and the old value is gone.
__global__ __launch_bounds__(256) void prio_clear_kernel(uint32_t* __restrict__ table, uint32_t C,
                                                         const uint64_t* __restrict__ entries, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) table[(uint32_t)(entries[b] % (uint64_t)C)] = 0u;
}

__global__ __launch_bounds__(256) void prio_max_kernel(uint32_t* __restrict__ table, uint32_t C,
                                                       const uint64_t* __restrict__ entries,
                                                       const uint32_t* __restrict__ q, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) atomicMax(table + (uint32_t)(entries[b] % (uint64_t)C), q[b]);
}

static int prio_scatter_launch(uint32_t* table, int64_t C, const uint64_t* entries, const uint32_t* q, int B,
                               hipStream_t s) {
    FI_REQUIRE(table && entries && q, "prio_scatter: null argument");
    FI_REQUIRE(C >= 1 && C <= 0x7fffffff, "prio_scatter: capacity " + std::to_string(C) + " outside 1 .. 2^31-1");
    FI_REQUIRE(B >= 1, "prio_scatter: B = " + std::to_string(B) + " < 1");
    FI_REQUIRE((uintptr_t)entries % 8 == 0 && (uintptr_t)table % 4 == 0 && (uintptr_t)q % 4 == 0,
               "prio_scatter: entries must be 8-byte, table and q_cols 4-byte aligned");
    const dim3 grid((unsigned)((B + 255) / 256));
    hipLaunchKernelGGL(prio_clear_kernel, grid, dim3(256), 0, s, table, (uint32_t)C, entries, B);
    hipLaunchKernelGGL(prio_max_kernel, grid, dim3(256), 0, s, table, (uint32_t)C, entries, q, B);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- the step's ingest
struct PrioBatch {
    RingBatch rb;
    uint32_t* table;
    uint64_t* sums;
    uint64_t fill_first, fill_count;
    uint32_t q_init;
    float beta;
    float* is_w;  // nullable: the step's importance weights (fi_weights.h); null: none are computed
};

// what a learner's prioritised step from a ring enqueues as its ingest (learner.cpp:
// learner_step_columns): the q_init fill, then the draw, the importance weights where the step has
// any, then the gathering ingest
static int learner_prio_ingest(const void* ctx, const BatchTensors& to) {
    const PrioBatch& pb = *(const PrioBatch*)ctx;
    FI_TRY(prio_init_launch(pb.table, pb.rb.C, pb.fill_first, pb.fill_count, pb.q_init, to.stream));
    FI_TRY(prio_columns_launch(pb.rb, pb.table, pb.sums, to.cols, to.B, to.versions, to.stream));
    if (pb.is_w)
        FI_TRY(prio_is_weights_launch(pb.rb.entries_out, to.B, pb.rb.n_fresh, pb.table, pb.rb.C, pb.rb.lo, pb.rb.n_valid,
                                      pb.sums, pb.beta, pb.is_w, to.stream));
    return gather_ingest(to);
}

// the host form of quantize() for init_priority (rintf: ties to even in the default rounding mode)
static uint32_t quantize_host(float p) {
    if (!(p < 32768.f)) return kQMax;
    const uint32_t q = (uint32_t)rintf(p * 65536.f);
    return q < 1u ? 1u : q;
}

}  // namespace fi

using namespace fi;

static uint64_t ring_lo(const fi_ring* r) { return r->head > (uint64_t)r->C ? r->head - (uint64_t)r->C : 0; }

// ------------------------------------------------------------------ enable / info
extern "C" int fi_prio_enable(fi_ring* r, float eta, float init_priority) {
    FI_REQUIRE(r, "prio_enable: null ring");
    if (r->prio_on) return fail(FI_ERR_STATE, "prio_enable: priorities are enabled already");
    FI_REQUIRE(eta >= 0.f && eta <= 1.f, "prio_enable: eta " + std::to_string(eta) + " outside [0, 1]");
    FI_REQUIRE(std::isfinite(init_priority) && init_priority >= 0.f,
               "prio_enable: init_priority " + std::to_string(init_priority) + " is negative or not finite");
    FI_REQUIRE(r->C <= kPrioMaxCapacity, "prio_enable: capacity " + std::to_string(r->C) +
                                             " above 2^20 = 1048576, the largest prioritised ring");
    FI_HIP_CHECK(hipSetDevice(r->dev));
    const size_t bytes = 4 * (size_t)r->C, ws = 8 * (size_t)kMaxChunks;
    uint32_t* table = nullptr;
    uint64_t* sums = nullptr;
    FI_TRY(dev_alloc((void**)&table, bytes, "prio_enable: the priorities of " + std::to_string(r->C) + " slots"));
    if (dev_alloc((void**)&sums, ws, "prio_enable: the chunk sums") != FI_OK) {
        (void)hipFree(table);
        return FI_ERR_OOM;
    }
    hipError_t e = hipSuccess;
    hipEvent_t done = nullptr;
    if ((e = hipEventCreateWithFlags(&done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipMemsetAsync(table, 0, bytes, r->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(r->stream)) != hipSuccess) {
        if (done) (void)hipEventDestroy(done);
        (void)hipFree(sums);
        (void)hipFree(table);
        return fail(FI_ERR_HIP, std::string("prio_enable: ") + hipGetErrorString(e));
    }
    r->prio = table;
    r->prio_sums = sums;
    r->prio_done = done;
    r->eta = eta;
    r->q_init = quantize_host(init_priority);
    r->prio_hi = ring_lo(r);
    r->prio_on = true;
    return FI_OK;
}

extern "C" int fi_prio_info(const fi_ring* r, fi_prio_state* out) {
    FI_REQUIRE(r && out, "prio_info: null argument");
    *out = fi_prio_state{};
    if (!r->prio_on) return FI_OK;
    *out = fi_prio_state{1u, r->eta, r->q_init, 0u, r->prio_hi, 4 * (uint64_t)r->C};
    return FI_OK;
}

// ------------------------------------------------------------------ read / set
// the checks both share; waits for the last refresh
static int prio_span(fi_ring* r, uint64_t first, int32_t n, const void* host, const std::string& nm) {
    FI_REQUIRE(r && host, nm + ": null argument");
    if (!r->prio_on) return fail(FI_ERR_STATE, nm + ": priorities are not enabled (fi_prio_enable)");
    const uint64_t lo = ring_lo(r);
    FI_REQUIRE(n >= 1 && first >= lo && first + (uint64_t)n <= r->tail,
               nm + ": entries " + std::to_string(first) + " .. " + std::to_string(first + (uint64_t)(n < 0 ? 0 : n)) +
                   " outside the replayable [" + std::to_string(lo) + ", " + std::to_string(r->tail) + ")");
    FI_HIP_CHECK(hipSetDevice(r->dev));
    if (r->have_prio_done) FI_HIP_CHECK(hipEventSynchronize(r->prio_done));
    return FI_OK;
}

// m table values from entry `first` on, host <-> device, in at most two pieces around the wrap
static int prio_copy(fi_ring* r, uint64_t first, uint64_t m, uint32_t* host, bool to_host) {
    const uint64_t C = (uint64_t)r->C, s0 = first % C, n0 = m < C - s0 ? m : C - s0;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    if (to_host) {
        if (n0) FI_HIP_CHECK(hipMemcpyAsync(host, r->prio + s0, 4 * n0, kind, r->stream));
        if (m > n0) FI_HIP_CHECK(hipMemcpyAsync(host + n0, r->prio, 4 * (m - n0), kind, r->stream));
    } else {
        if (n0) FI_HIP_CHECK(hipMemcpyAsync(r->prio + s0, host, 4 * n0, kind, r->stream));
        if (m > n0) FI_HIP_CHECK(hipMemcpyAsync(r->prio, host + n0, 4 * (m - n0), kind, r->stream));
    }
    FI_HIP_CHECK(hipStreamSynchronize(r->stream));
    return FI_OK;
}

extern "C" int fi_prio_read(fi_ring* r, uint64_t first_entry, int32_t n, uint32_t* dst) {
    FI_TRY(prio_span(r, first_entry, n, dst, "prio_read"));
    const uint64_t end = first_entry + (uint64_t)n;
    const uint64_t m = r->prio_hi > first_entry ? (r->prio_hi < end ? r->prio_hi : end) - first_entry : 0;
    if (m) FI_TRY(prio_copy(r, first_entry, m, dst, true));
    for (uint64_t i = m; i < (uint64_t)n; ++i) dst[i] = r->q_init;
    return FI_OK;
}

extern "C" int fi_prio_set(fi_ring* r, uint64_t first_entry, int32_t n, const uint32_t* src) {
    FI_TRY(prio_span(r, first_entry, n, src, "prio_set"));
    for (int32_t i = 0; i < n; ++i)
        FI_REQUIRE(src[i] >= 1u && src[i] <= kQMax, "prio_set: value " + std::to_string(src[i]) + " at index " +
                                                        std::to_string(i) + " outside 1 .. 2^31-1 = 2147483647");
    // the fill a prioritised step would make, up to tail only: prio_hi never passes an unread entry
    const uint64_t lo = ring_lo(r), f0 = r->prio_hi > lo ? r->prio_hi : lo;
    if (r->tail > f0) {
        FI_TRY(prio_init_launch(r->prio, r->C, f0, r->tail - f0, r->q_init, r->stream));
        r->prio_hi = r->tail;
    }
    return prio_copy(r, first_entry, (uint64_t)n, const_cast<uint32_t*>(src), false);
}

// ------------------------------------------------------------------ the learner steps from a ring
static int step_prio(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out, bool wait, const char* who) {
    const std::string nm = who;
    LearnerInfo li{};
    PrioBatch pb{};
    FI_TRY(ring_step_check(l, r, n_fresh, nm, &li, &pb.rb));
    if (!r->prio_on) return fail(FI_ERR_STATE, nm + ": priorities are not enabled (fi_prio_enable)");
    FI_REQUIRE(!r->prio_owner || r->prio_owner == l,
               nm + ": a second learner handle: this ring's priorities belong to the learner that took its first "
                    "prioritised step");
    if (r->beta > 0.f && li.column_weights)
        return fail(FI_ERR_STATE, nm + ": beta = " + std::to_string(r->beta) + " and the learner has column weights set: "
                                       "one source of weights per step (fi_learner_clear_column_weights, or beta = 0)");
    void *vs = nullptr, *values = nullptr;
    size_t vs_bytes = 0, values_bytes = 0;
    FI_TRY(fi_learner_tensor(l, "vs", &vs, &vs_bytes));
    FI_TRY(fi_learner_tensor(l, "values", &values, &values_bytes));
    FI_REQUIRE(vs_bytes == 4 * (size_t)li.T * li.B && values_bytes == 4 * (size_t)(li.T + 1) * li.B,
               nm + ": vs / values do not have the shapes (T, B) / (T + 1, B)");
    FI_TRY(ring_step_entries(r, li.B, nm));
    if (r->prio_q_cap < li.B) {
        // behind the last refresh, which read it
        if (r->prio_q) FI_HIP_CHECK(hipEventSynchronize(r->prio_done));
        FI_TRY(dev_grow(&r->prio_q, &r->prio_q_cap, li.B, nm + ": the column priorities"));
    }
    // importance weights: with beta == 0 or no replayed column nothing is computed or launched
    const bool weighted = r->beta > 0.f && n_fresh < li.B;
    if (weighted && r->is_w_cap < li.B) {
        if (r->is_w) {
            FI_HIP_CHECK(hipEventSynchronize(r->prio_done));  // behind the last step that read it
            r->is_w_valid = false;
        }
        FI_TRY(dev_grow(&r->is_w, &r->is_w_cap, li.B, nm + ": the importance weights"));
    }
    pb.beta = r->beta;
    pb.is_w = weighted ? r->is_w : nullptr;
    pb.rb.entries_out = r->last;
    pb.table = r->prio;
    pb.sums = r->prio_sums;
    pb.q_init = r->q_init;
    const uint64_t filled = pb.rb.tail + (uint64_t)n_fresh;
    pb.fill_first = r->prio_hi > pb.rb.lo ? r->prio_hi : pb.rb.lo;
    pb.fill_count = filled > pb.fill_first ? filled - pb.fill_first : 0;
    const int rc = learner_step_columns(l, r->have_pushed ? r->pushed : nullptr, learner_prio_ingest, &pb, out, wait, who,
                                        pb.is_w, scale_columns_launch);
    // after any other status the counters stay and nothing is refreshed; a fill that was enqueued
    // wrote q_init to entries at or above prio_hi only, which read as q_init anyway
    if (!step_taken(rc)) {
        if (weighted) r->is_w_valid = false;  // the weights buffer may have been rewritten
        return rc;
    }
    r->is_w_valid = weighted;
    if (filled > r->prio_hi) r->prio_hi = filled;
    r->prio_owner = l;
    return finish_taken(rc, [&]() -> int {
        // the refresh, behind the step on the learner's stream: r->last was written by the draw in
        // front of it on the same stream
        hipStream_t s = (hipStream_t)fi_learner_stream(l);
        FI_TRY(prio_from_td_launch((const float*)vs, (const float*)values, li.T, li.B, r->eta, r->prio_q, s, r->alpha));
        FI_TRY(prio_scatter_launch(r->prio, r->C, r->last, r->prio_q, li.B, s));
        FI_HIP_CHECK(hipEventRecord(r->prio_done, s));
        r->have_prio_done = true;
        return ring_step_taken(l, r, n_fresh, li.B);
    });
}

extern "C" int fi_learner_step_ring_prioritized(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out) {
    return step_prio(l, r, n_fresh, out, true, "step_ring_prioritized");
}

extern "C" int fi_learner_step_ring_prioritized_async(fi_learner* l, fi_ring* r, int32_t n_fresh) {
    return step_prio(l, r, n_fresh, nullptr, false, "step_ring_prioritized_async");
}

// ------------------------------------------------------------------ standalone kernels
extern "C" int fi_prio_from_td(const float* vs, const float* values, int32_t T, int32_t B, float eta, uint32_t* q_out,
                               void* stream) {
    return prio_from_td_launch(vs, values, T, B, eta, q_out, (hipStream_t)stream);
}

extern "C" int fi_prio_from_td_alpha(const float* vs, const float* values, int32_t T, int32_t B, float eta, float alpha,
                                     uint32_t* q_out, void* stream) {
    return prio_from_td_launch(vs, values, T, B, eta, q_out, (hipStream_t)stream, alpha);
}

extern "C" int fi_prio_scatter(uint32_t* table, int64_t capacity, const uint64_t* entries, const uint32_t* q_cols,
                               int32_t B, void* stream) {
    return prio_scatter_launch(table, capacity, entries, q_cols, B, (hipStream_t)stream);
}

extern "C" int fi_prio_fill_columns(const void** cols_dev, uint64_t* entries_out_dev, void* versions_dev, const void* base,
                                    size_t entry_bytes, int64_t capacity, int32_t B, int32_t n_fresh, uint64_t tail,
                                    uint64_t lo, uint64_t n_valid, const uint32_t* table, void* chunk_ws, uint64_t seed,
                                    uint64_t draw, void* stream) {
    FI_REQUIRE(capacity >= 1 && capacity <= kPrioMaxCapacity,
               "prio_fill_columns: capacity " + std::to_string(capacity) + " outside 1 .. 2^20 = 1048576");
    const RingBatch rb{(const char*)base, entry_bytes, (uint32_t)capacity, n_fresh, tail, lo, n_valid, seed, draw,
                       entries_out_dev};
    return prio_columns_launch(rb, table, (uint64_t*)chunk_ws, cols_dev, B, (uint32_t*)versions_dev, (hipStream_t)stream);
}
