// ring.hip -- the device entry ring (include/fi_ring.h, gfx950): the reference's SharedBuffer in
// device memory, between recording actors and a learner on the same device.
//   * ring_push_kernel: n source entries, `stride` apart, into the slots (first + i) mod C
//   * ring_columns_kernel: the batch rule, one lane per column -- the column table the gathering
//     ingest (gather.hip) reads its entries through, the chosen entry indices, and the version
//     block's neutral state. Every number arrives by value as a kernel argument, so an
//     asynchronous step needs no host buffer to outlive it.
// The handle keeps head / tail / draw on the host, which issues every operation. As in rollout.hip
// and gather.hip: 16-byte accesses contiguous over the wave, loads that name the global address
// space, ordinary vector stores, no LDS, no atomics.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "fi_common.h"
#include "fi_ring.h"
#include "host_util.h"
#include "ingest_kernels.h"
#include "kernels.h"
#include "ring_handle.h"

namespace fi {

namespace {
constexpr int kChunkPieces = 1024;  // 16-byte pieces a workgroup copies: 256 lanes x 4, 16 KiB
constexpr int64_t kMaxCapacity = 0x7fffffff;
// ld16 (a 16-byte load that names the global address space): ingest_kernels.h
}  // namespace

// ---------------------------------------------------------------- the push's copy
// A workgroup owns one source entry and one run of 1,024 of its 16-byte pieces: the entry index, the
// slot (first_slot + i, less C once past the end: n <= C, so the run wraps at most once inside a
// launch) and both base addresses come from blockIdx and stay on the scalar unit. A lane has its
// four loads in flight before its first store; each of them is contiguous over the wave. n *
// chunks workgroups; HBM traffic 2 * n * entry_bytes.
__global__ __launch_bounds__(256) void ring_push_kernel(char* __restrict__ ring, uint32_t pieces, uint32_t chunks,
                                                        uint32_t C, uint32_t first_slot,
                                                        const char* __restrict__ src, size_t stride) {
    const uint32_t i = blockIdx.x / chunks, chunk = blockIdx.x - i * chunks;
    uint32_t slot = first_slot + i;  // first_slot < C and i < n <= C < 2^31: no overflow
    if (slot >= C) slot -= C;
    const char* __restrict__ s = src + (size_t)i * stride;
    uint4* __restrict__ d = (uint4*)(ring + (size_t)slot * pieces * 16);
    const uint32_t p0 = chunk * kChunkPieces + threadIdx.x;
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = make_uint4(0u, 0u, 0u, 0u);
        if (p0 + 256 * k < pieces) v[k] = ld16(s + (size_t)(p0 + 256 * k) * 16);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + 256 * k < pieces) d[p0 + 256 * k] = v[k];
}

int ring_push_launch(void* ring, size_t entry_bytes, int64_t capacity, uint64_t first_entry, const void* src,
                     size_t stride, int n, hipStream_t s) {
    FI_REQUIRE(ring && src, "ring_copy_entries: null argument");
    FI_REQUIRE(entry_bytes >= 16 && entry_bytes % 16 == 0 && entry_bytes / 16 <= 0x7fffffffu,
               "ring_copy_entries: entry_bytes " + std::to_string(entry_bytes) + " is not a multiple of 16 (>= 16)");
    FI_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity,
               "ring_copy_entries: capacity " + std::to_string(capacity) + " outside 1 .. 2^31-1");
    FI_REQUIRE(n >= 1 && n <= capacity, "ring_copy_entries: n = " + std::to_string(n) + " outside 1 .. capacity " +
                                            std::to_string(capacity));
    FI_REQUIRE((uintptr_t)ring % 16 == 0 && (uintptr_t)src % 16 == 0 && stride % 16 == 0,
               "ring_copy_entries: dst_base, src and src_stride must be 16-byte aligned");
    FI_REQUIRE(stride >= entry_bytes, "ring_copy_entries: src_stride " + std::to_string(stride) + " < entry_bytes " +
                                          std::to_string(entry_bytes));
    const uint32_t pieces = (uint32_t)(entry_bytes / 16);
    const uint32_t chunks = (pieces + kChunkPieces - 1) / kChunkPieces;
    FI_REQUIRE((uint64_t)n * chunks <= 0x7fffffffull, "ring_copy_entries: " + std::to_string(n) + " entries of " +
                                                          std::to_string(entry_bytes) + " bytes pass the grid");
    hipLaunchKernelGGL(ring_push_kernel, dim3((unsigned)n * chunks), dim3(256), 0, s, (char*)ring, pieces, chunks,
                       (uint32_t)capacity, (uint32_t)(first_entry % (uint64_t)capacity), (const char*)src, stride);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// ---------------------------------------------------------------- the batch rule
// the numbers of one batch, taken before the call (include/fi_ring.h): RingBatch, ring_handle.h
// Column c < n_fresh: entry tail + c. Column c >= n_fresh: entry lo + ((x * n_valid) >> 32), x the
// first word of philox4(seed, draw * B + c, ST_REPLAY); n_valid <= C < 2^31, so the product stays
// inside 64 bits. Thread 0 also puts the version block into its neutral state, as
// fill_columns_kernel does.
__global__ __launch_bounds__(256) void ring_columns_kernel(RingBatch rb, const char** __restrict__ cols, int B,
                                                           uint32_t* __restrict__ versions) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0 && versions) {
        versions[0] = 0xffffffffu;
        versions[1] = versions[2] = versions[3] = 0u;
    }
    if (c >= B) return;
    uint64_t e = rb.tail + (uint64_t)c;
    if (c >= rb.n_fresh) {
        const uint32_t x = philox4(rb.seed, rb.draw * (uint64_t)B + (uint64_t)c, ST_REPLAY).x;
        e = rb.lo + (((uint64_t)x * rb.n_valid) >> 32);
    }
    const uint32_t slot = (uint32_t)(e % (uint64_t)rb.C);
    cols[c] = rb.base + (size_t)slot * rb.entry_bytes;
    if (rb.entries_out) rb.entries_out[c] = e;
}

int ring_columns_launch(const RingBatch& rb, const void** cols, int B, uint32_t* versions, hipStream_t s) {
    FI_REQUIRE(cols && rb.base && B >= 1, "ring_fill_columns: bad arguments");
    FI_REQUIRE((uintptr_t)cols % 8 == 0 && (uintptr_t)rb.entries_out % 8 == 0 && (uintptr_t)versions % 8 == 0,
               "ring_fill_columns: cols, entries_out and versions must be 8-byte aligned");
    FI_REQUIRE(rb.C >= 1 && rb.C <= (uint32_t)kMaxCapacity, "ring_fill_columns: capacity outside 1 .. 2^31-1");
    FI_REQUIRE(rb.n_fresh >= 0 && rb.n_fresh <= B, "ring_fill_columns: n_fresh " + std::to_string(rb.n_fresh) +
                                                       " outside 0 .. B = " + std::to_string(B));
    FI_REQUIRE(rb.lo + rb.n_valid == rb.tail && rb.n_valid <= rb.C,
               "ring_fill_columns: lo " + std::to_string(rb.lo) + " + n_valid " + std::to_string(rb.n_valid) +
                   " must be tail " + std::to_string(rb.tail) + " and n_valid <= capacity");
    FI_REQUIRE(rb.n_fresh == B || rb.n_valid >= 1, "ring_fill_columns: replayed columns need n_valid >= 1");
    hipLaunchKernelGGL(ring_columns_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, rb, (const char**)cols, B,
                       versions);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

// what a learner's step from a ring enqueues as its ingest (learner.cpp: learner_step_columns)
static int learner_ring_ingest(const void* ctx, const BatchTensors& to) {
    FI_TRY(ring_columns_launch(*(const RingBatch*)ctx, to.cols, to.B, to.versions, to.stream));
    return gather_ingest(to);
}

}  // namespace fi

using namespace fi;

// ------------------------------------------------------------------ the handle (struct fi_ring: ring_handle.h)
static void destroy(fi_ring* r) {
    if (!r) return;
    (void)hipSetDevice(r->dev);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->have_prio_done) (void)hipEventSynchronize(r->prio_done);  // behind the last refresh (fi_prio.h)
    if (r->is_w) (void)hipFree(r->is_w);  // fi_weights.h
    if (r->prio_q) (void)hipFree(r->prio_q);
    if (r->prio_sums) (void)hipFree(r->prio_sums);
    if (r->prio) (void)hipFree(r->prio);
    if (r->prio_done) (void)hipEventDestroy(r->prio_done);
    if (r->last) (void)hipFree(r->last);
    if (r->base) (void)hipFree(r->base);
    if (r->pushed) (void)hipEventDestroy(r->pushed);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

static int create(int32_t device, size_t entry_bytes, int64_t capacity, uint64_t seed, fi_ring** out) {
    FI_REQUIRE(out, "ring_create: null argument");
    *out = nullptr;
    FI_REQUIRE(entry_bytes >= 16 && entry_bytes % 16 == 0 && entry_bytes / 16 <= 0x7fffffffu,
               "ring_create: entry_bytes " + std::to_string(entry_bytes) + " is not a multiple of 16 (>= 16)");
    FI_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity,
               "ring_create: capacity " + std::to_string(capacity) + " outside 1 .. 2^31-1");
    int ndev = 0;
    FI_HIP_CHECK(hipGetDeviceCount(&ndev));
    FI_REQUIRE(device >= 0 && device < ndev, "ring_create: device " + std::to_string(device) + " of " + std::to_string(ndev));
    FI_HIP_CHECK(hipSetDevice(device));
    fi_ring* r = new fi_ring();
    std::unique_ptr<fi_ring, void (*)(fi_ring*)> guard(r, destroy);
    r->dev = device;
    r->entry = entry_bytes;
    r->C = capacity;
    r->seed = seed;
    const size_t bytes = (size_t)capacity * entry_bytes;
    FI_REQUIRE(bytes / entry_bytes == (size_t)capacity, "ring_create: capacity * entry_bytes passes 2^64");
    FI_TRY(dev_alloc((void**)&r->base, bytes, "ring_create: " + std::to_string(capacity) + " slots"));
    FI_HIP_CHECK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    FI_HIP_CHECK(hipEventCreateWithFlags(&r->pushed, hipEventDisableTiming));
    FI_HIP_CHECK(hipMemsetAsync(r->base, 0, bytes, r->stream));
    FI_HIP_CHECK(hipStreamSynchronize(r->stream));
    *out = guard.release();
    return FI_OK;
}

extern "C" int fi_ring_create(int32_t device, size_t entry_bytes, int64_t capacity, uint64_t seed, fi_ring** out) {
    return guarded("ring_create", FI_ERR_OOM, [&] { return create(device, entry_bytes, capacity, seed, out); });
}

extern "C" void fi_ring_destroy(fi_ring* r) { destroy(r); }

extern "C" int fi_ring_info(const fi_ring* r, fi_ring_state* out) {
    FI_REQUIRE(r && out, "ring_info: null argument");
    *out = fi_ring_state{(uint64_t)r->C, (uint64_t)r->entry, r->head, r->tail, r->draw, r->seed};
    return FI_OK;
}

extern "C" int fi_ring_seed(fi_ring* r, uint64_t seed, uint64_t draw) {
    FI_REQUIRE(r, "ring_seed: null ring");
    r->seed = seed;
    r->draw = draw;
    return FI_OK;
}

// ------------------------------------------------------------------ push
static int push(fi_ring* r, const void* entries, size_t stride, int32_t n, void* ready, const char* who) {
    const std::string nm = who;
    FI_REQUIRE(r && entries, nm + ": null argument");
    FI_REQUIRE(n >= 1, nm + ": n = " + std::to_string(n) + " < 1");
    FI_HIP_CHECK(hipSetDevice(r->dev));
    // the checks fi_learner_step_entries_dev makes on its buffer
    FI_TRY(check_entry_span(r->dev, entries, stride, n, r->entry, nm, "entry_bytes " + std::to_string(r->entry), "ring"));
    const uint64_t unread = r->head - r->tail, room = (uint64_t)r->C - unread;
    if ((uint64_t)n > room)
        return fail(FI_ERR_STATE, nm + ": full: " + std::to_string(n) + " entries, capacity " + std::to_string(r->C) +
                                      " - " + std::to_string(unread) + " unread leaves " + std::to_string(room));
    if (ready) FI_HIP_CHECK(hipStreamWaitEvent(r->stream, (hipEvent_t)ready, 0));
    FI_TRY(ring_push_launch(r->base, r->entry, r->C, r->head, entries, stride, n, r->stream));
    FI_HIP_CHECK(hipEventRecord(r->pushed, r->stream));
    r->have_pushed = true;
    r->head += (uint64_t)n;
    return FI_OK;
}

extern "C" int fi_ring_push(fi_ring* r, const void* entries_dev, size_t entry_stride, int32_t n, void* ready_event) {
    return push(r, entries_dev, entry_stride, n, ready_event, "ring_push");
}

extern "C" void* fi_ring_pushed_event(fi_ring* r) { return r && r->have_pushed ? (void*)r->pushed : nullptr; }
extern "C" void* fi_ring_stream(fi_ring* r) { return r ? (void*)r->stream : nullptr; }

extern "C" int fi_ring_push_rollout(fi_ring* r, fi_actor* a) {
    FI_REQUIRE(r && a, "ring_push_rollout: null argument");
    ActorInfo ai{};
    FI_TRY(actor_info(a, &ai));
    FI_REQUIRE(ai.dev == r->dev, "ring_push_rollout: the actor's device " + std::to_string(ai.dev) +
                                     " != the ring's " + std::to_string(r->dev));
    const size_t eb = fi_rollout_entry_bytes(a);  // 0: not recording, which the acquire reports
    FI_REQUIRE(eb == 0 || eb == r->entry, "ring_push_rollout: the actor's entry bytes " + std::to_string(eb) +
                                              " != the ring's entry_bytes " + std::to_string(r->entry));
    const void* entries = nullptr;
    size_t stride = 0;
    void* ready = nullptr;
    FI_TRY(fi_rollout_acquire(a, &entries, &stride, &ready));
    // a refusal (full, above all) leaves the unroll waiting: nothing was enqueued
    FI_TRY(push(r, entries, stride, ai.N, ready, "ring_push_rollout"));
    return fi_rollout_release(a, r->pushed);
}

// ------------------------------------------------------------------ read back
extern "C" int fi_ring_read_slots(fi_ring* r, int64_t first_slot, int32_t n, void* host_dst, size_t bytes) {
    FI_REQUIRE(r && host_dst, "ring_read_slots: null argument");
    FI_REQUIRE(n >= 1 && first_slot >= 0 && first_slot + n <= r->C,
               "ring_read_slots: slots " + std::to_string(first_slot) + " .. " + std::to_string(first_slot + n) +
                   " outside the capacity " + std::to_string(r->C));
    FI_REQUIRE(bytes == (size_t)n * r->entry, "ring_read_slots: bytes != n * entry_bytes = " +
                                                  std::to_string((size_t)n * r->entry));
    FI_HIP_CHECK(hipSetDevice(r->dev));
    FI_HIP_CHECK(hipMemcpyAsync(host_dst, r->base + (size_t)first_slot * r->entry, bytes, hipMemcpyDeviceToHost, r->stream));
    FI_HIP_CHECK(hipStreamSynchronize(r->stream));
    return FI_OK;
}

extern "C" int fi_ring_last_entries(fi_ring* r, uint64_t* dst, int32_t n) {
    FI_REQUIRE(r && dst, "ring_last_entries: null argument");
    if (r->last_n == 0) return fail(FI_ERR_STATE, "ring_last_entries: no ring step yet (fi_learner_step_ring)");
    FI_REQUIRE(n == r->last_n, "ring_last_entries: n = " + std::to_string(n) + " != the last step's batch " +
                                   std::to_string(r->last_n));
    FI_HIP_CHECK(hipSetDevice(r->dev));
    // the ring's stream waits for the step's consumed event, which lies behind the columns kernel
    FI_HIP_CHECK(hipMemcpyAsync(dst, r->last, 8 * (size_t)n, hipMemcpyDeviceToHost, r->stream));
    FI_HIP_CHECK(hipStreamSynchronize(r->stream));
    return FI_OK;
}

// ------------------------------------------------------------------ the learner steps from a ring
// It lives here, not in learner.cpp, because it holds both handles (as fi_learner_step_rollout in
// actor.hip): every refusal is made here, before learner.cpp enqueues anything.
int fi::ring_step_check(fi_learner* l, fi_ring* r, int32_t n_fresh, const std::string& nm, LearnerInfo* li_out,
                        RingBatch* rb) {
    FI_REQUIRE(l && r, nm + ": null argument");
    LearnerInfo li{};
    FI_TRY(learner_info(l, &li));
    FI_REQUIRE(li.dev == r->dev, nm + ": the ring's device " + std::to_string(r->dev) + " != the learner's " +
                                     std::to_string(li.dev));
    FI_TRY(require_dev_entries(li.dev_entries_ok, nm));
    const size_t need = fi_learner_entry_bytes(l);
    FI_REQUIRE(r->entry >= need, nm + ": the ring's entry_bytes " + std::to_string(r->entry) + " < " +
                                     std::to_string(need) + " = fi_learner_entry_bytes()");
    FI_REQUIRE(n_fresh >= 0 && n_fresh <= li.B, nm + ": n_fresh " + std::to_string(n_fresh) + " outside 0 .. batch " +
                                                    std::to_string(li.B));
    const uint64_t unread = r->head - r->tail;
    const uint64_t lo = r->head > (uint64_t)r->C ? r->head - (uint64_t)r->C : 0;
    const uint64_t n_valid = r->tail - lo;
    if ((uint64_t)n_fresh > unread)
        return fail(FI_ERR_STATE, nm + ": " + std::to_string(unread) + " entries unread, n_fresh = " +
                                      std::to_string(n_fresh));
    if (n_fresh < li.B && n_valid == 0)
        return fail(FI_ERR_STATE, nm + ": nothing to replay: " + std::to_string(li.B - n_fresh) +
                                      " columns of the batch " + std::to_string(li.B) +
                                      " are replayed and no entry was read yet (tail " + std::to_string(r->tail) + ")");
    *li_out = li;
    *rb = RingBatch{r->base, r->entry, (uint32_t)r->C, n_fresh, r->tail, lo, n_valid, r->seed, r->draw, nullptr};
    return FI_OK;
}

int fi::ring_step_entries(fi_ring* r, int B, const std::string& nm) {
    FI_HIP_CHECK(hipSetDevice(r->dev));
    if (r->last_cap >= B) return FI_OK;
    if (r->last) {
        FI_HIP_CHECK(hipStreamSynchronize(r->stream));  // behind the last step's columns kernel
        r->last_n = 0;
    }
    return dev_grow(&r->last, &r->last_cap, B, nm + ": the entry indices");
}

int fi::ring_step_taken(fi_learner* l, fi_ring* r, int32_t n_fresh, int B) {
    // a later push may overwrite the slots this batch names: it goes behind the ingest
    FI_HIP_CHECK(hipStreamWaitEvent(r->stream, (hipEvent_t)fi_learner_entries_consumed_event(l), 0));
    r->tail += (uint64_t)n_fresh;
    r->draw += 1;
    r->last_n = B;
    return FI_OK;
}

static int step_ring(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out, bool wait, const char* who) {
    const std::string nm = who;
    LearnerInfo li{};
    RingBatch rb{};
    FI_TRY(ring_step_check(l, r, n_fresh, nm, &li, &rb));
    FI_TRY(ring_step_entries(r, li.B, nm));
    rb.entries_out = r->last;
    const int rc = learner_step_columns(l, r->have_pushed ? r->pushed : nullptr, learner_ring_ingest, &rb, out, wait, who);
    // as fi_learner_step_rollouts; after any other status the counters stay
    if (!step_taken(rc)) return rc;
    return finish_taken(rc, [&] { return ring_step_taken(l, r, n_fresh, li.B); });
}

extern "C" int fi_learner_step_ring(fi_learner* l, fi_ring* r, int32_t n_fresh, fi_step_stats* out) {
    return step_ring(l, r, n_fresh, out, true, "step_ring");
}

extern "C" int fi_learner_step_ring_async(fi_learner* l, fi_ring* r, int32_t n_fresh) {
    return step_ring(l, r, n_fresh, nullptr, false, "step_ring_async");
}

// ------------------------------------------------------------------ standalone kernels
extern "C" int fi_ring_copy_entries(void* dst_base, size_t entry_bytes, int64_t capacity, uint64_t first_entry,
                                    const void* src, size_t src_stride, int32_t n, void* stream) {
    return ring_push_launch(dst_base, entry_bytes, capacity, first_entry, src, src_stride, n, (hipStream_t)stream);
}

extern "C" int fi_ring_fill_columns(const void** cols_dev, uint64_t* entries_out_dev, void* versions_dev, const void* base,
                                    size_t entry_bytes, int64_t capacity, int32_t B, int32_t n_fresh, uint64_t tail,
                                    uint64_t lo, uint64_t n_valid, uint64_t seed, uint64_t draw, void* stream) {
    FI_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity,
               "ring_fill_columns: capacity " + std::to_string(capacity) + " outside 1 .. 2^31-1");
    const RingBatch rb{(const char*)base, entry_bytes, (uint32_t)capacity, n_fresh, tail, lo, n_valid, seed, draw,
                       entries_out_dev};
    return ring_columns_launch(rb, cols_dev, B, (uint32_t*)versions_dev, (hipStream_t)stream);
}
