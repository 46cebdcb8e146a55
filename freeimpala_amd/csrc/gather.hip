// gather.hip -- the ingest kernels of ingest_kernels.h with one level of indirection (gfx950): batch
// column b's entry is read at cols[b], a table of B base addresses in device memory (the Table
// locator), so the columns of one learner batch may come from several buffers (several recording
// actors, include/fi_gather.h) with their own strides, in any order. Outputs and their layouts are
// the contiguous ingest's (misc.hip). Here also:
//   * fill_columns_kernel: the table from <= 64 segments {base, stride, first column, count} that
//     arrive by value as the kernel argument (no host buffer has to outlive an asynchronous step)
//   * the version block: the min / max / sum of the records' flags words (the parameter version
//     the acting policy held), which only this path's scalar kernel folds
// Record schemas: records.h.
#include <algorithm>

#include "fi_common.h"
#include "ingest_kernels.h"
#include "kernels.h"

namespace fi {

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

// the header tensors of T records, rec_stride apart, through the table
static void gather_header(int mu_off, int act_off, size_t rec_stride, const BatchTensors& to) {
    const Table at{(const char* const*)to.cols};
    launch_ingest_vec(at, to.T, to.B, to.A, mu_off, rec_stride, to.mu, to.stream);
    launch_ingest_scalar<Table, true>(at, to.T, to.B, to.A, act_off, rec_stride, to.act, to.rew, to.disc, to.bad,
                                      to.versions, to.stream);
}

int gather_records_launch(const BatchTensors& to) {
    const int T = to.T, B = to.B;
    FI_REQUIRE(to.cols && T >= 1 && B >= 1 && to.A >= 1 && to.A <= kMlpMaxActions && to.D <= kMlpMaxObs,
               "gather_records: bad shape");
    FI_REQUIRE(!to.versions || (uintptr_t)to.versions % 8 == 0, "gather_records: the version block must be 8-byte aligned");
    const Table at{(const char* const*)to.cols};
    if (to.obs) {
        FI_REQUIRE(to.D >= 1, "gather_records: D");
        launch_ingest_vec(at, T + 1, B, to.D, kMlpRecObs, kMlpRecBytes, to.obs, to.stream);
    }
    if (to.mu) launch_ingest_vec(at, T, B, to.A, kMlpRecMu, kMlpRecBytes, to.mu, to.stream);
    if (to.act && to.rew && to.disc)
        launch_ingest_scalar<Table, true>(at, T, B, to.A, kMlpRecAct, kMlpRecBytes, to.act, to.rew, to.disc, to.bad,
                                          to.versions, to.stream);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int gather_atari_planes_launch(const BatchTensors& to) {
    const int T = to.T, B = to.B, A = to.A;
    FI_REQUIRE(to.cols && to.frames && to.mu && to.act && to.rew && to.disc, "gather_atari_planes: null argument");
    FI_REQUIRE(T >= 1 && B >= 1 && A >= 1, "gather_atari_planes: bad shape");
    FI_REQUIRE(A <= kPlaneMaxActions, "gather_atari_planes: the plane record's header holds mu[18]: A = " +
                                          std::to_string(A) + " > 18");
    FI_REQUIRE((size_t)(T + 1) * (size_t)B <= (size_t)0x7fffffff / kPlaneRuns, "gather_atari_planes: too many frames");
    FI_REQUIRE((uintptr_t)to.cols % 8 == 0 && (uintptr_t)to.frames % 16 == 0,
               "gather_atari_planes: the column table must be 8-byte, frames 16-byte aligned");
    FI_REQUIRE(!to.versions || (uintptr_t)to.versions % 8 == 0,
               "gather_atari_planes: the version block must be 8-byte aligned");
    launch_ingest_planes(Table{(const char* const*)to.cols}, T, B, to.frames, to.stream);
    gather_header(kPlaneRecMu, kPlaneRecAct, kPlaneRecBytes, to);
    FI_HIP_CHECK(hipGetLastError());
    return FI_OK;
}

int gather_ingest(const BatchTensors& to) {
    return to.arch == FI_ARCH_MLP ? gather_records_launch(to) : gather_atari_planes_launch(to);
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
static int learner_gather_ingest(const void* tab, const BatchTensors& to) {
    FI_TRY(fill_columns_launch(*(const SegTable*)tab, to.cols, to.B, to.versions, to.stream));
    return gather_ingest(to);
}

// the standalone entry points: the caller's table (read only) and tensors, the version block reset
static int gather_standalone(int arch, const void* const* cols, int T, int B, int A, int D, float* obs, uint8_t* frames,
                             float* mu, int32_t* act, float* rew, float* disc, int* bad, void* versions, void* stream) {
    const BatchTensors to{arch, T, B, A, D, obs, frames, mu, act, rew, disc, bad, const_cast<const void**>(cols),
                          (uint32_t*)versions, (hipStream_t)stream};
    FI_TRY(versions_reset(versions, to.stream));
    return gather_ingest(to);
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
    return fi::gather_standalone(FI_ARCH_ATARI, cols_dev, T, B, A, 0, nullptr, frames, mu, actions, rewards, discounts,
                                 bad_dev, versions_dev, stream);
}

extern "C" int fi_ingest_records_gather(const void* const* cols_dev, int T, int B, int A, int D, float* obs, float* mu,
                                        int32_t* actions, float* rewards, float* discounts, int* bad_dev,
                                        void* versions_dev, void* stream) {
    return fi::gather_standalone(FI_ARCH_MLP, cols_dev, T, B, A, D, obs, nullptr, mu, actions, rewards, discounts,
                                 bad_dev, versions_dev, stream);
}
