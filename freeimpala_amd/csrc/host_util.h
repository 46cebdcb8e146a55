// host_util.h -- the host-side plumbing the handles of libfi_learner.so share: device allocations,
// the checks of a caller's device pointers, the exception boundary of a C entry point, the device of
// a create call, the dynamic-LDS limit of a kernel and the tail of a step that took its batch.
// Internal, header-only (inline functions and templates), so any translation unit uses it without
// depending on another one: learner.cpp still names nothing of actor.hip, ring.hip or the others. A
// second copy of host plumbing goes here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <exception>
#include <string>

#include "fi_common.h"

namespace fi {

// ---------------------------------------------------------------- device allocations
// hipMalloc; a refusal leaves *p null and HIP's sticky last error cleared, so that the next
// FI_HIP_CHECK(hipGetLastError()) behind a kernel launch on this thread does not report it
inline int dev_alloc(void** p, size_t bytes, const std::string& what) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return FI_OK;
    *p = nullptr;
    (void)hipGetLastError();
    return fail(FI_ERR_OOM, what + ": hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
}

// A grow-on-demand buffer of *cap elements: at least `need` afterwards. The old block is freed, so
// the caller has waited for whatever still reads it.
template <typename T>
inline int dev_grow(T** p, int* cap, int need, const std::string& what) {
    if (*cap >= need) return FI_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    FI_TRY(dev_alloc((void**)p, sizeof(T) * (size_t)need, what));
    *cap = need;
    return FI_OK;
}

// ---------------------------------------------------------------- dynamic LDS above 64 KB
// Kernel `fn` takes up to `most` bytes of dynamic LDS, more than the default limit: the limit is
// raised once per device. `raised` is the caller's flag for that kernel, a bit per device id (handles
// on different devices launch from their own threads).
inline int raise_lds(const void* fn, std::atomic<uint64_t>& raised, size_t most) {
    int dev = 0;
    FI_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? (uint64_t)1 << dev : 0;
    if (!bit || !(raised.load(std::memory_order_acquire) & bit)) {
        FI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        raised.fetch_or(bit, std::memory_order_acq_rel);
    }
    return FI_OK;
}

// ---------------------------------------------------------------- a caller's device pointers
// The one place that asks HIP about a pointer: p is device memory of device `dev` (the `owner`'s, in
// the message) and lies in an allocation; *have: the bytes from p to that allocation's end.
inline int dev_bytes_behind(int dev, const void* p, const std::string& what, const char* owner, size_t* have) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != dev) {
        (void)hipGetLastError();
        return fail(FI_ERR_INVALID, what + " is not device memory of the " + owner + "'s device " + std::to_string(dev));
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FI_ERR_INVALID, what + " lies in no device allocation");
    }
    *have = size - (size_t)((const char*)p - (const char*)base);
    return FI_OK;
}

// `bytes` from p on are device memory of device `dev` inside one allocation, and p is `align`-byte
// aligned. FI_ERR_INVALID with `what` (call: argument) in the message
inline int check_dev_span(int dev, const void* p, size_t bytes, size_t align, const std::string& what) {
    FI_REQUIRE(p, what + " is null");
    FI_REQUIRE((uintptr_t)p % align == 0, what + " must be " + std::to_string(align) + "-byte aligned");
    size_t have = 0;
    FI_TRY(dev_bytes_behind(dev, p, what, "handle", &have));
    FI_REQUIRE(bytes <= have, what + ": the allocation ends " + std::to_string(have) + " bytes behind the pointer, " +
                                  std::to_string(bytes) + " are read");
    return FI_OK;
}

// n entries of entry_bytes, `stride` apart, from `entries` on: the stride covers an entry, both are
// 16-byte aligned, and the span (n - 1) * stride + entry_bytes -- the last entry need not be followed
// by a whole stride -- is device memory of `dev` inside one allocation. `need` words what the stride
// is compared with; the stride and the alignment are refused before HIP is asked anything.
inline int check_entry_span(int dev, const void* entries, size_t stride, int n, size_t entry_bytes, const std::string& nm,
                            const std::string& need, const char* owner = "handle") {
    FI_REQUIRE(stride >= entry_bytes, nm + ": entry_stride " + std::to_string(stride) + " < " + need);
    FI_REQUIRE(stride % 16 == 0 && (uintptr_t)entries % 16 == 0,
               nm + ": entries_dev and entry_stride must be 16-byte aligned");
    size_t have = 0;
    FI_TRY(dev_bytes_behind(dev, entries, nm + ": entries_dev", owner, &have));
    const size_t span = (size_t)(n - 1) * stride + entry_bytes;
    FI_REQUIRE(span <= have, nm + ": the allocation ends " + std::to_string(have) + " bytes behind entries_dev, " +
                                 std::to_string(n) + " entries need " + std::to_string(span));
    return FI_OK;
}

// an Atari handle reads device entries in the planes format only (the stacked one is a host format)
inline int require_dev_entries(bool ok, const std::string& nm) {
    FI_REQUIRE(ok, nm + ": an Atari handle reads device entries in the planes format only "
                        "(fi_learner_set_record_format(FI_RECORDS_PLANES) first)");
    return FI_OK;
}

// ---------------------------------------------------------------- C entry points
// fn() behind the exception boundary of a C entry point: a std::exception becomes `code`
template <typename F>
inline int guarded(const char* who, int code, F&& fn) {
    try {
        return fn();
    } catch (const std::exception& e) {
        return fail(code, std::string(who) + ": " + e.what());
    }
}

// the device of a create call, made current
inline int use_device(int device, const std::string& who) {
    int ndev = 0;
    FI_HIP_CHECK(hipGetDeviceCount(&ndev));
    FI_REQUIRE(device >= 0 && device < ndev, who + ": no such HIP device");
    FI_HIP_CHECK(hipSetDevice(device));
    return FI_OK;
}

// ---------------------------------------------------------------- the tail of a step
// The batch counts as taken when the step ran -- FI_ERR_NONFINITE: it ran and skipped its update --
// or, asynchronously, was enqueued. Any other status: refused or broken before or at the enqueue.
inline bool step_taken(int rc) { return rc == FI_OK || rc == FI_ERR_NONFINITE; }

// What follows a taken step: hand_back() returns the buffers (and may set the thread's error on its
// way), then the step's status is reported again with the step's message, copied before that.
template <typename F>
inline int finish_taken(int rc, F&& hand_back) {
    std::string why;
    if (rc != FI_OK) why = fi_last_error();
    FI_TRY(hand_back());
    return rc == FI_OK ? FI_OK : fail(rc, why);
}

}  // namespace fi
