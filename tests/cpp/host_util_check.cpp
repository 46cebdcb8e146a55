// host_util_check.cpp -- the internal host helpers of freeimpala_amd/csrc/host_util.h on their own,
// linked against libfi_learner.so for fi::fail / fi_last_error. No kernel is launched. Prints OK,
// exits non-zero on the first failed check.
//
//   host_util_check cpu   what needs no device: the refusals made before HIP is asked, a host pointer,
//                         the exception boundary, the step tail (passes with a GPU too)
//   host_util_check gpu   the span checks against one 4,096-byte allocation, dev_alloc, dev_grow
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "host_util.h"

#define CHECK(c)                                                                                      \
    do {                                                                                              \
        if (!(c)) {                                                                                   \
            std::fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, \
                         fi_last_error());                                                            \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

static bool says(const char* part) { return std::strstr(fi_last_error(), part) != nullptr; }

static int run_cpu() {
    // What hipGetLastError() answers with nothing behind it: hipSuccess with a device. Without any, the
    // runtime fails to initialise inside every call, that one included, and it answers
    // hipErrorNoDevice each time: there "cleared" can only mean "what it said before anything ran".
    const hipError_t quiet = hipGetLastError();
    int ndev = 0;
    const bool no_device = hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0;
    CHECK(quiet == (no_device ? hipErrorNoDevice : hipSuccess));
    // check_dev_span: null, misaligned, host memory
    CHECK(fi::check_dev_span(0, nullptr, 16, 16, "call: p") == FI_ERR_INVALID && says("call: p is null"));
    alignas(16) static char local[64];
    CHECK(fi::check_dev_span(0, local + 8, 16, 16, "call: p") == FI_ERR_INVALID && says("call: p must be 16-byte aligned"));
    void* host = std::malloc(4096);
    CHECK(host);
    CHECK(fi::check_dev_span(0, host, 16, 1, "call: p") == FI_ERR_INVALID &&
          says("call: p is not device memory of the handle's device 0"));
    CHECK(hipGetLastError() == quiet);
    std::free(host);

    // check_entry_span: the stride and the alignment are refused before HIP is asked anything, so
    // a pointer that no allocation holds gets this far
    const void* nowhere = (const void*)(uintptr_t)0x1000;
    CHECK(fi::check_entry_span(0, nowhere, 32, 4, 48, "call", "48 = the entry") == FI_ERR_INVALID &&
          says("call: entry_stride 32 < 48 = the entry"));
    CHECK(fi::check_entry_span(0, nowhere, 56, 4, 48, "call", "48") == FI_ERR_INVALID &&
          says("call: entries_dev and entry_stride must be 16-byte aligned"));
    CHECK(fi::check_entry_span(0, (const char*)nowhere + 8, 64, 4, 48, "call", "48") == FI_ERR_INVALID &&
          says("16-byte aligned"));
    CHECK(hipGetLastError() == quiet);

    // guarded: the lambda's own value, and an exception as the given code
    CHECK(fi::guarded("who", FI_ERR_STATE, [] { return 42; }) == 42);
    CHECK(fi::guarded("who", FI_ERR_OOM, []() -> int { throw std::bad_alloc(); }) == FI_ERR_OOM);
    CHECK(std::string(fi_last_error()) == "who: std::bad_alloc");
    CHECK(fi::guarded("who", FI_ERR_STATE, []() -> int { throw std::bad_alloc(); }) == FI_ERR_STATE);

    // the step tail: the step's message survives a hand-back that set and cleared an error
    CHECK(fi::step_taken(FI_OK) && fi::step_taken(FI_ERR_NONFINITE) && !fi::step_taken(FI_ERR_INVALID) &&
          !fi::step_taken(FI_ERR_STATE) && !fi::step_taken(FI_ERR_HIP) && !fi::step_taken(FI_ERR_OOM));
    int rc = fi::fail(FI_ERR_NONFINITE, "step: the gradient norm is not finite");
    bool ran = false;
    rc = fi::finish_taken(rc, [&] {
        ran = true;
        (void)fi::fail(FI_ERR_HIP, "hand-back: something");
        fi::set_error("");
        return (int)FI_OK;
    });
    CHECK(ran && rc == FI_ERR_NONFINITE && std::string(fi_last_error()) == "step: the gradient norm is not finite");
    // a step that was fine stays fine; a hand-back that fails reports itself
    CHECK(fi::finish_taken(FI_OK, [] { return (int)FI_OK; }) == FI_OK);
    (void)fi::fail(FI_ERR_NONFINITE, "step: skipped");
    CHECK(fi::finish_taken(FI_ERR_NONFINITE, [] { return fi::fail(FI_ERR_HIP, "hand-back: broken"); }) == FI_ERR_HIP &&
          says("hand-back: broken"));
    CHECK(fi::require_dev_entries(true, "call") == FI_OK);
    CHECK(fi::require_dev_entries(false, "call") == FI_ERR_INVALID &&
          says("call: an Atari handle reads device entries in the planes format only"));

    // without a device an allocation is refused, and the refusal does not stay behind as HIP's last error
    if (no_device) {
        void* p = (void*)(uintptr_t)1;
        CHECK(fi::dev_alloc(&p, 16, "call") == FI_ERR_OOM && p == nullptr && says("call: hipMalloc(16): "));
        CHECK(hipGetLastError() == quiet);
        CHECK(fi::use_device(0, "call") != FI_OK);
    }
    std::printf("OK cpu\n");
    return 0;
}

static int run_gpu() {
    CHECK(fi::use_device(0, "call") == FI_OK);
    CHECK(fi::use_device(-1, "call") == FI_ERR_INVALID && says("call: no such HIP device"));
    char* blk = nullptr;
    CHECK(fi::dev_alloc((void**)&blk, 4096, "call") == FI_OK && blk);
    // check_dev_span: an exact fit at the end, and one that passes it
    CHECK(fi::check_dev_span(0, blk + 4080, 16, 16, "call: p") == FI_OK);
    CHECK(fi::check_dev_span(0, blk + 4080, 32, 16, "call: p") == FI_ERR_INVALID &&
          says("call: p: the allocation ends 16 bytes behind the pointer, 32 are read"));
    // check_entry_span: the last entry need not be followed by a whole stride
    CHECK(fi::check_entry_span(0, blk, 64, 64, 48, "call", "48") == FI_OK);  // 63 * 64 + 48 = 4,080
    CHECK(fi::check_entry_span(0, blk, 64, 64, 64, "call", "64") == FI_OK);  // 4,096
    CHECK(fi::check_entry_span(0, blk, 64, 65, 48, "call", "48") == FI_ERR_INVALID &&
          says("call: the allocation ends 4096 bytes behind entries_dev, 65 entries need 4144"));
    CHECK(fi::check_entry_span(0, blk + 64, 64, 64, 48, "call", "48") == FI_ERR_INVALID &&
          says("call: the allocation ends 4032 bytes behind entries_dev, 64 entries need 4080"));
    CHECK(fi::check_entry_span(0, blk, 64, 64, 48, "call", "48", "ring") == FI_OK);
    CHECK(hipGetLastError() == hipSuccess);
    // dev_alloc, and dev_grow: a second call with the same need keeps the block
    void* small = nullptr;
    CHECK(fi::dev_alloc(&small, 16, "call") == FI_OK && small);
    uint64_t* buf = nullptr;
    int cap = 0;
    CHECK(fi::dev_grow(&buf, &cap, 8, "call") == FI_OK && buf && cap == 8);
    CHECK(fi::check_dev_span(0, buf, 64, 16, "call: buf") == FI_OK);
    uint64_t* const first = buf;
    CHECK(fi::dev_grow(&buf, &cap, 8, "call") == FI_OK && buf == first && cap == 8);
    CHECK(fi::dev_grow(&buf, &cap, 4, "call") == FI_OK && buf == first && cap == 8);
    CHECK(hipFree(buf) == hipSuccess && hipFree(small) == hipSuccess && hipFree(blk) == hipSuccess);
    std::printf("OK gpu\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cpu") return run_cpu();
    if (mode == "gpu") return run_gpu();
    std::fprintf(stderr, "usage: host_util_check cpu|gpu\n");
    return 2;
}
