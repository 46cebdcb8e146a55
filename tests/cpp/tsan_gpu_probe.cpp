// tsan_gpu_probe.cpp -- can the ROCm runtime start inside a ThreadSanitizer process here?
//
// ThreadSanitizer fixes the layout of the address space (x86-64): application memory is
// [0, 2 TiB), [0x5500'0000'0000, 0x5a00'0000'0000) and [0x7a00'0000'0000, 2^47); all between
// is shadow, or protected. The ROCm runtime takes the addresses it shares with the GPU from
// plain mmap(NULL, ...) and needs them inside the GPU's virtual address range. On a bare-metal
// MI355X that range is nearly the whole 47 bits and mmap answers from the top, inside TSAN's
// upper application range. Some virtualised GPUs differ: once /dev/kfd is open, the process's
// mappings are placed below 0x5000'0000'0000 and the GPU's range starts at 16 TiB. In a TSAN
// process the only free application memory under that ceiling lies below 2 TiB, outside the
// GPU's range, so hsa_init fails (out of resources) and HIP reports no device -- before any of
// this project's code runs. tests/test_sanitizers.py asks this program first, and skips the
// TSAN run on the GPU where the answer is no.
//
//   exit 0, "tsan-gpu ok devices=N"         the runtime initialised and sees N >= 1 devices
//   exit 3, "tsan-gpu unavailable: <why>"   it did not, and with /dev/kfd open an anonymous page
//                                           lands outside TSAN's upper application ranges
//   exit 1, "tsan-gpu error: <why>"         it did not, for any other reason (a failure)
// Built with -fsanitize=thread by tests/cpp/tsan.mk (build/tsan/tsan_gpu_probe).
#include <hip/hip_runtime_api.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>

int main() {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e == hipSuccess && n > 0) {
        std::printf("tsan-gpu ok devices=%d\n", n);
        return 0;
    }
    const int fd = open("/dev/kfd", O_RDWR | O_CLOEXEC);
    void* p = mmap(nullptr, 4096, PROT_NONE, MAP_ANONYMOUS | MAP_NORESERVE | MAP_PRIVATE, -1, 0);
    const bool low = fd >= 0 && p != MAP_FAILED && (uintptr_t)p < 0x550000000000ull;
    if (low)
        std::printf("tsan-gpu unavailable: the ROCm runtime does not start under ThreadSanitizer on this "
                    "machine (hipGetDeviceCount: %s; with /dev/kfd open, mmap places a page at %p, "
                    "below TSAN's upper application ranges)\n", hipGetErrorString(e), p);
    else
        std::printf("tsan-gpu error: hipGetDeviceCount: %s (%d devices); /dev/kfd %s\n", hipGetErrorString(e), n,
                    fd >= 0 ? "opens" : "does not open");
    if (p != MAP_FAILED) munmap(p, 4096);
    if (fd >= 0) close(fd);
    return low ? 3 : 1;
}
