// interleave.h -- the byte interleave the plane ingest kernels share (misc.hip: ingest_planes_kernel,
// gather.hip: gather_planes_kernel).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fi {

// 4 pixels of channels 0..3 (one dword each) -> 4 NHWC pixels (byte c of a pixel = channel c)
__device__ __forceinline__ uint4 interleave4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    const uint32_t ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);
    const uint32_t cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
    return make_uint4(__builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u),   // a0 b0 c0 d0
                      __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u),   // a1 b1 c1 d1
                      __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u),
                      __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u));
}

}  // namespace fi
