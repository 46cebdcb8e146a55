// work_map.h -- which workgroup does what, as plain functions the host can call too (no HIP
// header needed: tests/test_fc_dgrad_map.py compiles them with the host compiler alone).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FI_HD __host__ __device__
#else
#define FI_HD
#endif

namespace fi {

// XCD-aware bijective remap (guide section 5, "XCD swizzle must be bijective"): blocks
// that share an XCD (same bid % 8) get consecutive logical ids.
FI_HD inline int xcd_remap(int bid, int nblk) {
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// ---------------------------------------------------------------- fc_dgrad_wreg_kernel
// da3[R][3136] is cut into row slots of 64 rows and column slices of 256 columns (13 slices, the
// last one 64 columns wide). Workgroup = (stream, slice): stream j of 19 walks the row slots
// j, j + 19, ... of its slice; wave w of 8 owns the 32 columns 256 slice + 32 w (in the last
// slice only waves 0 and 1 have columns). The 13 workgroups of a stream read the same dh rows at
// about the same pace, so they get consecutive logical ids of xcd_remap: consecutive positions on
// one XCD (whose L2 then serves a dh slot 12 times out of 13), except for the streams that
// straddle the end of an XCD's 30 or 31 workgroups.
constexpr int kDgStreams = 19, kDgSlices = 13, kDgBlocks = kDgStreams * kDgSlices;
constexpr int kDgSlotRows = 64, kDgSliceCols = 256, kDgWaveCols = 32;

struct FcDgradMap {
    int stream, slice;  // row slots stream, stream + kDgStreams, ... < nslots; columns 256 slice ..
    int nslots;         // ceil(rows / 64)
    int xcd, pos;       // where round-robin dispatch puts the block: XCD block % 8, its pos-th there
};

FI_HD inline FcDgradMap fc_dgrad_map(int block, int rows) {
    const int lg = xcd_remap(block, kDgBlocks);
    return FcDgradMap{lg / kDgSlices, lg % kDgSlices, (rows + kDgSlotRows - 1) / kDgSlotRows, block % 8, block / 8};
}

}  // namespace fi
