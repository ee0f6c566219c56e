// The binning scheme of a tabix index (deepgrp_amd/tabix.py states the format): min_shift 14, depth 5, so coordinates end at or
// below 2^29; and of a CSI index: the same scheme with the depth as an argument, 6 levels below the root reaching 2^32.  Shared by
// the index of the tracks (track_kernels.hip) and of the scored BED (bed_kernels.hip).
#pragma once
#include "dgrp_common.h"

#define TABIX_MIN_SHIFT 14
#define TABIX_MAX_END (1ll << 29)        // the largest coordinate of a tabix index
#define TABIX_DEPTH 5                    // of a .tbi; a .csi of this project has CSI_DEPTH
#define CSI_DEPTH 6

// the largest coordinate of an index of `depth` levels below the root: 2^29 at 5, 2^32 at 6
static inline int64_t tabix_max_end(int depth) { return 1ll << (TABIX_MIN_SHIFT + 3 * depth); }

namespace {

// the bin of [beg, end) (end exclusive, 0 <= beg < end <= TABIX_MAX_END): tabix.reg2bin
__device__ __forceinline__ uint32_t tabix_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// the bin of [beg, end) (0 <= beg < end <= tabix_max_end(depth)) at `depth` levels below the root (uniform; 5 or 6):
// tabix.csi_reg2bin.  Level l starts at bin ((1 << 3l) - 1) / 7 and has shift 14 + 3(depth - l); the search goes from the bottom
// level upwards.  At depth 5 this is tabix_reg2bin.  The largest bin, 37449 + 2^18 - 1, fits 32 bits with room.
__device__ __forceinline__ uint32_t tabix_reg2bin_depth(int64_t beg, int64_t end, int depth)
{
    --end;
    int shift = TABIX_MIN_SHIFT;
    for (int l = depth; l > 0; --l, shift += 3)
        if (beg >> shift == end >> shift) return (uint32_t)((((1ll << 3 * l) - 1) / 7) + (beg >> shift));
    return 0;
}

}  // namespace
