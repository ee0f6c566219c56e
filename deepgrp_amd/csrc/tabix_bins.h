// The binning scheme of a tabix index (deepgrp_amd/tabix.py states the format): min_shift 14, depth 5, so coordinates end at or
// below 2^29.  Shared by the index of the tracks (track_kernels.hip) and of the scored BED (bed_kernels.hip).
#pragma once
#include "dgrp_common.h"

#define TABIX_MIN_SHIFT 14
#define TABIX_MAX_END (1ll << 29)        // the largest coordinate of a tabix index

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

}  // namespace
