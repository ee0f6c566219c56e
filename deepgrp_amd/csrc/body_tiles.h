// Plain record bodies of one device buffer cut into tiles, shared by the kernels that stream over them (mask_kernels.hip,
// twobit_pack_kernels.hip): record r = bytes [off[r], off[r] + len[r]), a tile = BODY_TILE bytes from the 16-byte word in which
// the body starts, one workgroup of 256 lanes with one aligned 16-byte load each.
#pragma once
#include "dgrp_common.h"

namespace {

#define BODY_TILE 4096            // bytes per workgroup: 256 lanes x 16

__device__ __forceinline__ bool body_lineend(uint32_t b) { return b == '\n' || b == '\r'; }

// (the record of tile t is dgrp_record_of(tile0, nrec, t): records without tiles share their tile0 with the next record)

struct body_span {
    int64_t word;                 // 16-byte aligned address (offset in the buffer) of this lane's bytes
    int lo, hi;                   // the lane's bytes inside the record: word + [lo, hi)
};

__device__ __forceinline__ body_span body_lane_span(int64_t off, int64_t len, int64_t k)
{
    body_span s;
    s.word = (off & ~(int64_t)15) + k * BODY_TILE + (int64_t)threadIdx.x * 16;
    const int64_t a = s.word > off ? s.word : off, e = s.word + 16 < off + len ? s.word + 16 : off + len;
    s.lo = (int)(a - s.word);
    s.hi = e > a ? (int)(e - s.word) : s.lo;
    return s;
}

// (bytes outside the record read as line feeds: they are no sequence bytes)
__device__ __forceinline__ void body_load(const uint8_t *__restrict__ raw, const body_span &s, uint8_t *b)
{
    if (s.lo == 0 && s.hi == 16) {
        *(uint4 *)b = *(const uint4 *)(raw + s.word);
    } else {
        for (int j = 0; j < 16; ++j) b[j] = (j >= s.lo && j < s.hi) ? raw[s.word + j] : (uint8_t)'\n';
    }
}

static inline int64_t body_tiles_of(int64_t off, int64_t len)
{
    return len > 0 ? (off + len - (off & ~(int64_t)15) + BODY_TILE - 1) / BODY_TILE : 0;
}

// >= the sum of body_tiles_of over nrec records of total_bytes together
static inline int64_t body_tile_bound(int64_t nrec, int64_t total_bytes)
{
    return total_bytes / BODY_TILE + 2 * nrec + 1;
}

}   // namespace
