// Line finding of the text parsers (dgrp_rm_parse*: annotation_kernels.hip; dgrp_rows_parse: rows_parse_kernels.hip): the tile and
// chunk sizes, the chunk scan that finds the line feeds and the bytes a parser does not decide, and the run starts of the kept rows.
// Each translation unit gets its own copy of these small kernels (internal linkage), as with scan.h.
#pragma once
#include "scan.h"

namespace {

#define RM_CHUNK 128                     // bytes per lane
#define RM_TILE (256 * RM_CHUNK)         // bytes per workgroup (DGRP_RM_TILE_BYTES)
#define RM_HEAD 256                      // workspace head: [0] the not-plain flag

static_assert(RM_TILE == DGRP_RM_TILE_BYTES, "the header states the tile");

__host__ __device__ __forceinline__ bool rm_eol(uint8_t c) { return c == '\n' || c == '\r'; }
__host__ __device__ __forceinline__ bool rm_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// The lane's chunk: mask of its line feeds (bit k of lo / hi: byte c0 + k / c0 + 64 + k) and whether a byte of it makes the file not
// plain: outside 0x20..0x7e, tab and line feed, or a carriage return that no line feed follows.
__host__ __device__ __forceinline__ void rm_scan_chunk(const uint8_t *__restrict__ t, int64_t c0, int64_t n, bool aligned, uint64_t &lo,
                                              uint64_t &hi, bool &bad)
{
    lo = hi = 0;
    bool cr = false;                                                         // the byte before was a carriage return
    const int64_t c1 = c0 + RM_CHUNK < n ? c0 + RM_CHUNK : n;
#pragma unroll
    for (int g = 0; g < RM_CHUNK / 16; ++g) {
        const int64_t p0 = c0 + 16 * g;
        if (p0 >= c1) break;
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
        const int valid = c1 - p0 < 16 ? (int)(c1 - p0) : 16;
        if (valid == 16 && aligned) {
            const uint4 v = *reinterpret_cast<const uint4 *>(t + p0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            for (int j = 0; j < valid; ++j) w[j >> 2] |= (uint32_t)t[p0 + j] << (8 * (j & 3));
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < valid) {
                const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                const bool lf = c == '\n';
                if (cr && !lf) bad = true;
                cr = c == '\r';
                if (!((c >= 0x20u && c <= 0x7eu) || c == '\t' || lf || cr)) bad = true;
                if (lf) {
                    if (g < 4) lo |= 1ull << (16 * g + j); else hi |= 1ull << (16 * (g - 4) + j);
                }
            }
        }
    }
    if (cr && (c1 >= n || t[c1] != '\n')) bad = true;
}

__device__ __forceinline__ bool rm_span_differs(const uint8_t *__restrict__ t, int64_t pa, int32_t la, int64_t pb, int32_t lb)
{
    if (la != lb) return true;
    if (pa == pb) return false;
    for (int32_t j = 0; j < la; ++j)
        if (t[pa + j] != t[pb + j]) return true;
    return false;
}

// flag[i] = 1 where row i opens a run: its name differs from the name of row i - 1 (with pos2 / len2: its second span does, too)
__global__ void __launch_bounds__(256) rm_run_flag_kernel(const uint8_t *__restrict__ t, const int64_t *__restrict__ name_pos,
                                                          const int32_t *__restrict__ name_len, const int64_t *__restrict__ pos2,
                                                          const int32_t *__restrict__ len2, int64_t rows, uint64_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    bool opens = i == 0 || rm_span_differs(t, name_pos[i], name_len[i], name_pos[i - 1], name_len[i - 1]);
    if (!opens && pos2) opens = rm_span_differs(t, pos2[i], len2[i], pos2[i - 1], len2[i - 1]);
    flag[i] = opens ? 1ull : 0ull;
}

// run[i] = the exclusive scan of the flags, run[rows] their sum: row i opens run run[i] where the scan moves behind it
__global__ void __launch_bounds__(256) rm_run_first_kernel(const uint64_t *__restrict__ run, int64_t rows, int64_t *__restrict__ first)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows && run[i + 1] != run[i]) first[run[i]] = i;
}

static inline int64_t rm_tiles_of(int64_t n) { return (n + RM_TILE - 1) / RM_TILE; }

}   // namespace
