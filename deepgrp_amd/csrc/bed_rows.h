// What the chains over the scored rows share (bed_kernels.hip: BED and GFF3 text and their tabix pieces; bigbed_kernels.hip: bigBed item blocks
// and coverage zoom records): the envelope of a row's score, its four figures, the decimal writers, the refusals a check kernel
// raises as flag words and the head of the workspace they come back in.  Integers only.  Each translation unit gets its own copy
// (internal linkage), as with scan.h.
#pragma once
#include "dgrp_common.h"

namespace {

#define BED_ONE (1ull << 24)               // q(1.0)
#define BED_MAX_BASES (1ll << 40)          // the envelope of the 64-bit rounding below
#define BED_MAX_ROWS ((1ll << 31) - 256)   // one thread per row, 256 a workgroup

enum { F_BASES, F_NAME, F_RANGE, F_SPAN, F_END, F_RECORDS, F_STARTS, F_OVERLAP, F_LABEL, F_COUNT };
static const char *const FLAG_TEXT[F_COUNT] = {
    "a row has no scored base (bases <= 0)",
    "a row names a record outside the names (by_contig: contig not in 0..nnames-1)",
    "a row's figures lie outside the envelope (bases < 2^40, sum <= bases * 2^24, 0 <= agree <= bases)",
    "a row has start < 0 or start >= end",
    "a row lies outside the records or ends behind its record's end",
    "the records do not ascend with the rows",
    "the starts descend inside a record (tabix needs sorted rows)",
    "a row starts below the end of a row in front of it in its record (bigBed rows ascend and do not overlap)",
    "a row's label lies outside the class names (1..ncnames)",
};

// The four figures, R(num, den, k) = floor((2 k num + den) / (2 den)) of the header without a 128-bit division: with
// sum = a * bases + r (0 <= r < bases), R(sum, bases * 2^24, k) = (2 k a + 2^24 + floor(2 k r / bases)) >> 25, every term below
// 2^64 for k <= 10000, bases < 2^40 and a <= 2^24.
struct bed_figs { uint64_t score, mean, qmin, agree; };

__device__ __forceinline__ bool bed_scored(const dgrp_row_score &sc)
{
    return sc.bases > 0 && sc.bases < BED_MAX_BASES && sc.sum <= ((uint64_t)sc.bases << 24) && sc.agree >= 0 && sc.agree <= sc.bases;
}

__device__ __forceinline__ bed_figs bed_figures(const dgrp_row_score &sc)
{
    const uint64_t bases = (uint64_t)sc.bases, a = sc.sum / bases, r = sc.sum - a * bases;
    bed_figs f;
    f.score = (2000 * a + BED_ONE + 2000 * r / bases) >> 25;
    f.mean = (20000 * a + BED_ONE + 20000 * r / bases) >> 25;
    f.qmin = (20000ull * sc.qmin + BED_ONE) >> 25;
    f.agree = (20000 * (uint64_t)sc.agree + bases) / (2 * bases);
    return f;
}

__device__ __forceinline__ int dec_chars(uint64_t u)
{
    int d = 1;
    while (u >= 10) { u /= 10; ++d; }
    return d;
}

__device__ __forceinline__ int int_chars(long long v)
{
    return v < 0 ? 1 + dec_chars(0ull - (unsigned long long)v) : dec_chars((unsigned long long)v);
}

__device__ __forceinline__ char *put_dec(char *o, uint64_t u)
{
    const int d = dec_chars(u);
    for (int k = d - 1; k >= 0; --k) { o[k] = (char)('0' + u % 10); u /= 10; }
    return o + d;
}

__device__ __forceinline__ char *put_int(char *o, long long v)
{
    if (v < 0) { *o++ = '-'; return put_dec(o, 0ull - (unsigned long long)v); }
    return put_dec(o, (unsigned long long)v);
}

__device__ __forceinline__ char *put_fixed4(char *o, uint64_t v)          // v / 10^4 as "d.dddd"
{
    o = put_dec(o, v / 10000);
    const unsigned f = (unsigned)(v % 10000);
    *o++ = '.';
    *o++ = (char)('0' + f / 1000);
    *o++ = (char)('0' + f / 100 % 10);
    *o++ = (char)('0' + f / 10 % 10);
    *o++ = (char)('0' + f % 10);
    return o;
}

__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t *a, int64_t n, uint64_t x)      // the first index with a[i] >= x
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// header of the workspace: three totals, then the flag words (F_COUNT of them; the head has 256 bytes of the workspace)
struct bed_head { uint64_t bytes, lines, chunks, pad; uint32_t flags[16]; };

static int bed_refusal(const char *who, const bed_head &h)
{
    for (int k = 0; k < F_COUNT; ++k) {
        if (h.flags[k]) {
            dgrp_set_error("%s: %s", who, FLAG_TEXT[k]);
            return DGRP_EINVAL;
        }
    }
    return DGRP_OK;
}

}   // namespace
