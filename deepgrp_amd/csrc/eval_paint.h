// Rows painted onto flat per-base buffers, shared by `evaluate` (eval_kernels.hip) and the training truth (train_prep_kernels.hip):
// the clipping of a row to its record, the two binary searches and the length-balanced paint kernel.  Each translation unit gets its
// own copy (internal linkage), as with scan.h.
#pragma once
#include "dgrp_common.h"

namespace {

#define EVAL_SLICE 8192           // positions per workgroup: 256 lanes x 32, lane-interleaved (a wave's stores are 64 adjacent bytes)

// row j's span on the record: [cs, cs + cl) of its bases (cl = 0 when the row misses the record)
__device__ __forceinline__ void eval_clip(const dgrp_segment &q, int64_t origin, int64_t len, int64_t &cs, int64_t &cl)
{
    int64_t a = q.start - origin, e = q.end - origin;
    a = a < 0 ? 0 : (a > len ? len : a);
    e = e < 0 ? 0 : (e > len ? len : e);
    cs = a;
    cl = e > a ? e - a : 0;
}

// largest j in [lo, hi) with ex[j] <= p, given ex[lo] <= p < ex[hi]
__device__ __forceinline__ int64_t eval_row_of(const uint64_t *__restrict__ ex, int64_t lo, int64_t hi, uint64_t p)
{
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ex[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// ex[0..n] = exclusive scan of the rows' lengths in this pass (ex[n] = total): every position of the slice gets `label`
__global__ void __launch_bounds__(256) eval_paint_kernel(int8_t *__restrict__ labels, const uint64_t *__restrict__ ex,
                                                         const int64_t *__restrict__ dst, int64_t n, int label)
{
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 >= s1) return;
    int64_t j = eval_row_of(ex, 0, n, p0);
    uint64_t jst = ex[j], jend = ex[j + 1];
    for (uint64_t p = p0; p < s1; p += 256) {
        while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
        labels[dst[j] + (int64_t)(p - jst)] = (int8_t)label;
    }
}

}   // namespace
