// The zoom ladder of a BBI file (bigWig, bigBed), once, for bigwig_kernels.hip and bigbed_kernels.hip: ten levels of windows of
// R_k = R_0 * 4^k bases per record, numbered in record coordinates.  Level 0 comes from the format's own kernel; here level l + 1
// is reduced from level l four windows at a time, the windows with a covered base are counted per tile of 256 and (after the
// caller's scan of the tiles) written as 32-byte records in (class, level) segment order, with one block-table row per 1024
// records.  Every (class, level) segment of the window space starts at a multiple of 256 windows, so the scanned tile counts at
// the segment starts are the segment boundaries.
// A format brings, next to its window type Win (fields start, end, valid; valid 0: no covered base; Win() is the empty window):
//   * bbi_join(a, b): the summary of a and b, every base of b above every base of a;
//   * a functor from a record to its first base, for the window numbering of the reduction;
//   * a functor from a window to the second 16 bytes of its record (min, max, sum, sum of squares as float32 bits).
// Integers only: a format that converts to floating point does so in its own translation unit.  Each translation unit gets its own
// copy (internal linkage), as with scan.h.
#pragma once
#include "dgrp_common.h"
#include "scan.h"
#include <vector>

namespace {

#define BBI_LEVELS DGRP_TRACK_ZOOM_LEVELS
#define BBI_ZOOM_BLOCK 1024              // zoom records of a block

struct bbi_levels {
    int64_t R[BBI_LEVELS];               // window width in bases
    int64_t W[BBI_LEVELS];               // windows of all records
    int64_t seg[BBI_LEVELS + 1];         // where the level's windows start in a class's window space (multiples of 256); [10]: its size
};

// windows of width R that record r = [start, start + len) touches (h_start NULL: every record starts at 0)
static inline int64_t bbi_windows(const int64_t *h_start, const int64_t *h_len, int64_t r, int64_t R)
{
    const int64_t s = h_start ? h_start[r] : 0;
    return (s + h_len[r] - 1) / R - s / R + 1;
}

// the levels of windows of R0 * 4^k bases over the records; false: 2^31 or more tiles of 256 windows in ncls classes
static bool bbi_levels_of(int64_t R0, int ncls, int64_t nrec, const int64_t *h_start, const int64_t *h_len, bbi_levels *Z)
{
    Z->seg[0] = 0;
    for (int k = 0; k < BBI_LEVELS; ++k) {
        Z->R[k] = R0 << (2 * k);
        Z->W[k] = 0;
        for (int64_t r = 0; r < nrec; ++r) Z->W[k] += bbi_windows(h_start, h_len, r, Z->R[k]);
        Z->seg[k + 1] = Z->seg[k] + dgrp_align_up(Z->W[k] > 0 ? Z->W[k] : 1, 256);
    }
    return Z->seg[BBI_LEVELS] / 256 * ncls < (1ll << 31);
}

// windows in front of every record, level by level: [BBI_LEVELS][nrec + 1]
static std::vector<int64_t> bbi_wpref(const bbi_levels &Z, int64_t nrec, const int64_t *h_start, const int64_t *h_len)
{
    std::vector<int64_t> wpref((size_t)(nrec + 1) * BBI_LEVELS, 0);
    for (int k = 0; k < BBI_LEVELS; ++k) {
        int64_t *wp = wpref.data() + (size_t)k * (size_t)(nrec + 1);
        for (int64_t r = 0; r < nrec; ++r) wp[r + 1] = wp[r] + bbi_windows(h_start, h_len, r, Z.R[k]);
    }
    return wpref;
}

// level l >= 1 from level l - 1, four windows at a time; grid: the level's tiles of every class
template <class Win, class Start>
__global__ void __launch_bounds__(256) bbi_reduce_kernel(Start start, const int64_t *__restrict__ wpref_all, int64_t nrec, bbi_levels Z, int l,
                                                         Win *__restrict__ win)
{
    const int64_t Wpad = Z.seg[l + 1] - Z.seg[l], bpc = Wpad / 256;
    const int64_t k = blockIdx.x / bpc, i = ((int64_t)blockIdx.x % bpc) * 256 + threadIdx.x;
    const int64_t *wp = wpref_all + (int64_t)l * (nrec + 1), *wc = wp - (nrec + 1);
    Win w = Win();
    if (i < Z.W[l]) {
        const int64_t r = dgrp_record_of(wp, nrec, i);
        const int64_t off = start(r);
        const int64_t wi = off / Z.R[l] + (i - wp[r]);                   // the window's number in the record's coordinates
        const int64_t c0 = off / Z.R[l - 1], nc = wc[r + 1] - wc[r];     // the record's first window and windows one level down
        const Win *child = win + k * Z.seg[BBI_LEVELS] + Z.seg[l - 1] + wc[r];
        for (int64_t c = 4 * wi; c < 4 * wi + 4; ++c)
            if (c >= c0 && c < c0 + nc) w = bbi_join(w, child[c - c0]);
    }
    win[k * Z.seg[BBI_LEVELS] + Z.seg[l] + i] = w;
}

// windows with a covered base per tile of 256 windows (the window space of all classes)
template <class Win>
__global__ void __launch_bounds__(256) bbi_count_kernel(const Win *__restrict__ win, uint64_t *__restrict__ tilecount)
{
    __shared__ uint64_t lds[4];
    uint64_t s = win[(int64_t)blockIdx.x * 256 + threadIdx.x].valid != 0;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tilecount[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// One workgroup.  Per (class, level) segment s = k * 10 + l: the records and the blocks in front of it, segb [2][nseg + 1] (also
// copied to the host).  COVERED (256 lanes; 64 without): *covered = the covered bases of class 0, summed over its top level.
template <class Win, bool COVERED>
__global__ void __launch_bounds__(COVERED ? 256 : 64) bbi_bounds_kernel(const Win *__restrict__ win, const uint64_t *__restrict__ tileoff,
                                                                        const uint64_t *__restrict__ grand, bbi_levels Z, int ncls,
                                                                        uint64_t *__restrict__ segb, uint64_t *__restrict__ covered)
{
    if constexpr (COVERED) {
        __shared__ uint64_t lds[4];
        uint64_t c = 0;
        for (int64_t i = threadIdx.x; i < Z.W[BBI_LEVELS - 1]; i += 256) c += win[Z.seg[BBI_LEVELS - 1] + i].valid;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) *covered = lds[0] + lds[1] + lds[2] + lds[3];
    }
    if (threadIdx.x != 0) return;
    const int nseg = ncls * BBI_LEVELS;
    const int64_t tpc = Z.seg[BBI_LEVELS] / 256;
    uint64_t blocks = 0;
    for (int s = 0; s <= nseg; ++s) {
        const uint64_t at = s < nseg ? tileoff[(int64_t)(s / BBI_LEVELS) * tpc + Z.seg[s % BBI_LEVELS] / 256] : *grand;
        segb[s] = at;
        if (s > 0) blocks += (at - segb[s - 1] + BBI_ZOOM_BLOCK - 1) / BBI_ZOOM_BLOCK;
        segb[nseg + 1 + s] = blocks;
    }
}

// the zoom records (32 bytes, two 16-byte stores) back to back in segment order, and the block table
template <class Win, class Tail>
__global__ void __launch_bounds__(256) bbi_write_kernel(const Win *__restrict__ win, const int64_t *__restrict__ wpref_all, int64_t nrec,
                                                        bbi_levels Z, Tail tail, const uint64_t *__restrict__ tileoff,
                                                        const uint64_t *__restrict__ segb, int ncls, uint32_t chrom0,
                                                        uint4 *__restrict__ out, dgrp_track_zoom_block *__restrict__ table)
{
    __shared__ uint64_t lds[4];
    const int64_t tpc = Z.seg[BBI_LEVELS] / 256;
    const int64_t k = blockIdx.x / tpc, tc = (int64_t)blockIdx.x % tpc;
    int l = 0;
    while (l + 1 < BBI_LEVELS && Z.seg[l + 1] <= tc * 256) ++l;
    const int64_t i = tc * 256 - Z.seg[l] + threadIdx.x;                  // the window in its level
    const Win w = win[(int64_t)blockIdx.x * 256 + threadIdx.x];
    const uint64_t ex = block_exclusive_scan(w.valid != 0, nullptr, lds);
    if (w.valid == 0) return;
    const int nseg = ncls * BBI_LEVELS, s = (int)k * BBI_LEVELS + l;
    const uint64_t at = tileoff[blockIdx.x] + ex, j = at - segb[s], n = segb[s + 1] - segb[s];
    const int64_t r = dgrp_record_of(wpref_all + (int64_t)l * (nrec + 1), nrec, i);
    uint4 a;
    a.x = chrom0 + (uint32_t)r; a.y = w.start; a.z = w.end; a.w = w.valid;
    out[2 * at] = a;
    out[2 * at + 1] = tail(w);
    dgrp_track_zoom_block *row = table + segb[nseg + 1 + s] + j / BBI_ZOOM_BLOCK;
    if (j % BBI_ZOOM_BLOCK == 0) {
        const uint64_t left = n - j, count = left < BBI_ZOOM_BLOCK ? left : BBI_ZOOM_BLOCK;
        row->off = (int64_t)(32 * at);
        row->bytes = (int64_t)(32 * count);
        row->cls = (int32_t)k;
        row->level = l;
        row->rec0 = (int32_t)r;
        row->start = w.start;
    }
    if (j % BBI_ZOOM_BLOCK == BBI_ZOOM_BLOCK - 1 || j == n - 1) {
        row->rec1 = (int32_t)r;
        row->end = w.end;
    }
}

}   // namespace
