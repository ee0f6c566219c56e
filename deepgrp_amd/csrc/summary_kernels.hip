// Repeat content table (predict --summary_dir): per record the sequence positions per (label, kind of byte, case), and per bin of
// `bin` positions the ACGT bases and the positions under every label > 0.  One streaming pass over plain record bodies: the count
// pass of mask_kernels.hip (sequence bytes per body tile, scanned), a row check that leaves the good rows compacted in the
// workspace, a table of where every tile starts (its record, first position, rows and bin: one lane per tile, all searches side by
// side), then one workgroup of 256 lanes per body tile at a time, one aligned 16-byte load per lane.  A lane finds the row of
// its first position by binary search over the tile's rows and walks on from there; its counts go, one add per run of equal
// labels, into an LDS table of C * 10 counters (REP copies of every counter, a lane adds to copy lane mod REP: the 64 lanes of a
// wave that all see "label 0, upper-case A" then hit different banks and not one word).  A workgroup walks `per` consecutive tiles
// and flushes the table into d_counts when the record changes and at its end, with 64-bit integer atomics; bin counts go to
// d_bins with integer atomics too, through LDS where a whole tile lies in one bin.  Integer sums do not depend on their order, so
// the same call gives the same bytes whatever order the workgroups run in.  Bytes and integers only.  See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "body_tiles.h"
#include "scan.h"
#include <vector>

namespace {

#define SUMMARY_CELLS 10              // (kind 0..4) * 2 + (lower case)
#define SUMMARY_LDS_BYTES 16384       // the copies of the counters are sized to this
#define SUMMARY_GRID 2048             // workgroups of a launch (a workgroup walks consecutive tiles: few flushes per record)
#define SUMMARY_MAX_PER (1 << 19)     // tiles per workgroup: 2^19 * 4096 bytes = 2^31 positions, no 32-bit counter can wrap

__global__ void __launch_bounds__(256) summary_count_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ tile0,
                                                            const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                            int64_t nrec, uint64_t *__restrict__ tilecnt)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_rec;
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) s_rec = dgrp_record_of(tile0, nrec, t);
    __syncthreads();
    const int64_t r = s_rec;
    const body_span s = body_lane_span(off[r], len[r], t - tile0[r]);
    alignas(16) uint8_t b[16];
    body_load(raw, s, b);
    uint64_t c = 0;
    for (int j = 0; j < 16; ++j) c += body_lineend(b[j]) ? 0 : 1;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tilecnt[t] = lds[0] + lds[1] + lds[2] + lds[3];
}

// one lane per row (and one behind the last): keep[k] = 1 for a good row.  Bad: a label outside 0..C-1, start < 0, end <= start,
// end beyond the record's sequence, or the next row of the record starting below this row's end.  *bad = smallest bad row index
// (it holds -1 = all ones on entry: an unsigned minimum).
__global__ void __launch_bounds__(256) summary_check_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                            int64_t nrec, const int64_t *__restrict__ tile0,
                                                            const uint64_t *__restrict__ ex, int C, uint64_t *__restrict__ keep,
                                                            unsigned long long *__restrict__ bad)
{
    const int64_t first = row_off[0], nrows = row_off[nrec] - first;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nrows) return;
    if (k == nrows) {
        keep[k] = 0;
        return;
    }
    const int64_t i = first + k;
    const int64_t r = dgrp_record_of(row_off, nrec, i);
    const int64_t seqlen = (int64_t)(ex[tile0[r + 1]] - ex[tile0[r]]);
    const dgrp_segment q = rows[i];
    bool ok = q.label >= 0 && q.label < C && q.start >= 0 && q.end > q.start && q.end <= seqlen;
    if (i + 1 < row_off[r + 1] && rows[i + 1].start < q.end) ok = false;
    keep[k] = ok ? 1 : 0;
    if (!ok) atomicMin(bad, (unsigned long long)i);
}

// the good rows back to back: row first + k goes to crows[kidx[k]] (kidx: the exclusive scan of keep)
__global__ void __launch_bounds__(256) summary_compact_kernel(const dgrp_segment *__restrict__ rows, int64_t first, int64_t nrows,
                                                              const uint64_t *__restrict__ kidx, dgrp_segment *__restrict__ crows)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrows || kidx[k + 1] == kidx[k]) return;
    crows[kidx[k]] = rows[first + k];
}

struct summary_args {
    const uint8_t *raw;
    const int64_t *tile0, *off, *len, *row_off, *bin_off;       // [nrec + 1], [nrec], [nrec], [nrec + 1], [nrec + 1] (bin > 0)
    const uint64_t *ex;                                         // [ntiles + 1]: sequence bytes in front of every tile
    const uint64_t *kidx;                                       // [nrows + 1], NULL without rows
    const dgrp_segment *crows;                                  // the good rows
    int64_t nrec, ntiles, per, bin;
    int C, rep;
    unsigned long long *counts, *bins;
    struct summary_tile *meta;                                  // [ntiles]
};

// what the walk needs to start a tile, found for all tiles at once (one lane per tile: the searches run side by side)
struct summary_tile {
    int64_t rec, p0;              // the tile's record and first sequence position
    int64_t lo, hi;               // its rows among the good rows: the first that ends after p0 up to the first that starts at or after p1
    int64_t binfo;                // (bin of p0) << 1 | (the tile lies in one bin)
};

__global__ void __launch_bounds__(256) summary_tiles_kernel(summary_args a)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.ntiles) return;
    summary_tile m;
    const int64_t r = dgrp_record_of(a.tile0, a.nrec, t);
    const int64_t p0 = (int64_t)(a.ex[t] - a.ex[a.tile0[r]]), p1 = p0 + (int64_t)(a.ex[t + 1] - a.ex[t]);
    m.rec = r; m.p0 = p0; m.lo = m.hi = 0;
    if (a.kidx) {
        const int64_t first = a.row_off[0];
        int64_t x = (int64_t)a.kidx[a.row_off[r] - first], y = (int64_t)a.kidx[a.row_off[r + 1] - first];
        const int64_t end = y;
        while (x < y) {
            const int64_t mid = (x + y) >> 1;
            if (a.crows[mid].end <= p0) x = mid + 1; else y = mid;
        }
        m.lo = x;
        y = end;
        while (x < y) {
            const int64_t mid = (x + y) >> 1;
            if (a.crows[mid].start < p1) x = mid + 1; else y = mid;
        }
        m.hi = x;
    }
    int64_t b0 = 0, b1 = 0;
    if (a.bin > 0 && p1 > p0) {
        b0 = p0 / a.bin;
        b1 = (p1 - 1) / a.bin;
    }
    m.binfo = (b0 << 1) | (b0 == b1 ? 1 : 0);
    a.meta[t] = m;
}

__device__ __forceinline__ uint32_t summary_kind(uint32_t c)        // class_of of seq_kernels.hip
{
    const uint32_t l = c | 0x20u;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

__global__ void __launch_bounds__(256) summary_tile_kernel(summary_args a)
{
    extern __shared__ unsigned summary_lds[];
    unsigned *cnt = summary_lds;                                 // [C * 10][rep]
    unsigned *binacc = summary_lds + a.C * SUMMARY_CELLS * a.rep;    // [C]: the bin columns of a tile that lies in one bin
    __shared__ uint64_t lds[4];
    const int tid = threadIdx.x, slot = tid & (a.rep - 1);
    const int cells = a.C * SUMMARY_CELLS;
    for (int i = tid; i < cells * a.rep + a.C; i += 256) summary_lds[i] = 0u;
    // (the barriers of the first tile's scan publish the zeroes: no counter is touched in front of them)
    const int64_t t_begin = (int64_t)blockIdx.x * a.per, t_end = t_begin + a.per < a.ntiles ? t_begin + a.per : a.ntiles;
    int64_t cur = -1;

    auto flush = [&](int64_t rec) {                              // (uniform: every lane calls it)
        __syncthreads();
        for (int i = tid; i < cells; i += 256) {
            unsigned long long v = 0;
            for (int s = 0; s < a.rep; ++s) {
                v += cnt[i * a.rep + s];
                cnt[i * a.rep + s] = 0u;
            }
            if (v) atomicAdd(&a.counts[rec * cells + i], v);
        }
        __syncthreads();
    };

    for (int64_t t = t_begin; t < t_end; ++t) {
        const summary_tile m = a.meta[t];                        // (uniform: one load for the workgroup, no lane-0 section)
        const int64_t r = m.rec, rlo = m.lo, rhi = m.hi, p0 = m.p0;
        const bool one_bin = (m.binfo & 1) != 0;
        const int64_t tile_bin = m.binfo >> 1;
        if (r != cur) {
            if (cur >= 0) flush(cur);
            cur = r;
        }
        const body_span s = body_lane_span(a.off[r], a.len[r], t - a.tile0[r]);
        alignas(16) uint8_t b[16];
        body_load(a.raw, s, b);
        uint64_t c = 0;
        for (int j = 0; j < 16; ++j) c += body_lineend(b[j]) ? 0 : 1;
        int64_t p = p0 + (int64_t)block_exclusive_scan(c, nullptr, lds);
        const uint64_t w0 = ((const uint64_t *)b)[0], w1 = ((const uint64_t *)b)[1];      // (the walk shifts bytes out of registers)
        unsigned acgt = 0;                                       // ACGT bases of the lane's current bin
        if (c) {
            // the first row of the tile's list that ends after p
            int64_t j = rlo, hi = rhi;
            while (j < hi) {
                const int64_t mid = (j + hi) >> 1;
                if (a.crows[mid].end <= p) j = mid + 1; else hi = mid;
            }
            int64_t cs = 0, ce = 0;                              // row j, when j < rhi
            int cl = 0;
            if (j < rhi) {
                const dgrp_segment q = a.crows[j];
                cs = q.start; ce = q.end; cl = q.label;
            }
            unsigned long long *binrow = nullptr;                // the lane's current bin (tiles over several bins)
            int64_t edge = 0;                                    // first position of the next bin
            if (a.bin > 0 && !one_bin) {
                const int64_t bi = p / a.bin;
                binrow = a.bins + (a.bin_off[r] + bi) * a.C;
                edge = (bi + 1) * a.bin;
            }
            int run = -1;                                        // label of the run being counted
            uint64_t acc = 0;                                    // its counts: ten 5-bit fields (at most 16 each)
            unsigned runbin = 0;                                 // its positions in the current bin
            auto flush_run = [&]() {
                if (run < 0) return;
                for (int cell = 0; cell < SUMMARY_CELLS; ++cell) {
                    const unsigned v = (unsigned)(acc >> (5 * cell)) & 31u;
                    if (v) atomicAdd(&cnt[(run * SUMMARY_CELLS + cell) * a.rep + slot], v);
                }
                acc = 0;
            };
            auto flush_bin_label = [&]() {
                if (a.bin > 0 && run > 0 && runbin) {
                    if (one_bin) atomicAdd(&binacc[run], runbin);
                    else atomicAdd(&binrow[run], (unsigned long long)runbin);
                }
                runbin = 0;
            };
            for (int k = 0; k < 16; ++k) {
                const uint32_t x = (uint32_t)((k < 8 ? w0 >> (8 * k) : w1 >> (8 * (k - 8))) & 0xff);
                if (body_lineend(x)) continue;                   // (also the padding outside the record)
                while (j < rhi && ce <= p) {
                    ++j;
                    if (j < rhi) {
                        const dgrp_segment q = a.crows[j];
                        cs = q.start; ce = q.end; cl = q.label;
                    }
                }
                const int label = (j < rhi && cs <= p) ? cl : 0;
                if (binrow && p == edge) {                       // the next bin
                    flush_bin_label();
                    if (acgt) atomicAdd(&binrow[0], (unsigned long long)acgt);
                    acgt = 0;
                    binrow += a.C;
                    edge += a.bin;
                }
                if (label != run) {
                    flush_bin_label();
                    flush_run();
                    run = label;
                }
                const uint32_t kind = summary_kind(x);
                const uint32_t lower = (x >= 'a' && x <= 'z') ? 1u : 0u;
                acc += 1ull << (5 * (kind * 2 + lower));
                ++runbin;
                acgt += kind < 4 ? 1u : 0u;
                ++p;
            }
            flush_bin_label();
            flush_run();
            if (binrow && acgt) atomicAdd(&binrow[0], (unsigned long long)acgt);
        }
        if (a.bin > 0 && one_bin) {                              // (uniform) the tile's bin columns: LDS, then one add per column
            for (int o = 32; o > 0; o >>= 1) acgt += __shfl_xor(acgt, o);
            if ((tid & 63) == 0 && acgt) atomicAdd(&binacc[0], acgt);
            __syncthreads();
            if (tid < a.C) {
                const unsigned v = binacc[tid];
                binacc[tid] = 0u;
                if (v) atomicAdd(&a.bins[(a.bin_off[r] + tile_bin) * a.C + tid], (unsigned long long)v);
            }
            // (the barriers of the next tile's scan, or of the flush, stand between this and the next add to binacc)
        }
    }
    if (cur >= 0) flush(cur);
}

static inline int64_t summary_scan_tiles(int64_t nrows) { return (nrows + 1 + SCAN_TILE - 1) / SCAN_TILE; }

static inline int summary_rep(int C)
{
    int rep = 64;
    while (rep > 1 && (int64_t)C * SUMMARY_CELLS * rep * 4 > SUMMARY_LDS_BYTES) rep >>= 1;
    return rep;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_repeat_summary_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows)
{
    if (nrec < 0 || total_bytes < 0 || nrows < 0) return 0;
    const int64_t tiles = body_tile_bound(nrec, total_bytes);
    // tile counts and their scan; the tables; per row: keep flag / compacted index, the compacted row; the scan's tile sums
    return dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up((5 * nrec + 3) * 8, 256) + dgrp_align_up((nrows + 1) * 8, 256) +
           dgrp_align_up((nrows + 1) * (int64_t)sizeof(dgrp_segment), 256) + dgrp_align_up(summary_scan_tiles(nrows) * 8, 256) +
           dgrp_align_up(summary_scan_tiles(tiles) * 8, 256) + dgrp_align_up(tiles * (int64_t)sizeof(summary_tile), 256);
}

DGRP_EXPORT int dgrp_repeat_summary_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                          const dgrp_segment *d_rows, const int64_t *h_row_off, int C, int64_t bin,
                                          const int64_t *h_bin_off, int64_t *d_counts, int64_t *d_bins, int64_t *d_bad, void *d_work,
                                          int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    // ---- host tables and scalars
    DGRP_REQUIRE(C >= 2 && C <= DGRP_MAXC, "dgrp_repeat_summary_batch: 2 <= classes <= 64, got %d", C);
    DGRP_REQUIRE(bin >= 0, "dgrp_repeat_summary_batch: negative bin %lld", (long long)bin);
    DGRP_REQUIRE(nrec >= 0 && (nrec == 0 || (h_off && h_len && h_row_off && (bin == 0 || h_bin_off))),
                 "dgrp_repeat_summary_batch: bad arguments");
    DGRP_REQUIRE(work_bytes >= 0, "dgrp_repeat_summary_batch: negative size");
    DGRP_REQUIRE(nrec < ((int64_t)1 << 28), "dgrp_repeat_summary_batch: too many records");
    if (nrec == 0) return DGRP_OK;
    int64_t total = 0;
    // tile0[nrec + 1], off[nrec], len[nrec], row_off[nrec + 1], bin_off[nrec + 1]
    std::vector<int64_t> tab((size_t)(5 * nrec + 3), 0);
    int64_t *tile0 = tab.data(), *off = tile0 + nrec + 1, *len = off + nrec, *row_off = len + nrec, *bin_off = row_off + nrec + 1;
    DGRP_REQUIRE(h_row_off[0] >= 0, "dgrp_repeat_summary_batch: negative row offset");
    DGRP_REQUIRE(bin == 0 || h_bin_off[0] >= 0, "dgrp_repeat_summary_batch: negative bin offset");
    tile0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0, "dgrp_repeat_summary_batch: negative range (record %lld)", (long long)r);
        DGRP_REQUIRE(h_off[r] < ((int64_t)1 << 46) && h_len[r] < ((int64_t)1 << 46), "dgrp_repeat_summary_batch: too long (record %lld)",
                     (long long)r);
        DGRP_REQUIRE(r == 0 || h_off[r] >= h_off[r - 1] + h_len[r - 1],
                     "dgrp_repeat_summary_batch: record ranges must ascend and not overlap (record %lld)", (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "dgrp_repeat_summary_batch: row offsets must ascend (record %lld)", (long long)r);
        if (bin > 0) {
            // a record's sequence is at most its bytes: ceil(h_len / bin) bins hold every position
            DGRP_REQUIRE(h_bin_off[r + 1] - h_bin_off[r] >= (h_len[r] + bin - 1) / bin,
                         "dgrp_repeat_summary_batch: record %lld has room for %lld bins, below ceil(%lld / %lld)", (long long)r,
                         (long long)(h_bin_off[r + 1] - h_bin_off[r]), (long long)h_len[r], (long long)bin);
        }
        total += h_len[r];
        off[r] = h_off[r];
        len[r] = h_len[r];
        tile0[r + 1] = tile0[r] + body_tiles_of(h_off[r], h_len[r]);
    }
    for (int64_t r = 0; r <= nrec; ++r) {
        row_off[r] = h_row_off[r];
        bin_off[r] = bin > 0 ? h_bin_off[r] : 0;
    }
    const int64_t ntiles = tile0[nrec], nrows = row_off[nrec] - row_off[0], nbins = bin > 0 ? bin_off[nrec] : 0;
    DGRP_REQUIRE(nrows < ((int64_t)1 << 31), "dgrp_repeat_summary_batch: more than 2^31 - 1 rows");
    DGRP_REQUIRE(nbins < ((int64_t)1 << 40), "dgrp_repeat_summary_batch: more than 2^40 bins");
    DGRP_REQUIRE(ntiles < ((int64_t)1 << 31), "dgrp_repeat_summary_batch: more than 2^31 - 1 tiles of 4096 bytes");
    // ---- the workspace
    if (work_bytes < dgrp_repeat_summary_workspace_bytes(nrec, total, nrows)) {
        dgrp_set_error("dgrp_repeat_summary_batch: workspace too small");
        return DGRP_ENOMEM;
    }
    // ---- device pointers
    DGRP_REQUIRE(d_work && d_counts && d_bad && (nrows == 0 || d_rows) && (ntiles == 0 || d_raw) && (nbins == 0 || d_bins),
                 "dgrp_repeat_summary_batch: NULL device pointer");
    DGRP_REQUIRE(((uintptr_t)d_raw & 15) == 0, "dgrp_repeat_summary_batch: d_raw must be 16-byte aligned");
    DGRP_REQUIRE(((uintptr_t)d_rows & 7) == 0 && ((uintptr_t)d_counts & 7) == 0 && ((uintptr_t)d_bins & 7) == 0 &&
                 ((uintptr_t)d_bad & 7) == 0 && ((uintptr_t)d_work & 255) == 0,
                 "dgrp_repeat_summary_batch: d_rows, d_counts, d_bins and d_bad must be 8-byte aligned, d_work 256-byte aligned");
    const int64_t tiles_cap = body_tile_bound(nrec, total);
    char *w = (char *)d_work;
    uint64_t *ex = (uint64_t *)w;                                           // per tile: sequence bytes, then their exclusive scan
    w += dgrp_align_up((tiles_cap + 1) * 8, 256);
    int64_t *d_tab = (int64_t *)w;
    w += dgrp_align_up((5 * nrec + 3) * 8, 256);
    uint64_t *kidx = (uint64_t *)w;                                         // per row: good, then the exclusive scan of that
    w += dgrp_align_up((nrows + 1) * 8, 256);
    dgrp_segment *crows = (dgrp_segment *)w;                                // the good rows back to back
    w += dgrp_align_up((nrows + 1) * (int64_t)sizeof(dgrp_segment), 256);
    uint64_t *scan_a = (uint64_t *)w;
    w += dgrp_align_up(summary_scan_tiles(nrows) * 8, 256);
    uint64_t *scan_b = (uint64_t *)w;                                       // the tile sums of the scan over ex
    w += dgrp_align_up(summary_scan_tiles(tiles_cap) * 8, 256);
    summary_tile *meta = (summary_tile *)w;                                 // per tile: where the walk starts it
    const int64_t *d_tile0 = d_tab, *d_off = d_tab + nrec + 1, *d_len = d_off + nrec, *d_row_off = d_len + nrec,
                  *d_bin_off = d_row_off + nrec + 1;
    // the outputs are zeroed here (d_bad: -1); everything below is ordered on `stream`
    DGRP_HIP(hipMemsetAsync(d_counts, 0, (size_t)nrec * C * SUMMARY_CELLS * 8, stream));
    if (nbins > 0) DGRP_HIP(hipMemsetAsync(d_bins, 0, (size_t)nbins * C * 8, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0xFF, 8, stream));
    // (a pageable source is staged before hipMemcpyAsync returns: the vector may go when the entry does)
    DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    if (ntiles > 0) {
        hipLaunchKernelGGL(summary_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, d_tile0, d_off, d_len, nrec, ex);
        DGRP_LAUNCH_CHECK();
    }
    // ex[0 .. ntiles] <- exclusive scan of the tile counts and a zero behind them: ex[ntiles] is the total (three parallel launches:
    // one workgroup over the 6 * 10^4 tiles of a chromosome would take as long as the walk)
    DGRP_HIP(hipMemsetAsync(ex + ntiles, 0, 8, stream));
    {
        const int rc = device_exclusive_scan(ex, ex, ntiles + 1, scan_b, nullptr, stream);
        if (rc != DGRP_OK) return rc;
    }
    if (nrows > 0) {
        hipLaunchKernelGGL(summary_check_kernel, dim3((unsigned)((nrows + 1 + 255) / 256)), dim3(256), 0, stream, d_rows, d_row_off, nrec,
                           d_tile0, ex, C, kidx, (unsigned long long *)d_bad);
        DGRP_LAUNCH_CHECK();
        const int rc = device_exclusive_scan(kidx, kidx, nrows + 1, scan_a, nullptr, stream);
        if (rc != DGRP_OK) return rc;
        hipLaunchKernelGGL(summary_compact_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, d_rows, row_off[0], nrows,
                           kidx, crows);
        DGRP_LAUNCH_CHECK();
    }
    if (ntiles == 0) return DGRP_OK;
    summary_args a;
    a.raw = d_raw;
    a.tile0 = d_tile0; a.off = d_off; a.len = d_len; a.row_off = d_row_off; a.bin_off = d_bin_off;
    a.ex = ex;
    a.kidx = nrows > 0 ? kidx : nullptr;
    a.crows = crows;
    a.nrec = nrec; a.ntiles = ntiles; a.bin = bin;
    a.C = C; a.rep = summary_rep(C);
    const size_t lds = ((size_t)C * SUMMARY_CELLS * a.rep + C) * sizeof(unsigned);
    a.per = (ntiles + SUMMARY_GRID - 1) / SUMMARY_GRID;
    if (a.per > SUMMARY_MAX_PER) a.per = SUMMARY_MAX_PER;
    a.counts = (unsigned long long *)d_counts;
    a.bins = (unsigned long long *)d_bins;
    a.meta = meta;
    hipLaunchKernelGGL(summary_tiles_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, stream, a);
    DGRP_LAUNCH_CHECK();
    const int64_t grid = (ntiles + a.per - 1) / a.per;
    hipLaunchKernelGGL(summary_tile_kernel, dim3((unsigned)grid), dim3(256), lds, stream, a);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
