// Masked FASTA output (predict --mask_dir): the sequence bytes of plain record bodies rewritten in place of the file's bytes, soft
// (inside a masked row lower case, elsewhere upper case) or hard (inside 'N').  A byte stream: one read for the per-tile counts, one
// read and one write for the rewrite, 16 bytes per lane.  See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "body_tiles.h"
#include "scan.h"
#include <vector>

namespace {

#define MASK_LDS_ROWS 256         // rows of one tile staged in LDS; a tile crossing more reads them from global memory

__global__ void __launch_bounds__(256) mask_count_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ tile0,
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

// one lane per row: 0 <= start < end <= sequence length of its record, rows of a record ascending and disjoint.
// g[0] |= 1 on a bad row, g[1] = smallest bad row index.
__global__ void __launch_bounds__(256) mask_check_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                         int64_t nrec, const int64_t *__restrict__ tile0,
                                                         const uint64_t *__restrict__ ex, unsigned long long *__restrict__ g)
{
    const int64_t i = row_off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= row_off[nrec]) return;
    int64_t lo = 0, hi = nrec;                    // record of row i: largest r with row_off[r] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_off[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t seqlen = (int64_t)(ex[tile0[lo + 1]] - ex[tile0[lo]]);
    const int64_t st = rows[i].start, en = rows[i].end;
    bool bad = st < 0 || en <= st || en > seqlen;
    if (i + 1 < row_off[lo + 1] && rows[i + 1].start < en) bad = true;
    if (bad) {
        atomicOr(&g[0], 1ull);
        atomicMin(&g[1], (unsigned long long)i);
    }
}

// (raw and out may be the same buffer: every lane reads its 16 bytes before it writes them, and no lane touches another's)
__global__ void __launch_bounds__(256) mask_apply_kernel(const uint8_t *raw, uint8_t *out,
                                                         const int64_t *__restrict__ tile0, const int64_t *__restrict__ off,
                                                         const int64_t *__restrict__ len, const int64_t *__restrict__ row_off,
                                                         int64_t nrec, const uint64_t *__restrict__ ex,
                                                         const dgrp_segment *__restrict__ rows, int hard, uint64_t class_mask)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_rec, s_p0, s_lo, s_hi;
    __shared__ int64_t r_st[MASK_LDS_ROWS], r_en[MASK_LDS_ROWS];
    __shared__ uint8_t r_in[MASK_LDS_ROWS];
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) {
        const int64_t r = dgrp_record_of(tile0, nrec, t);
        const int64_t p0 = (int64_t)(ex[t] - ex[tile0[r]]), p1 = p0 + (int64_t)(ex[t + 1] - ex[t]);
        // rows of this tile: the first that ends after p0 up to the first that starts at or after p1
        int64_t a = row_off[r], b = row_off[r + 1];
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (rows[mid].end <= p0) a = mid + 1; else b = mid;
        }
        int64_t c = a, d = row_off[r + 1];
        while (c < d) {
            const int64_t mid = (c + d) >> 1;
            if (rows[mid].start < p1) c = mid + 1; else d = mid;
        }
        s_rec = r; s_p0 = p0; s_lo = a; s_hi = c;
    }
    __syncthreads();
    const int64_t r = s_rec, rlo = s_lo, rhi = s_hi;
    const bool staged = rhi - rlo <= MASK_LDS_ROWS;
    if (staged) {
        for (int64_t j = threadIdx.x; j < rhi - rlo; j += blockDim.x) {
            const dgrp_segment q = rows[rlo + j];
            r_st[j] = q.start;
            r_en[j] = q.end;
            r_in[j] = (q.label >= 0 && q.label < 64 && ((class_mask >> q.label) & 1)) ? 1 : 0;
        }
    }
    const body_span s = body_lane_span(off[r], len[r], t - tile0[r]);
    alignas(16) uint8_t b[16];
    body_load(raw, s, b);
    uint64_t c = 0;
    for (int j = 0; j < 16; ++j) c += body_lineend(b[j]) ? 0 : 1;
    int64_t p = s_p0 + (int64_t)block_exclusive_scan(c, nullptr, lds);      // (its barriers also publish the staged rows)
    // local row index: the first row of the tile's list that ends after p
    auto row_end = [&](int64_t j) { return staged ? r_en[j] : rows[rlo + j].end; };
    int64_t lo = 0, hi = rhi - rlo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_end(mid) <= p) lo = mid + 1; else hi = mid;
    }
    int64_t j = lo;
    const int64_t n = rhi - rlo;
    for (int k = 0; k < 16; ++k) {
        const uint32_t x = b[k];
        if (body_lineend(x)) continue;               // (also the padding outside the record)
        while (j < n && row_end(j) <= p) ++j;
        bool inside = false;
        if (j < n) {
            if (staged) {
                inside = r_st[j] <= p && r_in[j];
            } else {
                const dgrp_segment q = rows[rlo + j];
                inside = q.start <= p && q.label >= 0 && q.label < 64 && ((class_mask >> q.label) & 1);
            }
        }
        const uint32_t l = x | 0x20u;
        const bool letter = l >= 'a' && l <= 'z';
        b[k] = hard ? (inside ? (uint8_t)'N' : (uint8_t)x)
                    : (letter ? (uint8_t)(inside ? l : (x & ~0x20u)) : (uint8_t)x);
        ++p;
    }
    if (s.lo == 0 && s.hi == 16) {
        *(uint4 *)(out + s.word) = *(const uint4 *)b;
    } else {
        for (int k = s.lo; k < s.hi; ++k) out[s.word + k] = b[k];
    }
}

}   // namespace

DGRP_EXPORT int64_t dgrp_fasta_mask_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows)
{
    if (nrec < 0 || total_bytes < 0 || nrows < 0) return 0;
    const int64_t tiles = body_tile_bound(nrec, total_bytes);
    return 256 + dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up((4 * nrec + 2) * 8, 256);
}

DGRP_EXPORT int dgrp_fasta_mask_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                      const dgrp_segment *d_rows, const int64_t *h_row_off, int mode, uint64_t class_mask,
                                      uint8_t *d_out, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(nrec >= 0 && (nrec == 0 || (h_off && h_len && h_row_off)), "dgrp_fasta_mask_batch: bad arguments");
    DGRP_REQUIRE(mode == 0 || mode == 1, "dgrp_fasta_mask_batch: mode must be 0 (soft) or 1 (hard), got %d", mode);
    if (nrec == 0) return DGRP_OK;
    int64_t total = 0;
    std::vector<int64_t> tab((size_t)(4 * nrec + 2));                       // tile0[nrec + 1], off[nrec], len[nrec], row_off[nrec + 1]
    int64_t *tile0 = tab.data(), *off = tile0 + nrec + 1, *len = off + nrec, *row_off = len + nrec;
    DGRP_REQUIRE(h_row_off[0] >= 0, "dgrp_fasta_mask_batch: negative row offset");
    tile0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0, "dgrp_fasta_mask_batch: negative range (record %lld)", (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "dgrp_fasta_mask_batch: row offsets must ascend (record %lld)", (long long)r);
        total += h_len[r];
        off[r] = h_off[r];
        len[r] = h_len[r];
        tile0[r + 1] = tile0[r] + body_tiles_of(h_off[r], h_len[r]);
    }
    for (int64_t r = 0; r <= nrec; ++r) row_off[r] = h_row_off[r];
    const int64_t ntiles = tile0[nrec], nrows = row_off[nrec] - row_off[0];
    if (ntiles == 0) return DGRP_OK;
    DGRP_REQUIRE(d_raw && d_out && d_work && (nrows == 0 || d_rows), "dgrp_fasta_mask_batch: NULL pointer");
    DGRP_REQUIRE(((uintptr_t)d_raw & 15) == 0 && ((uintptr_t)d_out & 15) == 0, "dgrp_fasta_mask_batch: d_raw and d_out must be 16-byte aligned");
    if (work_bytes < dgrp_fasta_mask_workspace_bytes(nrec, total, nrows)) {
        dgrp_set_error("dgrp_fasta_mask_batch: workspace too small");
        return DGRP_ENOMEM;
    }
    unsigned long long *g = (unsigned long long *)d_work;
    uint64_t *ex = (uint64_t *)((char *)d_work + 256);                     // per tile: sequence characters, then their exclusive scan
    int64_t *d_tab = (int64_t *)((char *)ex + dgrp_align_up((ntiles + 1) * 8, 256));
    int64_t *d_tile0 = d_tab, *d_off = d_tile0 + nrec + 1, *d_len = d_off + nrec, *d_row_off = d_len + nrec;
    const unsigned long long init[2] = { 0ull, ~0ull };
    DGRP_HIP(hipMemcpyAsync(g, init, sizeof(init), hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, d_tile0, d_off, d_len, nrec, ex);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, ex, ntiles, ex + ntiles);
    DGRP_LAUNCH_CHECK();
    if (nrows > 0) {
        hipLaunchKernelGGL(mask_check_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, d_rows, d_row_off, nrec,
                           d_tile0, ex, g);
        DGRP_LAUNCH_CHECK();
        unsigned long long hg[2];
        DGRP_HIP(hipMemcpyAsync(hg, g, sizeof(hg), hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipStreamSynchronize(stream));
        if (hg[0]) {
            const int64_t i = (int64_t)hg[1];
            int64_t r = 0;
            while (r + 1 < nrec && row_off[r + 1] <= i) ++r;
            dgrp_segment q;
            uint64_t e[2];
            DGRP_HIP(hipMemcpy(&q, d_rows + i, sizeof(q), hipMemcpyDeviceToHost));
            DGRP_HIP(hipMemcpy(&e[0], ex + tile0[r], 8, hipMemcpyDeviceToHost));
            DGRP_HIP(hipMemcpy(&e[1], ex + tile0[r + 1], 8, hipMemcpyDeviceToHost));
            DGRP_REQUIRE(false, "dgrp_fasta_mask_batch: row %lld [%lld, %lld) of record %lld is empty, out of order or beyond its "
                                "sequence of %lld characters", (long long)i, (long long)q.start, (long long)q.end, (long long)r,
                         (long long)(e[1] - e[0]));
        }
    }
    hipLaunchKernelGGL(mask_apply_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, d_out, d_tile0, d_off, d_len,
                       d_row_off, nrec, ex, d_rows, mode, class_mask);
    DGRP_LAUNCH_CHECK();
    // (the tables above are host vectors: their copies were complete at the synchronisation; without rows, wait here)
    if (nrows == 0) DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}
