// N2: the evaluation helpers next to the prediction path, on per-base label arrays that are already in
// HBM -- deepgrp.prediction.confusion_matrix (deepgrp/prediction.py:204-222) and filter_segments (:244-260).
// Both are single-pass, HBM-bound byte scans (2 B/bp and 1-2 B/bp).
#include "dgrp_common.h"

// cnf[t][p] += 1 for every base: a 16 x 16 (beyond 16 classes: 64 x 64) histogram per workgroup in LDS (wave-private copies would not pay: at
// most a few distinct cells are hot, ds_add_u32 serialises those whatever the layout), flushed with one 64-bit
// atomic per non-zero cell.
__global__ void __launch_bounds__(256) confusion_kernel(const int8_t *__restrict__ truth, const int8_t *__restrict__ pred,
                                                        int64_t n, int ncls, unsigned long long *__restrict__ cnf,
                                                        int *__restrict__ bad)
{
    __shared__ unsigned hist[DGRP_MAXC * DGRP_MAXC];
    const int pitch = ncls <= 16 ? 16 : DGRP_MAXC;
    for (int i = threadIdx.x; i < pitch * pitch; i += 256) hist[i] = 0u;
    __syncthreads();
    const int64_t per = 16 * 256;                                     // bases per workgroup iteration (16 B per lane)
    for (int64_t base = (int64_t)blockIdx.x * per; base < n; base += (int64_t)gridDim.x * per) {
        const int64_t i0 = base + (int64_t)threadIdx.x * 16;
        if (i0 + 16 <= n) {
            const uint4 tv = *reinterpret_cast<const uint4 *>(truth + i0), pv = *reinterpret_cast<const uint4 *>(pred + i0);
            const uint32_t tw[4] = { tv.x, tv.y, tv.z, tv.w }, pw[4] = { pv.x, pv.y, pv.z, pv.w };
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int t = (int8_t)(tw[k >> 2] >> (8 * (k & 3))), q = (int8_t)(pw[k >> 2] >> (8 * (k & 3)));
                if ((unsigned)t < (unsigned)ncls && (unsigned)q < (unsigned)ncls) atomicAdd(&hist[t * pitch + q], 1u);
                else *bad = 1;
            }
        } else {
            for (int64_t i = i0; i < n && i < i0 + 16; ++i) {
                const int t = truth[i], q = pred[i];
                if ((unsigned)t < (unsigned)ncls && (unsigned)q < (unsigned)ncls) atomicAdd(&hist[t * pitch + q], 1u);
                else *bad = 1;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < pitch * pitch; i += 256) {
        const unsigned v = hist[i];
        const int t = i / pitch, q = i % pitch;
        if (v != 0u && t < ncls && q < ncls) atomicAdd(&cnf[t * ncls + q], (unsigned long long)v);
    }
}

DGRP_EXPORT int dgrp_confusion_matrix(const int8_t *d_true, const int8_t *d_pred, int64_t n, int ncls, int64_t *d_cnf,
                                      int *d_bad, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(n >= 0 && ncls >= 1 && ncls <= DGRP_MAXC && d_cnf && d_bad, "dgrp_confusion_matrix: bad arguments (1 <= classes <= 64)");
    DGRP_HIP(hipMemsetAsync(d_cnf, 0, sizeof(int64_t) * ncls * ncls, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
    if (n == 0) return DGRP_OK;
    DGRP_REQUIRE(d_true && d_pred, "dgrp_confusion_matrix: NULL pointer");
    DGRP_REQUIRE(((uintptr_t)d_true & 15) == 0 && ((uintptr_t)d_pred & 15) == 0, "dgrp_confusion_matrix: label arrays must be 16-byte aligned");
    const int64_t groups = (n + 4095) / 4096;
    const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
    hipLaunchKernelGGL(confusion_kernel, dim3(grid), dim3(256), 0, stream, d_true, d_pred, n, ncls,
                       reinterpret_cast<unsigned long long *>(d_cnf), d_bad);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// filter_segments: runs of one positive label shorter than min_len become 0.  A thread that sits on the first base
// of a positive run walks at most min_len bases forward; only runs that are about to be cleared are ever written,
// so the in-place form is race-free in effect: a neighbour that sees a half-cleared short run can only decide
// "start of a short run" for bases that are being cleared anyway, and long runs are never touched.
__global__ void __launch_bounds__(256) filter_segments_kernel(const int8_t *in, int8_t *out,
                                                              int64_t n, int64_t min_len)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int8_t v = in[i];
    if (in != out) {
        // out of place: every base decides for itself from the untouched input
        if (v <= 0) { out[i] = v; return; }
        int64_t lo = i, hi = i + 1;
        while (lo > 0 && i - lo + 1 < min_len && in[lo - 1] == v) --lo;
        while (hi < n && hi - lo < min_len && in[hi] == v) ++hi;
        out[i] = hi - lo < min_len ? (int8_t)0 : v;
        return;
    }
    if (v <= 0 || (i > 0 && in[i - 1] == v)) return;
    int64_t j = i + 1;
    while (j < n && j - i < min_len && in[j] == v) ++j;
    if (j - i < min_len)
        for (int64_t k = i; k < j; ++k) out[k] = 0;
}

DGRP_EXPORT int dgrp_filter_segments(const int8_t *d_labels, int8_t *d_out, int64_t n, int64_t min_len, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(n >= 0, "dgrp_filter_segments: negative length");
    if (n == 0) return DGRP_OK;
    DGRP_REQUIRE(d_labels && d_out, "dgrp_filter_segments: NULL pointer");
    DGRP_REQUIRE(n < (1ll << 39), "dgrp_filter_segments: too long");
    hipLaunchKernelGGL(filter_segments_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_labels, d_out, n, min_len);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// evaluate: label rows painted onto a flat per-base buffer, and per-row hit counts against such a buffer.  Records lie back to back
// in one int8 buffer (record r: [off[r], off[r] + len[r]), its first base has the original coordinate origin[r]); rows are
// dgrp_segment in original coordinates, clipped to their record.  Work is shared out by LENGTH, not by row: an exclusive scan of
// the clipped lengths gives every row its place on one line of positions, and workgroup b takes positions
// [b * EVAL_SLICE, (b + 1) * EVAL_SLICE) of that line (rows run from 10 bp to megabases).
// ------------------------------------------------------------------------------------------------------------------------------
#include "eval_rows.h"

namespace {

#define EVAL_LDS_ROWS 2048        // hits: the slice's per-row counters in LDS; a slice crossing more rows adds to d_hits directly
#define EVAL_HEAD 2048            // workspace head: flag + first bad row at 0, clipped length per label (128 x u64) at 1024

// one lane per row: 0 <= start <= end and 1 <= label <= max_label (at most 127), else g[0] |= 1 and g[1] = smallest bad row; tot[label] += clipped length
// (summed per workgroup in LDS first: a handful of labels would otherwise serialise one global atomic per row).  With `scores` (the
// rows are predict's scored rows, dgrp_paint_row_keys_batch) two more rules: a row with a base inside its record is bed_scored(), else
// g[0] |= 2 and g[2] = the smallest such row; a row does not start below the end of the row in front of it in its record, else
// g[0] |= 4 and g[3] likewise
__global__ void __launch_bounds__(256) eval_check_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                         int64_t nrec, const int64_t *__restrict__ len,
                                                         const int64_t *__restrict__ origin, int max_label,
                                                         const dgrp_row_score *__restrict__ scores,
                                                         unsigned long long *__restrict__ g, unsigned long long *__restrict__ tot,
                                                         const uint32_t *__restrict__ row_key)
{
    __shared__ unsigned long long s_tot[128];
    if (threadIdx.x < 128) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t i = row_off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < row_off[nrec]) {
        const dgrp_segment q = rows[i];
        // (rows with keys of their own: the label is not read, the key must not be the fill, the lengths are summed under label 1)
        const bool bad_mark = row_key ? row_key[i] == 0xFFFFFFFFu : (q.label < 1 || q.label > max_label);
        if (q.start < 0 || q.end < q.start || bad_mark) {
            atomicOr(&g[0], 1ull);
            atomicMin(&g[1], (unsigned long long)i);
        } else {
            const int64_t r = dgrp_record_of(row_off, nrec, i);
            int64_t cs, cl;
            eval_clip(q, origin[r], len[r], cs, cl);
            if (cl) atomicAdd(&s_tot[row_key ? 1 : q.label], (unsigned long long)cl);
            if (scores) {
                if (cl && !bed_scored(scores[i])) {
                    atomicOr(&g[0], 2ull);
                    atomicMin(&g[2], (unsigned long long)i);
                }
                if (i > row_off[r] && q.start < rows[i - 1].end) {
                    atomicOr(&g[0], 4ull);
                    atomicMin(&g[3], (unsigned long long)i);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 128 && s_tot[threadIdx.x]) atomicAdd(&tot[threadIdx.x], s_tot[threadIdx.x]);
}

// one lane per row j (= row row_off[0] + j): cl[j] = its clipped length if its label is `label` (0: any), else 0; dst[j] = the
// buffer position of its first clipped base
__global__ void __launch_bounds__(256) eval_span_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                        int64_t nrec, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                        const int64_t *__restrict__ origin, int label, uint64_t *__restrict__ cl,
                                                        int64_t *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = row_off[0] + j;
    if (i >= row_off[nrec]) return;
    const dgrp_segment q = rows[i];
    const int64_t r = dgrp_record_of(row_off, nrec, i);
    int64_t cs, n;
    eval_clip(q, origin[r], len[r], cs, n);
    cl[j] = (label == 0 || q.label == label) ? (uint64_t)n : 0;
    dst[j] = off[r] + cs;
}

// hits[j] += bases of row j's clipped span whose label equals row j's: per-lane counts per row, gathered in LDS per row of the
// slice, then one 64-bit atomic per (workgroup, row) with hits
__global__ void __launch_bounds__(256) eval_hits_kernel(const int8_t *__restrict__ labels, const uint64_t *__restrict__ ex,
                                                        const int64_t *__restrict__ dst, const dgrp_segment *__restrict__ rows,
                                                        int64_t n, unsigned long long *__restrict__ hits)
{
    __shared__ unsigned cnt[EVAL_LDS_ROWS];
    __shared__ int64_t s_r0, s_r1;
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;    // (s0 < total: the grid covers the line exactly)
    if (threadIdx.x == 0) {
        s_r0 = eval_row_of(ex, 0, n, s0);
        s_r1 = eval_row_of(ex, s_r0, n, s1 - 1);
    }
    for (int k = threadIdx.x; k < EVAL_LDS_ROWS; k += 256) cnt[k] = 0u;
    __syncthreads();
    const int64_t r0 = s_r0, r1 = s_r1;
    const bool staged = r1 - r0 < EVAL_LDS_ROWS;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 < s1) {
        int64_t j = eval_row_of(ex, r0, r1 + 1, p0);
        uint64_t jst = ex[j], jend = ex[j + 1];
        int lab = rows[j].label;
        unsigned c = 0;
        for (uint64_t p = p0; p < s1; p += 256) {
            if (jend <= p) {
                if (c) {
                    if (staged) atomicAdd(&cnt[j - r0], c);
                    else atomicAdd(&hits[j], (unsigned long long)c);
                }
                c = 0;
                while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
                lab = rows[j].label;
            }
            c += labels[dst[j] + (int64_t)(p - jst)] == lab ? 1u : 0u;
        }
        if (c) {
            if (staged) atomicAdd(&cnt[j - r0], c);
            else atomicAdd(&hits[j], (unsigned long long)c);
        }
    }
    __syncthreads();
    if (staged) {
        for (int64_t k = threadIdx.x; k <= r1 - r0; k += 256) {
            const unsigned v = cnt[k];
            if (v) atomicAdd(&hits[r0 + k], (unsigned long long)v);
        }
    }
}

}   // namespace

// (eval_rows.h) argument checks, tables to the device, the row check (one synchronisation): DGRP_EINVAL on a bad row before anything is written.
// d_scores: the rows are scored rows, checked as eval_check_kernel says; extra_bytes: more workspace, 256-byte aligned, at pl.d_extra
int eval_prepare(const char *what, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                 const dgrp_segment *d_rows, const int64_t *h_row_off, void *d_work, int64_t work_bytes, hipStream_t stream,
                 eval_plan &pl, int max_label, const dgrp_row_score *d_scores, int64_t extra_bytes, const uint32_t *d_row_key)
{
    DGRP_REQUIRE(nrec >= 0 && h_row_off && (nrec == 0 || (h_off && h_len && h_origin)), "%s: bad arguments", what);
    DGRP_REQUIRE(h_row_off[0] >= 0, "%s: negative row offset", what);
    pl.tab.assign((size_t)(4 * nrec + 1), 0);
    int64_t *off = pl.tab.data(), *len = off + nrec, *origin = len + nrec, *row_off = origin + nrec;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0 && h_origin[r] >= 0, "%s: negative offset, length or origin (record %lld)", what,
                     (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "%s: row offsets must ascend (record %lld)", what, (long long)r);
        off[r] = h_off[r];
        len[r] = h_len[r];
        origin[r] = h_origin[r];
    }
    for (int64_t r = 0; r <= nrec; ++r) row_off[r] = h_row_off[r];
    pl.nrows = row_off[nrec] - row_off[0];
    for (int k = 0; k < 128; ++k) pl.tot[k] = 0ull;
    if (pl.nrows == 0 || nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_work, "%s: NULL pointer", what);
    if (work_bytes < dgrp_eval_workspace_bytes(nrec, pl.nrows) + extra_bytes) {
        dgrp_set_error("%s: workspace too small", what);
        return DGRP_ENOMEM;
    }
    unsigned long long *g = (unsigned long long *)d_work, *d_tot = (unsigned long long *)((char *)d_work + 1024);
    char *p = (char *)d_work + EVAL_HEAD;
    pl.d_off = (int64_t *)p;
    pl.d_len = pl.d_off + nrec;
    pl.d_origin = pl.d_len + nrec;
    pl.d_row_off = pl.d_origin + nrec;
    p += dgrp_align_up((4 * nrec + 1) * 8, 256);
    pl.d_cl = (uint64_t *)p;
    p += dgrp_align_up((pl.nrows + 1) * 8, 256);
    pl.d_dst = (int64_t *)p;
    p += dgrp_align_up(pl.nrows * 8, 256);
    pl.d_tiles = (uint64_t *)p;
    pl.d_extra = (char *)d_work + dgrp_eval_workspace_bytes(nrec, pl.nrows);
    const unsigned long long init[4] = { 0ull, ~0ull, ~0ull, ~0ull };
    DGRP_HIP(hipMemcpyAsync(g, init, sizeof(init), hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemsetAsync(d_tot, 0, 128 * 8, stream));
    DGRP_HIP(hipMemcpyAsync(pl.d_off, pl.tab.data(), pl.tab.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(eval_check_kernel, dim3((unsigned)((pl.nrows + 255) / 256)), dim3(256), 0, stream, d_rows, pl.d_row_off, nrec,
                       pl.d_len, pl.d_origin, max_label, d_scores, g, d_tot, d_row_key);
    DGRP_LAUNCH_CHECK();
    unsigned long long hg[4];
    DGRP_HIP(hipMemcpyAsync(hg, g, sizeof(hg), hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(pl.tot, d_tot, sizeof(pl.tot), hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    if (hg[0]) {
        const int kind = (hg[0] & 1) ? 1 : (hg[0] & 2) ? 2 : 3;
        const int64_t i = (int64_t)hg[kind];
        dgrp_segment q;
        DGRP_HIP(hipMemcpy(&q, d_rows + i, sizeof(q), hipMemcpyDeviceToHost));
        DGRP_REQUIRE(kind != 2, "%s: row %lld [%lld, %lld) label %d has a base inside its record but no score (scored rows have 0 < "
                     "bases < 2^40, sum <= bases * 2^24, 0 <= agree <= bases)", what, (long long)i, (long long)q.start, (long long)q.end,
                     (int)q.label);
        DGRP_REQUIRE(kind != 3, "%s: row %lld [%lld, %lld) label %d starts below the end of the row in front of it in its record "
                     "(the rows of a record ascend and do not overlap)", what, (long long)i, (long long)q.start, (long long)q.end,
                     (int)q.label);
        DGRP_REQUIRE(!d_row_key, "%s: row %lld [%lld, %lld): rows need 0 <= start <= end and a key below 0xFFFFFFFF", what, (long long)i,
                     (long long)q.start, (long long)q.end);
        DGRP_REQUIRE(false, "%s: row %lld [%lld, %lld) label %d: rows need 0 <= start <= end and 1 <= label <= %d", what, (long long)i,
                     (long long)q.start, (long long)q.end, (int)q.label, max_label);
    }
    return DGRP_OK;
}

// the pass's clipped lengths and first positions, scanned: d_cl[0..nrows] = exclusive scan, d_cl[nrows] = the pass's total
int eval_spans(const eval_plan &pl, const dgrp_segment *d_rows, int64_t nrec, int label, hipStream_t stream)
{
    hipLaunchKernelGGL(eval_span_kernel, dim3((unsigned)((pl.nrows + 255) / 256)), dim3(256), 0, stream, d_rows, pl.d_row_off, nrec,
                       pl.d_off, pl.d_len, pl.d_origin, label, pl.d_cl, pl.d_dst);
    DGRP_LAUNCH_CHECK();
    return device_exclusive_scan(pl.d_cl, pl.d_cl, pl.nrows, pl.d_tiles, pl.d_cl + pl.nrows, stream);
}

DGRP_EXPORT int64_t dgrp_eval_workspace_bytes(int64_t nrec, int64_t nrows)
{
    if (nrec < 0 || nrows < 0) return 0;
    return EVAL_HEAD + dgrp_align_up((4 * nrec + 1) * 8, 256) + dgrp_align_up((nrows + 1) * 8, 256) + dgrp_align_up(nrows * 8, 256) +
           dgrp_align_up(((nrows + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_paint_rows_batch(int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                      const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off, void *d_work,
                                      int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    eval_plan pl;
    const int rc = eval_prepare("dgrp_paint_rows_batch", nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_work, work_bytes, stream, pl);
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_labels, "dgrp_paint_rows_batch: NULL pointer");
    const dgrp_segment *rows = d_rows;
    // one pass per label, highest first: the smallest label covering a base is written last (plain stores, no atomics)
    for (int lab = 127; lab >= 1; --lab) {
        if (pl.tot[lab] == 0) continue;
        const int e = eval_spans(pl, rows, nrec, lab, stream);
        if (e != DGRP_OK) return e;
        const uint64_t groups = (pl.tot[lab] + EVAL_SLICE - 1) / EVAL_SLICE;
        hipLaunchKernelGGL(eval_paint_kernel, dim3((unsigned)groups), dim3(256), 0, stream, d_labels, pl.d_cl, pl.d_dst, pl.nrows, lab);
        DGRP_LAUNCH_CHECK();
    }
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_row_hits_batch(const int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                    const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off, int64_t *d_hits,
                                    void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    eval_plan pl;
    const int rc = eval_prepare("dgrp_row_hits_batch", nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_work, work_bytes, stream, pl);
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_hits, "dgrp_row_hits_batch: NULL pointer");
    const int64_t r0 = h_row_off[0];
    DGRP_HIP(hipMemsetAsync(d_hits + r0, 0, pl.nrows * 8, stream));
    uint64_t total = 0;
    for (int k = 1; k < 128; ++k) total += pl.tot[k];
    if (total == 0) return DGRP_OK;
    DGRP_REQUIRE(d_labels, "dgrp_row_hits_batch: NULL pointer");
    const int e = eval_spans(pl, d_rows, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    hipLaunchKernelGGL(eval_hits_kernel, dim3((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE)), dim3(256), 0, stream, d_labels,
                       pl.d_cl, pl.d_dst, d_rows + r0, pl.nrows, reinterpret_cast<unsigned long long *>(d_hits + r0));
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// predict --bed_dir: per-row statistics of the row's label column of the merged probabilities [*, C] over its clipped span, as exact
// integers (include/deepgrp_hip.h states them).  The same line of positions as the hits above: workgroup b takes positions
// [b * EVAL_SLICE, (b + 1) * EVAL_SLICE) of the scanned clipped lengths, lane-interleaved, so the 64 lanes of a wave read 64
// consecutive rows of the array -- 64 * C * 4 contiguous bytes -- and every lane reads its row whole.
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

// q(p): p * 2^24 rounded half up, clamped to [0, 2^24].  The product is exact in double; so is x + 0.5 except below 2^-30, where
// it stays under 1 and the floor is 0 either way.
__device__ __forceinline__ uint32_t score_q(float p)
{
    if (!(p > 0.0f)) return 0u;
    const double x = (double)p * 16777216.0;
    if (x >= 16777216.0) return 16777216u;
    return (uint32_t)floor(x + 0.5);
}

// one lane per row j, after the scan: bases = its clipped length, qmin = the identity of the minimum when it has bases, the rest 0
__global__ void __launch_bounds__(256) score_init_kernel(const uint64_t *__restrict__ ex, int64_t n, dgrp_row_score *__restrict__ sc)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t cl = ex[j + 1] - ex[j];
    dgrp_row_score v;
    v.sum = 0;
    v.bases = (int64_t)cl;
    v.agree = 0;
    v.qmin = cl ? 0xffffffffu : 0u;
    v.pad = 0;
    sc[j] = v;
}

struct score_acc {
    unsigned long long sum;
    unsigned agree, qmin;
};

// CT: the class count at compile time (0: the runtime value) -- the row's loads are then issued together
template <int CT>
__global__ void __launch_bounds__(256) score_rows_kernel(const float *__restrict__ probs, int Crt, const uint64_t *__restrict__ ex,
                                                         const int64_t *__restrict__ dst, const dgrp_segment *__restrict__ rows,
                                                         int64_t n, dgrp_row_score *__restrict__ sc)
{
    __shared__ unsigned long long s_sum[EVAL_LDS_ROWS];
    __shared__ unsigned s_agree[EVAL_LDS_ROWS], s_min[EVAL_LDS_ROWS];
    __shared__ int64_t s_r0, s_r1;
    const int C = CT ? CT : Crt;
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;    // (s0 < total: the grid covers the line exactly)
    if (threadIdx.x == 0) {
        s_r0 = eval_row_of(ex, 0, n, s0);
        s_r1 = eval_row_of(ex, s_r0, n, s1 - 1);
    }
    for (int k = threadIdx.x; k < EVAL_LDS_ROWS; k += 256) {
        s_sum[k] = 0ull;
        s_agree[k] = 0u;
        s_min[k] = 0xffffffffu;
    }
    __syncthreads();
    const int64_t r0 = s_r0, r1 = s_r1;
    const bool staged = r1 - r0 < EVAL_LDS_ROWS;
    auto flush = [&](int64_t j, const score_acc &a) {
        if (staged) {
            atomicAdd(&s_sum[j - r0], a.sum);
            if (a.agree) atomicAdd(&s_agree[j - r0], a.agree);
            atomicMin(&s_min[j - r0], a.qmin);
        } else {
            atomicAdd(reinterpret_cast<unsigned long long *>(&sc[j].sum), a.sum);
            if (a.agree) atomicAdd(reinterpret_cast<unsigned long long *>(&sc[j].agree), (unsigned long long)a.agree);
            atomicMin(&sc[j].qmin, a.qmin);
        }
    };
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 < s1) {
        int64_t j = eval_row_of(ex, r0, r1 + 1, p0);
        uint64_t jst = ex[j], jend = ex[j + 1];
        int lab = rows[j].label;
        score_acc a = { 0ull, 0u, 0xffffffffu };
        bool any = false;
        for (uint64_t p = p0; p < s1; p += 256) {
            if (jend <= p) {
                if (any) flush(j, a);
                a = { 0ull, 0u, 0xffffffffu };
                any = false;
                while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
                lab = rows[j].label;
            }
            const float *__restrict__ row = probs + (dst[j] + (int64_t)(p - jst)) * C;
            float vbest = row[0], vlab = vbest;
            int best = 0;
#pragma unroll
            for (int c = 1; c < C; ++c) {
                const float v = row[c];
                if (c == lab) vlab = v;
                if (v > vbest) { vbest = v; best = c; }
            }
            const uint32_t q = score_q(vlab);
            a.sum += q;
            a.agree += best == lab ? 1u : 0u;
            a.qmin = q < a.qmin ? q : a.qmin;
            any = true;
        }
        if (any) flush(j, a);
    }
    __syncthreads();
    if (staged) {
        for (int64_t k = threadIdx.x; k <= r1 - r0; k += 256) {
            const unsigned m = s_min[k];
            if (m == 0xffffffffu) continue;                                   // no position of this row in the slice (q <= 2^24)
            atomicAdd(reinterpret_cast<unsigned long long *>(&sc[r0 + k].sum), s_sum[k]);
            if (s_agree[k]) atomicAdd(reinterpret_cast<unsigned long long *>(&sc[r0 + k].agree), (unsigned long long)s_agree[k]);
            atomicMin(&sc[r0 + k].qmin, m);
        }
    }
}

}   // namespace

DGRP_EXPORT int64_t dgrp_row_scores_workspace_bytes(int64_t nrec, int64_t nrows)
{
    return dgrp_eval_workspace_bytes(nrec, nrows);
}

DGRP_EXPORT int dgrp_row_scores_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                      const int64_t *h_startpos, const dgrp_segment *d_rows, const int64_t *h_row_off,
                                      dgrp_row_score *d_scores, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    static_assert(sizeof(dgrp_row_score) == 32, "dgrp_row_score is 32 bytes");
    DGRP_REQUIRE(C >= 2 && C <= DGRP_MAXC, "dgrp_row_scores_batch: 2 <= classes <= 64");
    DGRP_REQUIRE(nrec >= 0 && (nrec == 0 || h_n), "dgrp_row_scores_batch: bad arguments");
    for (int64_t r = 0; r < nrec; ++r)
        DGRP_REQUIRE(h_n[r] >= 1, "dgrp_row_scores_batch: record %lld has no row of probabilities", (long long)r);
    eval_plan pl;
    const int rc = eval_prepare("dgrp_row_scores_batch", nrec, h_row0, h_n, h_startpos, d_rows, h_row_off, d_work, work_bytes, stream, pl,
                                C - 1);
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_scores, "dgrp_row_scores_batch: NULL pointer");
    const int64_t r0 = h_row_off[0];
    uint64_t total = 0;
    for (int k = 1; k < C; ++k) total += pl.tot[k];
    if (total == 0) {
        DGRP_HIP(hipMemsetAsync(d_scores + r0, 0, pl.nrows * sizeof(dgrp_row_score), stream));
        return DGRP_OK;
    }
    DGRP_REQUIRE(d_probs, "dgrp_row_scores_batch: NULL pointer");
    const int e = eval_spans(pl, d_rows, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    hipLaunchKernelGGL(score_init_kernel, dim3((unsigned)((pl.nrows + 255) / 256)), dim3(256), 0, stream, pl.d_cl, pl.nrows, d_scores + r0);
    DGRP_LAUNCH_CHECK();
    const dim3 grid((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE));
    if (C == 5)
        hipLaunchKernelGGL(score_rows_kernel<5>, grid, dim3(256), 0, stream, d_probs, C, pl.d_cl, pl.d_dst, d_rows + r0, pl.nrows, d_scores + r0);
    else
        hipLaunchKernelGGL(score_rows_kernel<0>, grid, dim3(256), 0, stream, d_probs, C, pl.d_cl, pl.d_dst, d_rows + r0, pl.nrows, d_scores + r0);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// evaluate --curves --curve_elements: the detection score of every annotation row -- the largest --bed_min_score at which the
// --min_overlap rule still finds it (include/deepgrp_hip.h states it).  The predicted rows are painted once as 16-bit keys
// (label << 10 | BED score) on the same line of positions as the label paint; the annotation rows then bisect on the score: a pass
// is the walk of eval_hits_kernel with the test "key in [label << 10 | mid, (label + 1) << 10)", a one-lane-per-row kernel between
// the passes moves lo or hi.  The search runs over [-1, 1001) -- -1 ("not found even at 0") holds by definition -- so ten passes
// settle all 1002 outcomes.  Integer adds only: the same bytes on every run.
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

#define DETECT_PASSES 10          // 1002 -> 501 -> 251 -> 126 -> 63 -> 32 -> 16 -> 8 -> 4 -> 2 -> 1

// one lane per row j, after the scan: the key of its bases (0 for a row without a base inside its record: nothing paints it)
__global__ void __launch_bounds__(256) row_key_kernel(const dgrp_segment *__restrict__ rows, const dgrp_row_score *__restrict__ scores,
                                                      const uint64_t *__restrict__ ex, int64_t n, uint16_t *__restrict__ key)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    key[j] = ex[j + 1] > ex[j] ? (uint16_t)((unsigned)rows[j].label << 10 | (unsigned)bed_figures(scores[j]).score) : (uint16_t)0;
}

// eval_paint_kernel with a value per row
__global__ void __launch_bounds__(256) paint_keys_kernel(uint16_t *__restrict__ keys, const uint64_t *__restrict__ ex,
                                                         const int64_t *__restrict__ dst, int64_t n, const uint16_t *__restrict__ key)
{
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 >= s1) return;
    int64_t j = eval_row_of(ex, 0, n, p0);
    uint64_t jst = ex[j], jend = ex[j + 1];
    uint16_t v = key[j];
    for (uint64_t p = p0; p < s1; p += 256) {
        if (jend <= p) {
            while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
            v = key[j];
        }
        keys[dst[j] + (int64_t)(p - jst)] = v;
    }
}

struct detect_state {
    int2 *lohi;                    // the row's detection score lies in [lo, hi)
    unsigned long long *cnt;       // the pass's hits of the row
    uint32_t *thr;                 // label << 10 | the pass's midpoint
};

__device__ __forceinline__ uint32_t detect_thr(int label, int2 s)
{
    const int mid = s.y - s.x > 1 ? (s.x + s.y) >> 1 : (s.x > 0 ? s.x : 0);       // (a settled row's count is not read)
    return (uint32_t)label << 10 | (uint32_t)mid;
}

// one lane per row j, after the scan: [-1, 1001) where the row has a base inside its record and needs one, else settled at -1
__global__ void __launch_bounds__(256) detect_init_kernel(const dgrp_segment *__restrict__ rows, const uint64_t *__restrict__ ex,
                                                          const int64_t *__restrict__ need, int64_t n, detect_state st)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int2 s = make_int2(-1, ex[j + 1] > ex[j] && need[j] > 0 ? 1001 : 0);
    st.lohi[j] = s;
    st.cnt[j] = 0ull;
    st.thr[j] = detect_thr(rows[j].label, s);
}

// cnt[j] += bases of row j's clipped span with a key in [thr[j], (label + 1) << 10): eval_hits_kernel's walk and flush
__global__ void __launch_bounds__(256) detect_walk_kernel(const uint16_t *__restrict__ keys, const uint64_t *__restrict__ ex,
                                                          const int64_t *__restrict__ dst, const uint32_t *__restrict__ thr, int64_t n,
                                                          unsigned long long *__restrict__ hits)
{
    __shared__ unsigned cnt[EVAL_LDS_ROWS];
    __shared__ int64_t s_r0, s_r1;
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;    // (s0 < total: the grid covers the line exactly)
    if (threadIdx.x == 0) {
        s_r0 = eval_row_of(ex, 0, n, s0);
        s_r1 = eval_row_of(ex, s_r0, n, s1 - 1);
    }
    for (int k = threadIdx.x; k < EVAL_LDS_ROWS; k += 256) cnt[k] = 0u;
    __syncthreads();
    const int64_t r0 = s_r0, r1 = s_r1;
    const bool staged = r1 - r0 < EVAL_LDS_ROWS;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 < s1) {
        int64_t j = eval_row_of(ex, r0, r1 + 1, p0);
        uint64_t jst = ex[j], jend = ex[j + 1];
        uint32_t klo = thr[j], width = (((klo >> 10) + 1u) << 10) - klo;
        unsigned c = 0;
        for (uint64_t p = p0; p < s1; p += 256) {
            if (jend <= p) {
                if (c) {
                    if (staged) atomicAdd(&cnt[j - r0], c);
                    else atomicAdd(&hits[j], (unsigned long long)c);
                }
                c = 0;
                while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
                klo = thr[j];
                width = (((klo >> 10) + 1u) << 10) - klo;
            }
            c += (uint32_t)keys[dst[j] + (int64_t)(p - jst)] - klo < width ? 1u : 0u;      // (a key below klo wraps to a large value)
        }
        if (c) {
            if (staged) atomicAdd(&cnt[j - r0], c);
            else atomicAdd(&hits[j], (unsigned long long)c);
        }
    }
    __syncthreads();
    if (staged) {
        for (int64_t k = threadIdx.x; k <= r1 - r0; k += 256) {
            const unsigned v = cnt[k];
            if (v) atomicAdd(&hits[r0 + k], (unsigned long long)v);
        }
    }
}

// one lane per row j between the passes: the midpoint becomes lo where the row still has its hits, else hi; the counter is zeroed
// and the next midpoint set; behind the last pass lo is the detection score
__global__ void __launch_bounds__(256) detect_step_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ need,
                                                          int64_t n, detect_state st, int32_t *__restrict__ detect)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    int2 s = st.lohi[j];
    if (s.y - s.x > 1) {
        const int mid = (s.x + s.y) >> 1;
        if ((long long)st.cnt[j] >= (long long)need[j]) s.x = mid; else s.y = mid;
        st.lohi[j] = s;
    }
    st.cnt[j] = 0ull;
    st.thr[j] = detect_thr(rows[j].label, s);
    if (detect) detect[j] = s.x;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_row_detect_workspace_bytes(int64_t nrec, int64_t nrows)
{
    if (nrec < 0 || nrows < 0) return 0;
    return dgrp_eval_workspace_bytes(nrec, nrows) + 2 * dgrp_align_up(nrows * 8, 256) + dgrp_align_up(nrows * 4, 256);
}

DGRP_EXPORT int dgrp_paint_row_keys_batch(uint16_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                          const int64_t *h_origin, const dgrp_segment *d_pred, const int64_t *h_pred_off,
                                          const dgrp_row_score *d_scores, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_paint_row_keys_batch";
    DGRP_REQUIRE(nrec >= 0 && h_pred_off, "%s: bad arguments", what);
    const int64_t nrows = h_pred_off[nrec] - h_pred_off[0];
    DGRP_REQUIRE(nrows <= 0 || nrec == 0 || d_scores, "%s: NULL pointer", what);
    eval_plan pl;
    const int rc = eval_prepare(what, nrec, h_off, h_len, h_origin, d_pred, h_pred_off, d_work, work_bytes, stream, pl, 63, d_scores,
                                dgrp_row_detect_workspace_bytes(nrec, nrows > 0 ? nrows : 0) - dgrp_eval_workspace_bytes(nrec, nrows > 0 ? nrows : 0));
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    uint64_t total = 0;
    for (int k = 1; k < 64; ++k) total += pl.tot[k];
    if (total == 0) return DGRP_OK;
    DGRP_REQUIRE(d_keys && ((uintptr_t)d_keys & 1) == 0, "%s: the key track must be a 2-byte aligned device pointer", what);
    const int64_t r0 = h_pred_off[0];
    const int e = eval_spans(pl, d_pred, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    uint16_t *d_key = (uint16_t *)pl.d_extra;
    hipLaunchKernelGGL(row_key_kernel, dim3((unsigned)((pl.nrows + 255) / 256)), dim3(256), 0, stream, d_pred + r0, d_scores + r0, pl.d_cl,
                       pl.nrows, d_key);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(paint_keys_kernel, dim3((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE)), dim3(256), 0, stream, d_keys, pl.d_cl,
                       pl.d_dst, pl.nrows, d_key);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_row_detect_batch(const uint16_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                      const int64_t *h_origin, const dgrp_segment *d_true, const int64_t *h_true_off,
                                      const int64_t *d_need, int32_t *d_detect, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_row_detect_batch";
    DGRP_REQUIRE(nrec >= 0 && h_true_off, "%s: bad arguments", what);
    const int64_t nrows = h_true_off[nrec] - h_true_off[0];
    eval_plan pl;
    const int rc = eval_prepare(what, nrec, h_off, h_len, h_origin, d_true, h_true_off, d_work, work_bytes, stream, pl, 63, nullptr,
                                dgrp_row_detect_workspace_bytes(nrec, nrows > 0 ? nrows : 0) - dgrp_eval_workspace_bytes(nrec, nrows > 0 ? nrows : 0));
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_detect && d_need, "%s: NULL pointer", what);
    const int64_t r0 = h_true_off[0];
    uint64_t total = 0;
    for (int k = 1; k < 64; ++k) total += pl.tot[k];
    if (total == 0) {                                                         // no row has a base inside its record: all -1
        DGRP_HIP(hipMemsetAsync(d_detect + r0, 0xff, pl.nrows * sizeof(int32_t), stream));
        return DGRP_OK;
    }
    DGRP_REQUIRE(d_keys && ((uintptr_t)d_keys & 1) == 0, "%s: the key track must be a 2-byte aligned device pointer", what);
    const int e = eval_spans(pl, d_true, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    detect_state st;
    st.cnt = (unsigned long long *)pl.d_extra;
    st.lohi = (int2 *)(pl.d_extra + dgrp_align_up(pl.nrows * 8, 256));
    st.thr = (uint32_t *)(pl.d_extra + 2 * dgrp_align_up(pl.nrows * 8, 256));
    const dim3 per_row((unsigned)((pl.nrows + 255) / 256)), per_slice((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE));
    hipLaunchKernelGGL(detect_init_kernel, per_row, dim3(256), 0, stream, d_true + r0, pl.d_cl, d_need + r0, pl.nrows, st);
    DGRP_LAUNCH_CHECK();
    for (int pass = 0; pass < DETECT_PASSES; ++pass) {
        hipLaunchKernelGGL(detect_walk_kernel, per_slice, dim3(256), 0, stream, d_keys, pl.d_cl, pl.d_dst, st.thr, pl.nrows, st.cnt);
        DGRP_LAUNCH_CHECK();
        hipLaunchKernelGGL(detect_step_kernel, per_row, dim3(256), 0, stream, d_true + r0, d_need + r0, pl.nrows, st,
                           pass == DETECT_PASSES - 1 ? d_detect + r0 : (int32_t *)nullptr);
        DGRP_LAUNCH_CHECK();
    }
    return DGRP_OK;
}
