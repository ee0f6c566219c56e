// evaluate --boundaries: how well a found element is delimited.  Per row of one track against the label track of the other: the
// hits of dgrp_row_hits_batch, the runs of the row's label under it, the first and last matching base, and how far the label runs
// on beyond the row's two ends (at most W bases, never beyond the row's record) -- dgrp_row_bounds_batch; and the three small
// tables `evaluate` sums over its work items from those rows -- dgrp_bound_hist_batch.  include/deepgrp_hip.h states both.
//
// The walk is the "line of positions" of eval_kernels.hip over WIDENED spans: row j contributes its left flank, its clipped span
// and its right flank, wl + cl + wr positions; an exclusive scan places it on the line and workgroup b takes positions
// [b * EVAL_SLICE, (b + 1) * EVAL_SLICE), lane-interleaved.  Integer adds, minima and maxima only: the bytes do not depend on the
// grid, the timing or the order.
#include "dgrp_common.h"
#include "eval_rows.h"

namespace {

#define BOUNDS_LDS_ROWS 1024      // the slice's rows with their six counters in LDS (24 KiB); a slice crossing more goes to d_bounds directly
#define BOUNDS_MAX_W 4096
#define BOUNDS_NONE 0xffffffffu

// one lane per row j (= row row_off[0] + j), before the pass: its flanks, its width on the line, the buffer position of the first base
// of its left flank, and the identities of the six reductions.  Between this kernel and bounds_finish_kernel the fields of out[j]
// hold: hits, runs the sums; first = the smallest matching base counted from the clipped start (identity: all ones); last = the
// largest such + 1 (0); lead = the largest non-matching position of the left flank, counted from the flank's first base (-1);
// trail = the smallest non-matching position of the right flank, counted from the clipped end (wr)
__global__ void __launch_bounds__(256) bounds_span_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                          int64_t nrec, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                          const int64_t *__restrict__ origin, int W, uint64_t *__restrict__ width,
                                                          int64_t *__restrict__ dst, int2 *__restrict__ flank,
                                                          dgrp_row_bound *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = row_off[0] + j;
    if (i >= row_off[nrec]) return;
    const int64_t r = dgrp_record_of(row_off, nrec, i);
    int64_t cs, cl;
    eval_clip(rows[i], origin[r], len[r], cs, cl);
    const int64_t room = len[r] - cs - cl;                               // bases of the record behind the clipped end
    const int wl = cl ? (int)(cs < W ? cs : W) : 0, wr = cl ? (int)(room < W ? room : W) : 0;
    width[j] = (uint64_t)(wl + cl + wr);
    dst[j] = off[r] + cs - wl;
    flank[j] = make_int2(wl, wr);
    dgrp_row_bound v;
    v.hits = 0;
    v.runs = 0;
    v.first = -1;
    v.last = 0;
    v.lead = -1;
    v.trail = wr;
    out[i] = v;
}

// one lane per row, behind the pass: the reductions become the stated outputs
__global__ void __launch_bounds__(256) bounds_finish_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                            int64_t nrec, const int64_t *__restrict__ len,
                                                            const int64_t *__restrict__ origin, const int2 *__restrict__ flank,
                                                            dgrp_row_bound *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = row_off[0] + j;
    if (i >= row_off[nrec]) return;
    const int64_t r = dgrp_record_of(row_off, nrec, i);
    int64_t cs, cl;
    eval_clip(rows[i], origin[r], len[r], cs, cl);
    const int64_t a = origin[r] + cs;
    dgrp_row_bound v = out[i];
    v.first = v.hits ? a + v.first : -1;
    v.last = v.hits ? a + v.last - 1 : -1;
    v.lead = flank[j].x - 1 - v.lead;
    out[i] = v;
}

struct bounds_acc {
    unsigned hits, runs;
    unsigned first, last;          // slice positions of matching bases of the clipped span: the smallest (NONE), the largest + 1 (0)
    unsigned lstop, rstop;         // non-matching flank positions: left the largest + 1 (0), right the smallest (NONE)
};

__device__ __forceinline__ bounds_acc bounds_identity()
{
    return { 0u, 0u, BOUNDS_NONE, 0u, 0u, BOUNDS_NONE };
}

// what a lane (or the slice's LDS counters) holds for row j goes onto the row; s0: the slice's first position, jst: the row's
__device__ __forceinline__ void bounds_commit(dgrp_row_bound *__restrict__ o, const bounds_acc &a, uint64_t s0, uint64_t jst, int wl)
{
    if (a.hits) atomicAdd(reinterpret_cast<unsigned long long *>(&o->hits), (unsigned long long)a.hits);
    if (a.runs) atomicAdd(reinterpret_cast<unsigned long long *>(&o->runs), (unsigned long long)a.runs);
    if (a.first != BOUNDS_NONE) atomicMin(reinterpret_cast<unsigned long long *>(&o->first), (unsigned long long)(s0 + a.first - jst - wl));
    if (a.last) atomicMax(reinterpret_cast<unsigned long long *>(&o->last), (unsigned long long)(s0 + a.last - jst - wl));
    if (a.lstop) atomicMax(&o->lead, (int)a.lstop - 1);
    if (a.rstop != BOUNDS_NONE) atomicMin(&o->trail, (int)a.rstop);
}

// the pass.  A lane's positions are 256 apart; the 64 lanes of a wave read 64 adjacent bytes.  Whether base b - 1 matches -- the
// start of a run -- is the previous lane's answer of the same iteration (one __shfl_up: b - 1 lies in the same row's clipped span
// whenever it is asked for); lane 0 of a wave reads that byte itself.  The loop's trip count is the workgroup's, so every wave
// reaches the shuffle whole.
__global__ void __launch_bounds__(256) row_bounds_kernel(const int8_t *__restrict__ labels, const uint64_t *__restrict__ ex,
                                                         const int64_t *__restrict__ dst, const dgrp_segment *__restrict__ rows,
                                                         const int2 *__restrict__ flank, int64_t n, dgrp_row_bound *__restrict__ out)
{
    __shared__ unsigned s_hits[BOUNDS_LDS_ROWS], s_runs[BOUNDS_LDS_ROWS], s_first[BOUNDS_LDS_ROWS], s_last[BOUNDS_LDS_ROWS],
        s_lstop[BOUNDS_LDS_ROWS], s_rstop[BOUNDS_LDS_ROWS];
    __shared__ int64_t s_r0, s_r1;
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    if (s0 >= total) return;                                                  // (the grid is sized from a bound on the line's length)
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;
    if (threadIdx.x == 0) {
        s_r0 = eval_row_of(ex, 0, n, s0);
        s_r1 = eval_row_of(ex, s_r0, n, s1 - 1);
    }
    for (int k = threadIdx.x; k < BOUNDS_LDS_ROWS; k += 256) {
        s_hits[k] = s_runs[k] = s_last[k] = s_lstop[k] = 0u;
        s_first[k] = s_rstop[k] = BOUNDS_NONE;
    }
    __syncthreads();
    const int64_t r0 = s_r0, r1 = s_r1;
    const bool staged = r1 - r0 < BOUNDS_LDS_ROWS;
    const int lane = threadIdx.x & 63;
    int64_t j = 0, jdst = 0;
    uint64_t jst = 0, jend = 0, core_end = 0;                                 // core_end: wl + the clipped length
    int lab = 0, wl = 0;
    bounds_acc a = bounds_identity();
    auto flush = [&]() {
        if (staged) {
            const int64_t k = j - r0;
            if (a.hits) atomicAdd(&s_hits[k], a.hits);
            if (a.runs) atomicAdd(&s_runs[k], a.runs);
            if (a.first != BOUNDS_NONE) atomicMin(&s_first[k], a.first);
            if (a.last) atomicMax(&s_last[k], a.last);
            if (a.lstop) atomicMax(&s_lstop[k], a.lstop);
            if (a.rstop != BOUNDS_NONE) atomicMin(&s_rstop[k], a.rstop);
        } else {
            bounds_commit(out + j, a, s0, jst, wl);
        }
        a = bounds_identity();
    };
    auto enter = [&]() {                                                      // row j's constants, ex[j] <= p < ex[j + 1]
        const int2 f = flank[j];
        wl = f.x;
        core_end = jend - jst - (uint64_t)f.y;
        lab = rows[j].label;
        jdst = dst[j];
    };
    const bool any = s0 + threadIdx.x < s1;
    if (any) {
        j = eval_row_of(ex, r0, r1 + 1, s0 + threadIdx.x);
        jst = ex[j];
        jend = ex[j + 1];
        enter();
    }
    for (uint64_t base = s0; base < s1; base += 256) {
        const uint64_t p = base + threadIdx.x;
        const bool live = p < s1;
        uint64_t idx = 0;
        int64_t pos = 0;
        int m = 0;
        if (live) {
            if (jend <= p) {
                flush();
                while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
                enter();
            }
            idx = p - jst;
            pos = jdst + (int64_t)idx;
            m = labels[pos] == lab ? 1 : 0;
        }
        int before = __shfl_up(m, 1);
        if (live) {
            if (idx < (uint64_t)wl) {
                if (!m) a.lstop = (unsigned)idx + 1u;                         // (a lane's positions ascend: the last one is the largest)
            } else if (idx < core_end) {
                if (m) {
                    const unsigned q = (unsigned)(p - s0);
                    ++a.hits;
                    if (a.first == BOUNDS_NONE) a.first = q;
                    a.last = q + 1u;
                    if (idx == (uint64_t)wl) {
                        ++a.runs;
                    } else {
                        if (lane == 0) before = labels[pos - 1] == lab ? 1 : 0;
                        if (!before) ++a.runs;
                    }
                }
            } else if (!m) {
                const unsigned t = (unsigned)(idx - core_end);
                if (t < a.rstop) a.rstop = t;
            }
        }
    }
    if (any) flush();
    __syncthreads();
    if (staged) {
        for (int64_t k = threadIdx.x; k <= r1 - r0; k += 256) {
            const bounds_acc v = { s_hits[k], s_runs[k], s_first[k], s_last[k], s_lstop[k], s_rstop[k] };
            if (v.hits | v.lstop | (v.rstop != BOUNDS_NONE ? 1u : 0u)) bounds_commit(out + r0 + k, v, s0, ex[r0 + k], flank[r0 + k].x);
        }
    }
}

#define BH_FRAG 17
#define BH_LDS_CELLS 16384            // 64 KiB of 32-bit counters: frag and tally always, the edge offsets where they fit beside them

// one lane per row, grid-stride: frag, tally and (where they fit) the edge offsets in 32-bit LDS counters -- a workgroup sees fewer
// than 2^32 rows --, flushed with one 64-bit atomic per non-zero cell
__global__ void __launch_bounds__(256) bound_hist_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                         int64_t nrec, const int64_t *__restrict__ len,
                                                         const int64_t *__restrict__ origin, const dgrp_row_bound *__restrict__ bounds,
                                                         const int64_t *__restrict__ need, int C, int W, int edge_in_lds,
                                                         unsigned long long *__restrict__ frag, unsigned long long *__restrict__ edge,
                                                         unsigned long long *__restrict__ tally, int *__restrict__ bad)
{
    extern __shared__ unsigned bh_cnt[];
    const int E = 2 * W + 1, nfrag = C * BH_FRAG, ntally = C * 2, nedge = edge_in_lds ? C * 2 * E : 0;
    unsigned *s_frag = bh_cnt, *s_tally = s_frag + nfrag, *s_edge = s_tally + ntally;
    for (int k = threadIdx.x; k < nfrag + ntally + nedge; k += 256) bh_cnt[k] = 0u;
    __syncthreads();
    const int64_t first_row = row_off[0], end_row = row_off[nrec];
    for (int64_t i = first_row + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end_row; i += (int64_t)gridDim.x * 256) {
        const dgrp_segment q = rows[i];
        const int64_t r = dgrp_record_of(row_off, nrec, i);
        const int64_t o = origin[r], n = len[r];
        int64_t cs, cl;
        eval_clip(q, o, n, cs, cl);
        if (cl == 0) continue;
        if ((unsigned)q.label >= (unsigned)C) { *bad = 1; continue; }
        const int L = q.label;
        const dgrp_row_bound b = bounds[i];
        const int64_t a = o + cs, e = a + cl, runs = b.runs < BH_FRAG - 1 ? (b.runs < 0 ? 0 : b.runs) : BH_FRAG - 1;
        atomicAdd(&s_frag[L * BH_FRAG + (int)runs], 1u);
        const int64_t nd = need[i];
        if (!(nd > 0 && b.hits >= nd)) continue;
        const int64_t ds = b.first > a ? (b.first - a < W ? b.first - a : W) : -(int64_t)b.lead;
        const int64_t de = b.last + 1 < e ? -(e - 1 - b.last < W ? e - 1 - b.last : W) : (int64_t)b.trail;
        if (ds < -W || ds > W || de < -W || de > W) { *bad = 1; continue; }  // (bounds taken with another W)
        atomicAdd(&s_tally[L * 2], 1u);
        const bool cut_start = q.start < o, cut_end = q.end > o + n;
        if (!cut_start) {
            const int cell = (L * 2 + 0) * E + (int)ds + W;
            if (edge_in_lds) atomicAdd(&s_edge[cell], 1u); else atomicAdd(&edge[cell], 1ull);
        }
        if (!cut_end) {
            const int cell = (L * 2 + 1) * E + (int)de + W;
            if (edge_in_lds) atomicAdd(&s_edge[cell], 1u); else atomicAdd(&edge[cell], 1ull);
        }
        if (!cut_start && !cut_end && ds == 0 && de == 0) atomicAdd(&s_tally[L * 2 + 1], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nfrag; k += 256)
        if (s_frag[k]) atomicAdd(&frag[k], (unsigned long long)s_frag[k]);
    for (int k = threadIdx.x; k < ntally; k += 256)
        if (s_tally[k]) atomicAdd(&tally[k], (unsigned long long)s_tally[k]);
    for (int k = threadIdx.x; k < nedge; k += 256)
        if (s_edge[k]) atomicAdd(&edge[k], (unsigned long long)s_edge[k]);
}

}   // namespace

DGRP_EXPORT int64_t dgrp_row_bounds_workspace_bytes(int64_t nrec, int64_t nrows)
{
    if (nrec < 0 || nrows < 0) return 0;
    return dgrp_eval_workspace_bytes(nrec, nrows) + dgrp_align_up(nrows * 8, 256);
}

DGRP_EXPORT int dgrp_row_bounds_batch(const int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                      const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off, int W,
                                      dgrp_row_bound *d_bounds, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_row_bounds_batch";
    static_assert(sizeof(dgrp_row_bound) == 40, "dgrp_row_bound is 40 bytes");
    DGRP_REQUIRE(W >= 0 && W <= BOUNDS_MAX_W, "%s: 0 <= W <= %d", what, BOUNDS_MAX_W);
    DGRP_REQUIRE(nrec >= 0 && h_row_off, "%s: bad arguments", what);
    const int64_t nrows = h_row_off[nrec] - h_row_off[0];
    eval_plan pl;
    const int rc = eval_prepare(what, nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_work, work_bytes, stream, pl, 127, nullptr,
                                dgrp_align_up((nrows > 0 ? nrows : 0) * 8, 256));
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_bounds && ((uintptr_t)d_bounds & 7) == 0, "%s: the bounds are NULL or not 8-byte aligned", what);
    const int64_t r0 = h_row_off[0];
    uint64_t total = 0;
    for (int k = 1; k < 128; ++k) total += pl.tot[k];
    DGRP_REQUIRE(total == 0 || d_labels, "%s: NULL pointer", what);
    int2 *d_flank = (int2 *)pl.d_extra;
    const dim3 per_row((unsigned)((pl.nrows + 255) / 256));
    hipLaunchKernelGGL(bounds_span_kernel, per_row, dim3(256), 0, stream, d_rows, pl.d_row_off, nrec, pl.d_off, pl.d_len, pl.d_origin, W,
                       pl.d_cl, pl.d_dst, d_flank, d_bounds);
    DGRP_LAUNCH_CHECK();
    if (total) {
        const int e = device_exclusive_scan(pl.d_cl, pl.d_cl, pl.nrows, pl.d_tiles, pl.d_cl + pl.nrows, stream);
        if (e != DGRP_OK) return e;
        // the line is at most this long (the flanks of rows at a record's edge are shorter): workgroups behind its end return at once
        const uint64_t bound = total + 2ull * (uint64_t)W * (uint64_t)pl.nrows;
        const uint64_t groups = (bound + EVAL_SLICE - 1) / EVAL_SLICE;
        DGRP_REQUIRE(groups < (1ull << 31), "%s: too long", what);
        hipLaunchKernelGGL(row_bounds_kernel, dim3((unsigned)groups), dim3(256), 0, stream, d_labels, pl.d_cl, pl.d_dst, d_rows + r0, d_flank,
                           pl.nrows, d_bounds + r0);
        DGRP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bounds_finish_kernel, per_row, dim3(256), 0, stream, d_rows, pl.d_row_off, nrec, pl.d_len, pl.d_origin, d_flank,
                       d_bounds);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_bound_hist_workspace_bytes(int64_t nrec)
{
    if (nrec < 0 || nrec >= (1ll << 40)) return 0;
    return dgrp_align_up((3 * nrec + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_bound_hist_batch(int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                                      const dgrp_segment *d_rows, const int64_t *h_row_off, const dgrp_row_bound *d_bounds,
                                      const int64_t *d_need, int C, int W, int64_t *d_frag, int64_t *d_edge, int64_t *d_tally, int *d_bad,
                                      void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_bound_hist_batch";
    DGRP_REQUIRE(C >= 2 && C <= DGRP_MAXC, "%s: 2 <= classes <= 64", what);
    DGRP_REQUIRE(W >= 0 && W <= BOUNDS_MAX_W, "%s: 0 <= W <= %d", what, BOUNDS_MAX_W);
    DGRP_REQUIRE(nrec >= 0 && nrec < (1ll << 28) && h_row_off && (nrec == 0 || (h_off && h_len && h_origin)), "%s: bad arguments", what);
    DGRP_REQUIRE(d_frag && d_edge && d_tally && d_bad, "%s: NULL pointer", what);
    DGRP_REQUIRE((((uintptr_t)d_frag | (uintptr_t)d_edge | (uintptr_t)d_tally) & 7) == 0, "%s: the counts must be 8-byte aligned", what);
    DGRP_REQUIRE(h_row_off[0] >= 0, "%s: negative row offset", what);
    std::vector<int64_t> tab((size_t)(3 * nrec + 1), 0);
    int64_t *len = tab.data(), *origin = len + nrec, *row_off = origin + nrec;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0 && h_origin[r] >= 0, "%s: negative offset, length or origin (record %lld)", what,
                     (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "%s: row offsets must ascend (record %lld)", what, (long long)r);
        len[r] = h_len[r];
        origin[r] = h_origin[r];
    }
    for (int64_t r = 0; r <= nrec; ++r) row_off[r] = h_row_off[r];
    const int64_t nrows = row_off[nrec] - row_off[0];
    const int E = 2 * W + 1;
    DGRP_HIP(hipMemsetAsync(d_frag, 0, sizeof(int64_t) * C * BH_FRAG, stream));
    DGRP_HIP(hipMemsetAsync(d_edge, 0, sizeof(int64_t) * C * 2 * E, stream));
    DGRP_HIP(hipMemsetAsync(d_tally, 0, sizeof(int64_t) * C * 2, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
    if (nrows == 0 || nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_bounds && d_need && d_work, "%s: NULL pointer", what);
    DGRP_REQUIRE(nrows < (1ll << 31), "%s: too many rows", what);
    if (work_bytes < dgrp_bound_hist_workspace_bytes(nrec)) {
        dgrp_set_error("%s: workspace too small", what);
        return DGRP_ENOMEM;
    }
    int64_t *d_tab = (int64_t *)d_work;
    DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    const int small = C * (BH_FRAG + 2);
    const int edge_in_lds = small + C * 2 * E <= BH_LDS_CELLS ? 1 : 0;
    const size_t lds = (size_t)(small + (edge_in_lds ? C * 2 * E : 0)) * 4;
    hipLaunchKernelGGL(bound_hist_kernel, dim3((unsigned)grid_for(nrows, 256, 256)), dim3(256), lds, stream, d_rows, d_tab + 2 * nrec, nrec,
                       d_tab, d_tab + nrec, d_bounds, d_need, C, W, edge_in_lds, reinterpret_cast<unsigned long long *>(d_frag),
                       reinterpret_cast<unsigned long long *>(d_edge), reinterpret_cast<unsigned long long *>(d_tally), d_bad);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
