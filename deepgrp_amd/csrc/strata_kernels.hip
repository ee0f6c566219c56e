// evaluate --strata: where does a model lose elements -- the truth track that knows WHICH element won each base, and the histogram
// of the true class's probability split by that (include/deepgrp_hip.h states both).
//
// dgrp_paint_strata_batch.  key = label << 8 | stratum, 0xFFFFFFFF where no row covers the base.  A base takes the SMALLEST key among
// the rows that cover it: the label dgrp_paint_rows_batch paints there, and the lowest stratum among that label's rows.  A minimum
// does not depend on order: the track is filled with ones, then ONE pass over the line of positions of all rows (the scan of the
// clipped lengths, 8192 positions a workgroup, lane-interleaved as eval_paint_kernel) does a 32-bit atomicMin per position.  The rows
// are checked by the kernel under dgrp_paint_rows_batch (eval_rows.h) before a byte is written.
// dgrp_paint_keys_batch (evaluate --offtarget) is the same body with a key of the caller's per row: the label is not read there.
//
// dgrp_prob_hist_strata_batch.  A cell is a (class, stratum) pair, `bins` 32-bit counters in LDS.  Where C * S * bins counters do not
// fit the 160 KiB prob_hist_kernels.hip uses, the cells are cut into groups of G = 40960 / bins along grid.y; every group reads the
// 4 bytes of key of every base and the one float P[b, t] of the bases whose cell it owns.  A wave takes 64 consecutive bases: the keys
// are one coalesced load, and neighbours mostly share an element and -- under a trained model -- a bin, so the wave first peels the
// counter of its first pending lane with a ballot (one ds_add of the popcount instead of 64 serialised ones on one word), twice, and
// only what is left adds by itself.  Integer sums whatever the order: a workgroup counts fewer than 2^32 bases (the grid is sized
// for it), and every non-zero word goes to d_hist with one 64-bit atomic add.
#include "eval_rows.h"
#include <mutex>

namespace {

#define SH_THREADS 256
#define SH_ROWS 4096                  // bases of a tile
#define SH_LDS (160 * 1024)           // the budget of prob_hist_kernels.hip
#define SH_MAX_TILES (1 << 19)        // tiles per workgroup: 2^19 * SH_ROWS = 2^31 bases
#define SH_NONE 0xFFFFFFFFu

// the key of row j: its own (dgrp_paint_keys_batch: the label is not read), or label << 8 | stratum
__device__ __forceinline__ unsigned strata_key_of(const dgrp_segment *__restrict__ rows, const uint8_t *__restrict__ stratum,
                                                  const unsigned *__restrict__ row_key, int64_t j)
{
    return row_key ? row_key[j] : ((unsigned)rows[j].label << 8 | stratum[j]);
}

// every position of the slice: keys[its base] = min(keys[its base], the key of its row)
__global__ void __launch_bounds__(256) strata_paint_kernel(unsigned *__restrict__ keys, const uint64_t *__restrict__ ex,
                                                           const int64_t *__restrict__ dst, const dgrp_segment *__restrict__ rows,
                                                           const uint8_t *__restrict__ stratum, const unsigned *__restrict__ row_key,
                                                           int64_t n)
{
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 >= s1) return;
    int64_t j = eval_row_of(ex, 0, n, p0);
    uint64_t jst = ex[j], jend = ex[j + 1];
    unsigned key = strata_key_of(rows, stratum, row_key, j);
    for (uint64_t p = p0; p < s1; p += 256) {
        if (jend <= p) {
            while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
            key = strata_key_of(rows, stratum, row_key, j);
        }
        atomicMin(&keys[dst[j] + (int64_t)(p - jst)], key);
    }
}

struct sh_args {
    const float *probs;
    const unsigned *keys;
    const int64_t *tcum, *row0, *len, *off;   // workspace tables: tiles before record r [nrec + 1], then the caller's three
    int64_t nrec;
    int C, S, bins, G, cells;
    float fbins;
    unsigned long long *hist;
    int *bad;
};

__global__ void __launch_bounds__(SH_THREADS) strata_hist_kernel(sh_args a)
{
    extern __shared__ __align__(16) unsigned sh_cnt[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.y * a.G, G = a.cells - c0 < a.G ? a.cells - c0 : a.G;
    const int words = G * a.bins;
    for (int i = tid; i < words; i += SH_THREADS) sh_cnt[i] = 0u;
    __syncthreads();
    const int64_t tiles = a.tcum[a.nrec];
    int64_t r = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        {   // the record of tile t (uniform: tiles ascend, so the search starts at the last record)
            int64_t lo = r, hi = a.nrec;
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (a.tcum[mid] <= t) lo = mid;
                else hi = mid;
            }
            r = lo;
        }
        const int64_t lt = (t - a.tcum[r]) * SH_ROWS, left = a.len[r] - lt;
        const int nr = (int)(left < SH_ROWS ? left : SH_ROWS);
        const unsigned *kp = a.keys + a.off[r] + lt;
        const float *pp = a.probs + (a.row0[r] + lt) * a.C;
        for (int j0 = 0; j0 < nr; j0 += SH_THREADS) {                 // (uniform bounds: whole waves reach the ballots)
            const int j = j0 + tid;
            int w = -1;
            if (j < nr) {
                const unsigned key = kp[j];
                if (key != SH_NONE) {
                    const unsigned cls = key >> 8, s = key & 255u;
                    if (cls >= (unsigned)a.C || s >= (unsigned)a.S) {
                        *a.bad = 1;
                    } else {
                        const int cell = (int)cls * a.S + (int)s - c0;
                        if ((unsigned)cell < (unsigned)G) {
                            const float p = pp[(int64_t)j * a.C + cls];
                            if (!(p >= 0.0f && p <= 1.0f)) {
                                *a.bad = 1;
                            } else {
                                int k = (int)(p * a.fbins);
                                k = k < a.bins - 1 ? k : a.bins - 1;
                                w = cell * a.bins + k;
                            }
                        }
                    }
                }
            }
            bool todo = w >= 0;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const unsigned long long act = __ballot(todo);
                if (!act) break;
                const int leader = __ffsll(act) - 1;
                const int wl = __shfl(w, leader, 64);
                const bool mine = todo && w == wl;
                const unsigned long long same = __ballot(mine);
                if (lane == leader) atomicAdd(&sh_cnt[wl], (unsigned)__popcll(same));
                if (mine) todo = false;
            }
            if (todo) atomicAdd(&sh_cnt[w], 1u);
        }
    }
    __syncthreads();
    unsigned long long *out = a.hist + (int64_t)c0 * a.bins;
    for (int i = tid; i < words; i += SH_THREADS) {
        const unsigned v = sh_cnt[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
}

}   // namespace

namespace {

// both paints: the fill, then one pass of atomic minima.  d_row_key NULL: the strata paint (label << 8 | stratum, labels 1..63 checked);
// else the keys are the rows' own and the label is not read.
int strata_paint_run(const char *what, uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                     const dgrp_segment *d_rows, const int64_t *h_row_off, const uint8_t *d_row_stratum, const uint32_t *d_row_key,
                     bool own_keys, void *d_work, int64_t work_bytes, hipStream_t stream)
{
    DGRP_REQUIRE(nrec >= 0 && h_off, "%s: bad arguments", what);
    DGRP_REQUIRE(h_off[nrec] >= 0 && h_off[nrec] < (1ll << 40), "%s: a track of %lld keys", what, (long long)h_off[nrec]);
    for (int64_t r = 0; r < nrec; ++r)
        DGRP_REQUIRE(h_len && h_off[r] >= 0 && h_len[r] >= 0 && h_len[r] <= h_off[nrec] && h_off[r] <= h_off[nrec] - h_len[r],
                     "%s: record %lld does not lie in the track of %lld keys", what, (long long)r, (long long)h_off[nrec]);
    eval_plan pl;
    DGRP_REQUIRE(!own_keys || d_row_key || !h_row_off || h_row_off[nrec] == h_row_off[0], "%s: NULL keys", what);
    const int rc = eval_prepare(what, nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_work, work_bytes, stream, pl, 63, nullptr, 0,
                                own_keys ? d_row_key : nullptr);
    if (rc != DGRP_OK) return rc;
    const int64_t n = h_off[nrec];
    if (n == 0) return DGRP_OK;
    DGRP_REQUIRE(d_keys && ((uintptr_t)d_keys & 3) == 0, "%s: the track is NULL or not 4-byte aligned", what);
    DGRP_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)n * 4, stream));
    uint64_t total = 0;
    for (int k = 1; k < 128; ++k) total += pl.tot[k];
    if (pl.nrows == 0 || nrec == 0 || total == 0) return DGRP_OK;
    DGRP_REQUIRE(own_keys || d_row_stratum, "%s: NULL strata", what);
    const int e = eval_spans(pl, d_rows, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    const int64_t r0 = h_row_off[0];
    hipLaunchKernelGGL(strata_paint_kernel, dim3((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE)), dim3(256), 0, stream, d_keys, pl.d_cl,
                       pl.d_dst, d_rows + r0, own_keys ? (const uint8_t *)nullptr : d_row_stratum + r0,
                       own_keys ? d_row_key + r0 : (const uint32_t *)nullptr, pl.nrows);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

}   // namespace

DGRP_EXPORT int dgrp_paint_strata_batch(uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                        const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off,
                                        const uint8_t *d_row_stratum, void *d_work, int64_t work_bytes, void *stream_)
{
    return strata_paint_run("dgrp_paint_strata_batch", d_keys, nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_row_stratum, nullptr, false,
                            d_work, work_bytes, (hipStream_t)stream_);
}

DGRP_EXPORT int dgrp_paint_keys_batch(uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                                      const dgrp_segment *d_rows, const int64_t *h_row_off, const uint32_t *d_row_key, void *d_work,
                                      int64_t work_bytes, void *stream_)
{
    return strata_paint_run("dgrp_paint_keys_batch", d_keys, nrec, h_off, h_len, h_origin, d_rows, h_row_off, nullptr, d_row_key, true,
                            d_work, work_bytes, (hipStream_t)stream_);
}

DGRP_EXPORT int64_t dgrp_prob_hist_strata_workspace_bytes(int64_t nrec)
{
    if (nrec < 0 || nrec >= (1ll << 28)) return 0;
    return dgrp_align_up((4 * nrec + 1) * 8, 256) + 256;
}

DGRP_EXPORT int dgrp_prob_hist_strata_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                            const uint32_t *d_keys, const int64_t *h_off, int S, int bins, int64_t *d_hist, int *d_bad,
                                            void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_prob_hist_strata_batch";
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "%s: 1 <= classes <= 64", what);
    DGRP_REQUIRE(S >= 1 && S <= 256, "%s: 1 <= strata <= 256", what);
    DGRP_REQUIRE(bins >= 2 && bins <= 1000, "%s: 2 <= bins <= 1000", what);
    DGRP_REQUIRE(nrec >= 0 && d_hist && d_bad && (nrec == 0 || (h_row0 && h_n && h_off)), "%s: bad arguments", what);
    DGRP_REQUIRE(((uintptr_t)d_hist & 7) == 0, "%s: the histogram must be 8-byte aligned", what);
    DGRP_REQUIRE(nrec < (1ll << 28), "%s: too many records", what);
    std::vector<int64_t> tab((size_t)(4 * nrec + 1), 0);
    int64_t *tcum = tab.data(), *row0 = tcum + nrec + 1, *len = row0 + nrec, *off = len + nrec;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_row0[r] >= 0 && h_n[r] >= 0 && h_off[r] >= 0, "%s: negative offset, length or origin (record %lld)", what, (long long)r);
        DGRP_REQUIRE(h_row0[r] < (1ll << 40) && h_n[r] < (1ll << 40) && h_off[r] < (1ll << 40), "%s: too long (record %lld)", what, (long long)r);
        tcum[r + 1] = tcum[r] + (h_n[r] + SH_ROWS - 1) / SH_ROWS;
        row0[r] = h_row0[r];
        len[r] = h_n[r];
        off[r] = h_off[r];
    }
    const int64_t tiles = tcum[nrec];
    if (tiles) {
        DGRP_REQUIRE(d_probs && d_keys && d_work, "%s: NULL pointer", what);
        DGRP_REQUIRE(((uintptr_t)d_probs & 3) == 0 && ((uintptr_t)d_keys & 3) == 0, "%s: probabilities and keys must be 4-byte aligned", what);
        if (work_bytes < dgrp_prob_hist_strata_workspace_bytes(nrec)) {
            dgrp_set_error("%s: workspace too small", what);
            return DGRP_ENOMEM;
        }
    }
    DGRP_HIP(hipMemsetAsync(d_hist, 0, sizeof(int64_t) * C * S * bins, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
    if (tiles == 0) return DGRP_OK;
    const int cells = C * S;
    const int room = SH_LDS / 4 / bins;                               // cells of one workgroup (>= 40)
    const int G = cells < room ? cells : room;
    const size_t lds = (size_t)G * bins * 4;
    static std::once_flag configured;        // the attribute is per function, not per launch (records run on a pool of host threads)
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] { cfg_err = hipFuncSetAttribute((const void *)strata_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SH_LDS); });
    DGRP_HIP(cfg_err);
    DGRP_HIP(hipMemcpyAsync(d_work, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    const int groups = (cells + G - 1) / G;
    const int64_t resident = lds <= SH_LDS / 2 ? 2048 : 1024;         // workgroups of 256 lanes: what the counters leave room for
    int64_t gx = tiles < resident ? tiles : resident;
    const int64_t least = (tiles + SH_MAX_TILES - 1) / SH_MAX_TILES;  // no 32-bit counter can wrap
    if (gx < least) gx = least;
    DGRP_REQUIRE(gx < (1ll << 31), "%s: too long", what);
    sh_args a;
    a.probs = d_probs;
    a.keys = d_keys;
    a.tcum = (const int64_t *)d_work;
    a.row0 = a.tcum + nrec + 1;
    a.len = a.row0 + nrec;
    a.off = a.len + nrec;
    a.nrec = nrec;
    a.C = C;
    a.S = S;
    a.bins = bins;
    a.G = G;
    a.cells = cells;
    a.fbins = (float)bins;
    a.hist = reinterpret_cast<unsigned long long *>(d_hist);
    a.bad = d_bad;
    hipLaunchKernelGGL(strata_hist_kernel, dim3((unsigned)gx, (unsigned)groups), dim3(SH_THREADS), lds, stream, a);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
