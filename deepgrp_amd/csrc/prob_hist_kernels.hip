// evaluate --curves: per class c, the histogram of the merged probability P[b, c] over the evaluated bases, split by whether the
// base's truth is c (include/deepgrp_hip.h states it).  Every threshold curve is an exact function of these integers on the host.
//
// One pass over the flat float32 array, 4 C + 1 bytes per base.  A workgroup of 512 lanes takes tiles of PH_ROWS rows of one
// record: it stages the tile's truth bytes in LDS, then reads the tile's R * C floats as 16-byte vectors, lane after lane, and
// derives (base, class) of every element from its index (one multiply-high per vector, a step per element).
//
// Counters, all 32-bit words of one LDS array:
//   * body [Cg][2][bins]: one ds_add per element that falls in bins 1 .. bins-2;
//   * ends [Cg][2][2][REP]: bins 0 and bins-1 -- where a trained model puts almost every element -- REP copies of each cell, a
//     lane adds to copy (lane mod REP).  At REP = 256 the 64 lanes of a wave-instruction touch 64 different banks whatever the
//     data: a hot cell costs what a cold one does (one shared word would serialise the 64 lanes of every instruction).
// Cg, the classes of one workgroup, is C when [C][2][bins] and 32 copies of the ends fit 160 KiB beside the truth tile; else the
// classes are cut into groups of Cg along grid.y and every group reads the array (bins <= 4096: one class always fits).
// A workgroup counts fewer than 2^32 elements (the grid is sized for it), so no counter wraps; at the end the copies are folded
// into the body and every non-zero word goes to d_hist with one 64-bit atomic add: integer sums, the same bytes on every run.
#include "dgrp_common.h"
#include <mutex>
#include <vector>

namespace {

#define PH_THREADS 512
#define PH_ROWS 4096                  // rows of a tile (its truth bytes in LDS)
#define PH_LDS (160 * 1024)
#define PH_MAX_TILES 16384            // tiles per workgroup: 16384 * PH_ROWS * DGRP_MAXC = 2^32 elements

struct ph_args {
    const float *probs;
    const int8_t *truth;
    const int64_t *tcum, *row0, *len, *off;   // workspace tables: tiles before record r [nrec + 1], then the caller's three
    int64_t nrec;
    int C, bins, Cg, rep;
    unsigned magic;                   // floor(2^32 / C) + 1 (C > 1): e / C == umulhi(e, magic) for e < 2^18
    float fbins;
    unsigned long long *hist;
    int *bad;
};

struct ph_ctx {
    unsigned *cnt;                    // body, then ends
    const int8_t *tr;                 // the tile's truth
    int C, bins, c0, Cg, rep, slot, ends0;
    float fbins;
    int *bad;
};

__device__ __forceinline__ void ph_count(const ph_ctx &x, float p, int b, int c)
{
    const int cg = c - x.c0;
    if ((unsigned)cg >= (unsigned)x.Cg) return;
    const int t = x.tr[b];
    if (!(p >= 0.0f && p <= 1.0f) || (unsigned)t >= (unsigned)x.C) {
        *x.bad = 1;
        return;
    }
    int k = (int)(p * x.fbins);
    k = k < x.bins - 1 ? k : x.bins - 1;
    const int cell = cg * 2 + (t == c ? 1 : 0);
    int w = cell * x.bins + k;
    if (k == 0) w = x.ends0 + (cell * 2) * x.rep + x.slot;
    else if (k == x.bins - 1) w = x.ends0 + (cell * 2 + 1) * x.rep + x.slot;
    atomicAdd(&x.cnt[w], 1u);
}

__global__ void __launch_bounds__(PH_THREADS) prob_hist_kernel(ph_args a)
{
    extern __shared__ __align__(16) unsigned char ph_lds[];
    int8_t *tr = reinterpret_cast<int8_t *>(ph_lds);
    unsigned *cnt = reinterpret_cast<unsigned *>(ph_lds + PH_ROWS);
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * a.Cg, Cg = a.C - c0 < a.Cg ? a.C - c0 : a.Cg;
    const int body = Cg * 2 * a.bins, words = body + Cg * 4 * a.rep;
    for (int i = tid; i < words; i += PH_THREADS) cnt[i] = 0u;
    ph_ctx x = { cnt, tr, a.C, a.bins, c0, Cg, a.rep, tid & (a.rep - 1), body, a.fbins, a.bad };
    // the array from a 16-byte boundary: element s of `al` is element s - A of probs
    const int A = (int)((reinterpret_cast<uintptr_t>(a.probs) >> 2) & 3);
    const float *al = a.probs - A;
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
        const int64_t lt = (t - a.tcum[r]) * PH_ROWS, left = a.len[r] - lt;
        const int nr = (int)(left < PH_ROWS ? left : PH_ROWS);
        __syncthreads();                                              // the zeroing; the last tile's readers of tr
        {
            const int8_t *src = a.truth + a.off[r] + lt;
            for (int j = tid; j < nr; j += PH_THREADS) tr[j] = src[j];
        }
        __syncthreads();
        const int64_t S0 = (a.row0[r] + lt) * a.C + A, S1 = S0 + (int64_t)nr * a.C;
        const int64_t v0 = (S0 + 3) >> 2, v1 = S1 >> 2;               // whole vectors [v0, v1) when v1 > v0
        const int64_t head1 = v0 * 4 < S1 ? v0 * 4 : S1, tail0 = v1 > v0 ? v1 * 4 : head1;
        if (tid < 3) {                                                // at most 3 elements in front of the first vector boundary
            const int64_t s = S0 + tid;
            if (s < head1) {
                const int e = tid, b = a.C > 1 ? (int)__umulhi((unsigned)e, a.magic) : e;
                ph_count(x, al[s], b, e - b * a.C);
            }
        } else if (tid < 6) {                                         // and at most 3 behind the last
            const int64_t s = tail0 + (tid - 3);
            if (s < S1) {
                const int e = (int)(s - S0), b = a.C > 1 ? (int)__umulhi((unsigned)e, a.magic) : e;
                ph_count(x, al[s], b, e - b * a.C);
            }
        }
        const int nv = v1 > v0 ? (int)(v1 - v0) : 0;
        const float4 *vec = reinterpret_cast<const float4 *>(al) + v0;
        const int e00 = (int)(v0 * 4 - S0);                           // tile-local element of vector 0
        for (int i0 = 0; i0 < nv; i0 += 4 * PH_THREADS) {
            float4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * PH_THREADS + tid;
                if (i < nv) q[u] = vec[i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * PH_THREADS + tid;
                if (i < nv) {
                    const int e = e00 + 4 * i;
                    int b = a.C > 1 ? (int)__umulhi((unsigned)e, a.magic) : e;
                    int c = e - b * a.C;
                    const float pv[4] = { q[u].x, q[u].y, q[u].z, q[u].w };
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ph_count(x, pv[j], b, c);
                        if (++c == a.C) { c = 0; ++b; }
                    }
                }
            }
        }
    }
    __syncthreads();
    // fold the copies of the end cells into the body: a wave per cell, a shuffle tree over its lanes
    const int wave = tid >> 6, lane = tid & 63;
    for (int cell = wave; cell < Cg * 4; cell += PH_THREADS / 64) {
        unsigned s = 0;
        for (int i = lane; i < a.rep; i += 64) s += cnt[body + cell * a.rep + i];
        for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
        if (lane == 0 && s) cnt[(cell >> 1) * a.bins + ((cell & 1) ? a.bins - 1 : 0)] += s;
    }
    __syncthreads();
    unsigned long long *out = a.hist + (int64_t)c0 * 2 * a.bins;
    for (int i = tid; i < body; i += PH_THREADS) {
        const unsigned v = cnt[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
}

// the classes of one workgroup and the copies of its end cells: the largest group that fits with 32 copies, then the most copies
static void ph_layout(int C, int bins, int &Cg, int &rep)
{
    const int64_t room = PH_LDS - PH_ROWS;
    Cg = C;
    while (Cg > 1 && (int64_t)Cg * (8 * bins + 16 * 32) > room) --Cg;
    rep = 256;
    while (rep > 32 && (int64_t)Cg * (8 * bins + 16 * rep) > room) rep >>= 1;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_prob_hist_workspace_bytes(int64_t nrec, int C, int bins)
{
    if (nrec < 0 || nrec >= (1ll << 40) || C < 1 || C > DGRP_MAXC || bins < 2 || bins > 4096) return 0;
    return dgrp_align_up((4 * nrec + 1) * 8, 256) + 256;
}

DGRP_EXPORT int dgrp_prob_hist_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                     const int8_t *d_truth, const int64_t *h_off, int bins, int64_t *d_hist, int *d_bad, void *d_work,
                                     int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "dgrp_prob_hist_batch: 1 <= classes <= 64");
    DGRP_REQUIRE(bins >= 2 && bins <= 4096, "dgrp_prob_hist_batch: 2 <= bins <= 4096");
    DGRP_REQUIRE(nrec >= 0 && d_hist && d_bad && (nrec == 0 || (h_row0 && h_n && h_off)), "dgrp_prob_hist_batch: bad arguments");
    DGRP_REQUIRE(((uintptr_t)d_hist & 7) == 0, "dgrp_prob_hist_batch: the histogram must be 8-byte aligned");
    DGRP_REQUIRE(nrec < (1ll << 28), "dgrp_prob_hist_batch: too many records");
    std::vector<int64_t> tab((size_t)(4 * nrec + 1), 0);
    int64_t *tcum = tab.data(), *row0 = tcum + nrec + 1, *len = row0 + nrec, *off = len + nrec;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_row0[r] >= 0 && h_n[r] >= 0 && h_off[r] >= 0, "dgrp_prob_hist_batch: negative offset, length or origin (record %lld)",
                     (long long)r);
        DGRP_REQUIRE(h_row0[r] < (1ll << 40) && h_n[r] < (1ll << 40) && h_off[r] < (1ll << 40), "dgrp_prob_hist_batch: too long (record %lld)",
                     (long long)r);
        tcum[r + 1] = tcum[r] + (h_n[r] + PH_ROWS - 1) / PH_ROWS;
        row0[r] = h_row0[r];
        len[r] = h_n[r];
        off[r] = h_off[r];
    }
    const int64_t tiles = tcum[nrec];
    if (tiles) {
        DGRP_REQUIRE(d_probs && d_truth && d_work, "dgrp_prob_hist_batch: NULL pointer");
        DGRP_REQUIRE(((uintptr_t)d_probs & 3) == 0, "dgrp_prob_hist_batch: the probabilities must be 4-byte aligned");
        DGRP_REQUIRE(work_bytes >= dgrp_prob_hist_workspace_bytes(nrec, C, bins), "dgrp_prob_hist_batch: workspace too small");
    }
    DGRP_HIP(hipMemsetAsync(d_hist, 0, sizeof(int64_t) * C * 2 * bins, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
    if (tiles == 0) return DGRP_OK;
    int Cg, rep;
    ph_layout(C, bins, Cg, rep);
    const size_t lds = (size_t)PH_ROWS + (size_t)Cg * (8 * bins + 16 * rep);
    static std::once_flag configured;        // the attribute is per function, not per launch (records run on a pool of host threads)
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] { cfg_err = hipFuncSetAttribute((const void *)prob_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PH_LDS); });
    DGRP_HIP(cfg_err);
    DGRP_HIP(hipMemcpyAsync(d_work, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    const int groups = (C + Cg - 1) / Cg;
    const int64_t resident = lds <= PH_LDS / 2 ? 1024 : 512;          // two workgroups per CU where the counters leave room
    int64_t gx = tiles < resident ? tiles : resident;
    const int64_t least = (tiles + PH_MAX_TILES - 1) / PH_MAX_TILES;  // no 32-bit counter can wrap
    if (gx < least) gx = least;
    DGRP_REQUIRE(gx < (1ll << 31), "dgrp_prob_hist_batch: too long");
    ph_args a;
    a.probs = d_probs;
    a.truth = d_truth;
    a.tcum = (const int64_t *)d_work;
    a.row0 = a.tcum + nrec + 1;
    a.len = a.row0 + nrec;
    a.off = a.len + nrec;
    a.nrec = nrec;
    a.C = C;
    a.bins = bins;
    a.Cg = Cg;
    a.rep = rep;
    a.magic = C > 1 ? (unsigned)((1ull << 32) / (unsigned)C + 1) : 0u;
    a.fbins = (float)bins;
    a.hist = reinterpret_cast<unsigned long long *>(d_hist);
    a.bad = d_bad;
    hipLaunchKernelGGL(prob_hist_kernel, dim3((unsigned)gx, (unsigned)groups), dim3(PH_THREADS), lds, stream, a);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
