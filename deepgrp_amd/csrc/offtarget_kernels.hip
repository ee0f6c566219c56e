// evaluate --offtarget: what the predicted repeats lie on (include/deepgrp_hip.h states the three entries).
//
// dgrp_token_ids.  Tokens are spans of the listing's text in HBM, `a` or the logical string `a/b` of two spans, never joined in memory.
// An open-addressing table of DGRP_TOKEN_SLOTS 64-bit words, EMPTY or the row that claimed the slot with one atomicCAS.  A row that
// finds a slot taken compares ITS bytes with the claimant's bytes: equal -> that is its slot, unequal -> the next slot.  The hash only
// says where to start looking; nothing is decided by it.  A slot never changes hands, so two rows of one token always meet in one
// slot whichever of them came first.  The occupied slots are compacted (scan.h), their spans go to the host, the host reads the
// strings, sorts them and sends back the rank of every compacted slot; the last kernel writes the rank of every row's slot.
//
// dgrp_key_crosstab_batch.  A cell is (predicted label, key column), one 32-bit counter in LDS; where C * K cells do not fit the
// 160 KiB strata_kernels.hip uses, they are cut into groups along grid.y and every group reads every base (5 bytes).  Neighbours share
// their cell, so a wave peels the counter of its first pending lane with a ballot, twice, before the lanes left add by themselves.
//
// dgrp_row_key_classes_batch.  The line of positions of dgrp_row_hits_batch, four counters per row instead of one.
#include "eval_rows.h"
#include <algorithm>
#include <mutex>
#include <string.h>

namespace {

#define TOK_SLOTS DGRP_TOKEN_SLOTS
#define TOK_MAX DGRP_TOKEN_MAX
#define TOK_HEAD 256                     // workspace head: [0] flags: 1 a span leaves the text, 2 the table is full
#define TOK_EMPTY 0xFFFFFFFFFFFFFFFFull

static_assert((TOK_SLOTS & (TOK_SLOTS - 1)) == 0 && TOK_MAX * 4 == TOK_SLOTS, "a power of two, a quarter full at the most");

struct tok_spans {
    const int64_t *pos;
    const int32_t *len;
    const int64_t *pos2;
    const int32_t *len2;
};

struct tok_str {
    int64_t a, b;
    int32_t la, lb;                      // lb = 0: the first span alone
    __device__ __forceinline__ int64_t len() const { return (int64_t)la + (lb > 0 ? 1 + (int64_t)lb : 0); }
    __device__ __forceinline__ uint8_t at(const uint8_t *__restrict__ t, int64_t j) const
    {
        return j < la ? t[a + j] : (j == la ? (uint8_t)'/' : t[b + (j - la - 1)]);
    }
};

__device__ __forceinline__ tok_str tok_of(const tok_spans &S, int64_t i)
{
    tok_str s;
    s.a = S.pos[i];
    s.la = S.len[i];
    s.lb = S.len2[i];
    s.b = s.lb > 0 ? S.pos2[i] : 0;
    return s;
}

__device__ __forceinline__ bool tok_inside(const tok_str &s, int64_t n)
{
    if (s.la < 0 || s.lb < 0 || s.a < 0 || s.a > n - s.la) return false;
    return s.lb == 0 || (s.b >= 0 && s.b <= n - s.lb);
}

// one lane per row: slot_of[i] = the slot of its token, claimed here when it is the first
__global__ void __launch_bounds__(256) tok_insert_kernel(const uint8_t *__restrict__ t, int64_t n, tok_spans S, int64_t rows,
                                                         unsigned long long *__restrict__ table, int32_t *__restrict__ slot_of,
                                                         unsigned long long *__restrict__ g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    slot_of[i] = -1;
    const tok_str s = tok_of(S, i);
    if (!tok_inside(s, n)) {
        atomicOr(&g[0], 1ull);
        return;
    }
    const int64_t L = s.len();
    uint64_t h = 0xcbf29ce484222325ull;                                       // FNV-1a: only where the search starts
    for (int64_t j = 0; j < L; ++j) h = (h ^ s.at(t, j)) * 0x100000001b3ull;
    uint32_t slot = (uint32_t)(h ^ (h >> 32)) & (TOK_SLOTS - 1);
    for (int probe = 0; probe < TOK_SLOTS; ++probe, slot = (slot + 1) & (TOK_SLOTS - 1)) {
        unsigned long long owner = table[slot];
        if (owner == TOK_EMPTY) owner = atomicCAS(&table[slot], TOK_EMPTY, (unsigned long long)i);
        if (owner == TOK_EMPTY) {                                             // claimed
            slot_of[i] = (int32_t)slot;
            return;
        }
        const tok_str o = tok_of(S, (int64_t)owner);
        bool same = tok_inside(o, n) && o.len() == L;
        for (int64_t j = 0; same && j < L; ++j) same = o.at(t, j) == s.at(t, j);
        if (same) {
            slot_of[i] = (int32_t)slot;
            return;
        }
    }
    atomicOr(&g[0], 2ull);
}

__global__ void __launch_bounds__(256) tok_flag_kernel(const unsigned long long *__restrict__ table, uint64_t *__restrict__ flag)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    flag[s] = table[s] != TOK_EMPTY ? 1ull : 0ull;
}

// ex = the exclusive scan of the flags: compacted slot ex[s] is represented by the row that claimed slot s
__global__ void __launch_bounds__(256) tok_spans_kernel(const unsigned long long *__restrict__ table, const uint64_t *__restrict__ ex,
                                                        tok_spans S, int64_t *__restrict__ spans)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long owner = table[s];
    if (owner == TOK_EMPTY || ex[s] >= TOK_MAX) return;
    int64_t *o = spans + 4 * (int64_t)ex[s];
    const int32_t lb = S.len2[owner];
    o[0] = S.pos[owner];
    o[1] = S.len[owner];
    o[2] = lb > 0 ? S.pos2[owner] : 0;
    o[3] = lb;
}

// one lane per compacted slot: its logical string to blob[off[c] .. off[c + 1])
__global__ void __launch_bounds__(256) tok_gather_kernel(const uint8_t *__restrict__ t, const int64_t *__restrict__ spans,
                                                         const int64_t *__restrict__ off, int F, uint8_t *__restrict__ blob)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= F) return;
    tok_str s;
    s.a = spans[4 * c];
    s.la = (int32_t)spans[4 * c + 1];
    s.b = spans[4 * c + 2];
    s.lb = (int32_t)spans[4 * c + 3];
    const int64_t L = off[c + 1] - off[c];
    for (int64_t j = 0; j < L; ++j) blob[off[c] + j] = s.at(t, j);
}

__global__ void __launch_bounds__(256) tok_fid_kernel(const int32_t *__restrict__ slot_of, const uint64_t *__restrict__ ex,
                                                      const int32_t *__restrict__ rank, int64_t rows, int32_t *__restrict__ fid)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) fid[i] = rank[ex[slot_of[i]]];
}

struct tok_layout {
    unsigned long long *g, *table;
    uint64_t *ex, *tiles;
    int64_t *spans, *blob_off;
    int32_t *slot_of, *rank;
    uint8_t *blob;
    int64_t bytes;
};

// the scan's total, ex[TOK_SLOTS], lies directly in front of the spans: both reach the host in one copy
tok_layout tok_layout_of(void *d_work, int64_t rows, int64_t names_cap)
{
    tok_layout l;
    char *p = (char *)d_work;
    l.g = (unsigned long long *)p;
    p += TOK_HEAD;
    l.table = (unsigned long long *)p;
    p += (int64_t)TOK_SLOTS * 8;
    l.ex = (uint64_t *)p;
    l.spans = (int64_t *)(l.ex + TOK_SLOTS + 1);
    p += dgrp_align_up(((int64_t)TOK_SLOTS + 1) * 8 + (int64_t)TOK_MAX * 32, 256);
    l.tiles = (uint64_t *)p;
    p += dgrp_align_up((TOK_SLOTS / SCAN_TILE + 1) * 8, 256);
    l.blob_off = (int64_t *)p;
    p += dgrp_align_up(((int64_t)TOK_MAX + 1) * 8, 256);
    l.rank = (int32_t *)p;
    p += dgrp_align_up((int64_t)TOK_MAX * 4, 256);
    l.slot_of = (int32_t *)p;
    p += dgrp_align_up(rows * 4, 256);
    l.blob = (uint8_t *)p;
    p += dgrp_align_up(names_cap, 256);
    l.bytes = p - (char *)d_work;
    return l;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_token_ids_workspace_bytes(int64_t rows, int64_t names_cap)
{
    if (rows < 0 || names_cap < 0 || rows >= (1ll << 40) || names_cap >= (1ll << 40)) return 0;
    return tok_layout_of(nullptr, rows, names_cap).bytes;
}

DGRP_EXPORT int dgrp_token_ids(const uint8_t *d_text, int64_t n, int64_t rows, const int64_t *d_pos, const int32_t *d_len,
                               const int64_t *d_pos2, const int32_t *d_len2, int32_t *d_fid, uint8_t *h_names, int64_t names_cap,
                               int64_t *h_name_off, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_token_ids";
    DGRP_REQUIRE(h_counts && h_name_off, "%s: NULL counts", what);
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    h_name_off[0] = 0;
    DGRP_REQUIRE(n >= 0 && rows >= 0 && rows < (1ll << 40) && names_cap >= 0 && names_cap < (1ll << 40), "%s: bad sizes", what);
    DGRP_REQUIRE(h_names || names_cap == 0, "%s: NULL names", what);
    if (rows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_text && d_pos && d_len && d_pos2 && d_len2 && d_fid, "%s: NULL pointer", what);
    DGRP_REQUIRE(d_work && ((uintptr_t)d_work & 255) == 0, "%s: workspace NULL or not 256-byte aligned", what);
    if (work_bytes < dgrp_token_ids_workspace_bytes(rows, names_cap)) {
        dgrp_set_error("%s: workspace too small", what);
        return DGRP_ENOMEM;
    }
    const tok_layout l = tok_layout_of(d_work, rows, names_cap);
    const tok_spans S = { d_pos, d_len, d_pos2, d_len2 };
    DGRP_HIP(hipMemsetAsync(l.g, 0, TOK_HEAD, stream));
    DGRP_HIP(hipMemsetAsync(l.table, 0xFF, (size_t)TOK_SLOTS * 8, stream));
    hipLaunchKernelGGL(tok_insert_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, d_text, n, S, rows, l.table, l.slot_of,
                       l.g);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(tok_flag_kernel, dim3(TOK_SLOTS / 256), dim3(256), 0, stream, l.table, l.ex);
    DGRP_LAUNCH_CHECK();
    int rc = device_exclusive_scan(l.ex, l.ex, TOK_SLOTS, l.tiles, l.ex + TOK_SLOTS, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(tok_spans_kernel, dim3(TOK_SLOTS / 256), dim3(256), 0, stream, l.table, l.ex, S, l.spans);
    DGRP_LAUNCH_CHECK();
    // the flags, then the count and the spans in one copy: the first synchronisation
    std::vector<int64_t> got((size_t)1 + 4 * TOK_MAX);
    unsigned long long flags = 0;
    hipError_t e = hipMemcpyAsync(&flags, l.g, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(got.data(), l.ex + TOK_SLOTS, got.size() * 8, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);
    DGRP_HIP(e);
    DGRP_HIP(e2);
    DGRP_REQUIRE(!(flags & 1), "%s: a token span leaves the text of %lld bytes", what, (long long)n);
    const int64_t F = got[0];
    h_counts[0] = F;
    if ((flags & 2) || F > TOK_MAX) {                                         // too many distinct tokens: the caller's host path
        h_counts[1] = 1;
        return DGRP_OK;
    }
    const int64_t *spans = got.data() + 1;
    std::vector<int64_t> off((size_t)F + 1, 0);
    for (int64_t c = 0; c < F; ++c) off[c + 1] = off[c] + spans[4 * c + 1] + (spans[4 * c + 3] > 0 ? 1 + spans[4 * c + 3] : 0);
    const int64_t total = off[F];
    h_counts[2] = total;
    if (total > names_cap) {
        dgrp_set_error("%s: %lld bytes of names for a capacity of %lld", what, (long long)total, (long long)names_cap);
        return DGRP_ENOMEM;
    }
    // the strings: gathered on the device, one copy back: the second synchronisation
    std::vector<uint8_t> blob((size_t)total + 1);
    DGRP_HIP(hipMemcpyAsync(l.blob_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(tok_gather_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, stream, d_text, l.spans, l.blob_off, (int)F, l.blob);
    DGRP_LAUNCH_CHECK();
    e = total ? hipMemcpyAsync(blob.data(), l.blob, (size_t)total, hipMemcpyDeviceToHost, stream) : hipSuccess;
    const hipError_t e3 = hipStreamSynchronize(stream);
    DGRP_HIP(e);
    DGRP_HIP(e3);
    // ascending byte order, a proper prefix first
    std::vector<int32_t> order((size_t)F), rank((size_t)F);
    for (int64_t c = 0; c < F; ++c) order[c] = (int32_t)c;
    const uint8_t *b = blob.data();
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int64_t lx = off[x + 1] - off[x], ly = off[y + 1] - off[y];
        const int c = memcmp(b + off[x], b + off[y], (size_t)(lx < ly ? lx : ly));
        return c != 0 ? c < 0 : lx < ly;
    });
    int64_t at = 0;
    for (int64_t k = 0; k < F; ++k) {
        const int32_t c = order[k];
        rank[c] = (int32_t)k;
        const int64_t len = off[c + 1] - off[c];
        if (len) memcpy(h_names + at, b + off[c], (size_t)len);
        at += len;
        h_name_off[k + 1] = at;
    }
    // the ranks go up, every row takes the rank of its slot: the third synchronisation (the host table dies on return)
    DGRP_HIP(hipMemcpyAsync(l.rank, rank.data(), (size_t)F * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(tok_fid_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, l.slot_of, l.ex, l.rank, rows, d_fid);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
namespace {

#define XT_THREADS 256
#define XT_ROWS 4096                  // bases of a tile
#define XT_LDS (160 * 1024)           // the budget of strata_kernels.hip
#define XT_MAX_TILES (1 << 19)        // tiles per workgroup: 2^19 * XT_ROWS = 2^31 bases, no 32-bit counter can wrap
#define XT_NONE 0xFFFFFFFFu

__global__ void __launch_bounds__(XT_THREADS) key_crosstab_kernel(const int8_t *__restrict__ pred, const unsigned *__restrict__ keys,
                                                                 int64_t n, int C, int K, int G, int cells,
                                                                 unsigned long long *__restrict__ hist, int *__restrict__ bad)
{
    extern __shared__ __align__(16) unsigned xt_cnt[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.y * G, own = cells - c0 < G ? cells - c0 : G;
    for (int i = tid; i < own; i += XT_THREADS) xt_cnt[i] = 0u;
    __syncthreads();
    const int64_t tiles = (n + XT_ROWS - 1) / XT_ROWS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t b0 = t * XT_ROWS, left = n - b0;
        const int nr = (int)(left < XT_ROWS ? left : XT_ROWS);
        for (int j0 = 0; j0 < nr; j0 += XT_THREADS) {                 // (uniform bounds: whole waves reach the ballots)
            const int j = j0 + tid;
            int w = -1;
            if (j < nr) {
                const unsigned key = keys[b0 + j];
                const int p = pred[b0 + j];
                const unsigned col = key == XT_NONE ? (unsigned)(K - 1) : key;
                if ((unsigned)p >= (unsigned)C || (key != XT_NONE && key >= (unsigned)(K - 1))) {
                    *bad = 1;
                } else {
                    const int cell = p * K + (int)col - c0;
                    if ((unsigned)cell < (unsigned)own) w = cell;
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
                if (lane == leader) atomicAdd(&xt_cnt[wl], (unsigned)__popcll(same));
                if (mine) todo = false;
            }
            if (todo) atomicAdd(&xt_cnt[w], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < own; i += XT_THREADS) {
        const unsigned v = xt_cnt[i];
        if (v) atomicAdd(&hist[(int64_t)c0 + i], (unsigned long long)v);
    }
}

#define RK_LDS_ROWS 1024              // the slice's rows with their four counters in LDS; a slice crossing more adds to d_cls directly

// cls[j][k] += bases of row j's clipped span whose key is of kind k: 0 the row's label, 1 another label, 2 a family, 3 none
__global__ void __launch_bounds__(256) row_key_classes_kernel(const unsigned *__restrict__ keys, const uint64_t *__restrict__ ex,
                                                              const int64_t *__restrict__ dst, const dgrp_segment *__restrict__ rows,
                                                              int64_t n, unsigned long long *__restrict__ cls)
{
    __shared__ unsigned cnt[RK_LDS_ROWS * 4];
    __shared__ int64_t s_r0, s_r1;
    const uint64_t total = ex[n], s0 = (uint64_t)blockIdx.x * EVAL_SLICE;
    const uint64_t s1 = s0 + EVAL_SLICE < total ? s0 + EVAL_SLICE : total;    // (s0 < total: the grid covers the line exactly)
    if (threadIdx.x == 0) {
        s_r0 = eval_row_of(ex, 0, n, s0);
        s_r1 = eval_row_of(ex, s_r0, n, s1 - 1);
    }
    for (int k = threadIdx.x; k < RK_LDS_ROWS * 4; k += 256) cnt[k] = 0u;
    __syncthreads();
    const int64_t r0 = s_r0, r1 = s_r1;
    const bool staged = r1 - r0 < RK_LDS_ROWS;
    const uint64_t p0 = s0 + threadIdx.x;
    if (p0 < s1) {
        int64_t j = eval_row_of(ex, r0, r1 + 1, p0);
        uint64_t jst = ex[j], jend = ex[j + 1];
        unsigned lab = (unsigned)rows[j].label;
        unsigned c[4] = { 0u, 0u, 0u, 0u };
        auto flush = [&]() {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c[k]) {
                    if (staged) atomicAdd(&cnt[(j - r0) * 4 + k], c[k]);
                    else atomicAdd(&cls[j * 4 + k], (unsigned long long)c[k]);
                }
                c[k] = 0u;
            }
        };
        for (uint64_t p = p0; p < s1; p += 256) {
            if (jend <= p) {
                flush();
                while (jend <= p) { ++j; jst = jend; jend = ex[j + 1]; }
                lab = (unsigned)rows[j].label;
            }
            const unsigned key = keys[dst[j] + (int64_t)(p - jst)];
            c[0] += key == lab ? 1u : 0u;
            c[1] += key < 64u && key != lab ? 1u : 0u;
            c[2] += key >= 64u && key != XT_NONE ? 1u : 0u;
            c[3] += key == XT_NONE ? 1u : 0u;
        }
        flush();
    }
    __syncthreads();
    if (staged) {
        for (int64_t k = threadIdx.x; k < (r1 - r0 + 1) * 4; k += 256) {
            const unsigned v = cnt[k];
            if (v) atomicAdd(&cls[r0 * 4 + k], (unsigned long long)v);
        }
    }
}

}   // namespace

DGRP_EXPORT int dgrp_key_crosstab_batch(const int8_t *d_pred, const uint32_t *d_keys, int64_t n, int C, int64_t K, int64_t *d_hist,
                                        int *d_bad, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_key_crosstab_batch";
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "%s: 1 <= classes <= 64", what);
    DGRP_REQUIRE(K >= 65 && K <= 64 + (int64_t)DGRP_TOKEN_MAX + 1, "%s: 65 <= key columns <= %d", what, 64 + DGRP_TOKEN_MAX + 1);
    DGRP_REQUIRE(n >= 0 && n < (1ll << 40) && d_hist && d_bad, "%s: bad arguments", what);
    DGRP_REQUIRE(((uintptr_t)d_hist & 7) == 0, "%s: the counts must be 8-byte aligned", what);
    DGRP_HIP(hipMemsetAsync(d_hist, 0, sizeof(int64_t) * (size_t)C * (size_t)K, stream));
    DGRP_HIP(hipMemsetAsync(d_bad, 0, sizeof(int), stream));
    if (n == 0) return DGRP_OK;
    DGRP_REQUIRE(d_pred && d_keys && ((uintptr_t)d_keys & 3) == 0, "%s: NULL labels, or keys NULL or not 4-byte aligned", what);
    const int64_t cells = (int64_t)C * K;                              // (< 2^21)
    const int room = XT_LDS / 4;
    const int G = (int)(cells < room ? cells : room);
    const size_t lds = (size_t)G * 4;
    static std::once_flag configured;        // the attribute is per function, not per launch (records run on a pool of host threads)
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] { cfg_err = hipFuncSetAttribute((const void *)key_crosstab_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, XT_LDS); });
    DGRP_HIP(cfg_err);
    const int groups = (int)((cells + G - 1) / G);
    const int64_t tiles = (n + XT_ROWS - 1) / XT_ROWS;
    const int64_t resident = lds <= XT_LDS / 2 ? 2048 : 1024;          // workgroups of 256 lanes: what the counters leave room for
    int64_t gx = tiles < resident ? tiles : resident;
    const int64_t least = (tiles + XT_MAX_TILES - 1) / XT_MAX_TILES;
    if (gx < least) gx = least;
    hipLaunchKernelGGL(key_crosstab_kernel, dim3((unsigned)gx, (unsigned)groups), dim3(XT_THREADS), lds, stream, d_pred, d_keys, n, C, (int)K,
                       G, (int)cells, reinterpret_cast<unsigned long long *>(d_hist), d_bad);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_row_key_classes_batch(const uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                           const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off, int64_t *d_cls,
                                           void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_row_key_classes_batch";
    eval_plan pl;
    const int rc = eval_prepare(what, nrec, h_off, h_len, h_origin, d_rows, h_row_off, d_work, work_bytes, stream, pl, 63);
    if (rc != DGRP_OK || pl.nrows == 0 || nrec == 0) return rc;
    DGRP_REQUIRE(d_cls && ((uintptr_t)d_cls & 7) == 0, "%s: the counts are NULL or not 8-byte aligned", what);
    const int64_t r0 = h_row_off[0];
    DGRP_HIP(hipMemsetAsync(d_cls + 4 * r0, 0, (size_t)pl.nrows * 32, stream));
    uint64_t total = 0;
    for (int k = 1; k < 128; ++k) total += pl.tot[k];
    if (total == 0) return DGRP_OK;
    DGRP_REQUIRE(d_keys && ((uintptr_t)d_keys & 3) == 0, "%s: keys NULL or not 4-byte aligned", what);
    const int e = eval_spans(pl, d_rows, nrec, 0, stream);
    if (e != DGRP_OK) return e;
    hipLaunchKernelGGL(row_key_classes_kernel, dim3((unsigned)((total + EVAL_SLICE - 1) / EVAL_SLICE)), dim3(256), 0, stream, d_keys, pl.d_cl,
                       pl.d_dst, d_rows + r0, pl.nrows, reinterpret_cast<unsigned long long *>(d_cls + 4 * r0));
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
