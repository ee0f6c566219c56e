// train from a sequence file: what `train` prepared on the host for a .npz input, built on the device for records that the FASTA /
// BGZF / 2bit ingest left in HBM -- the multi-hot truth of preprocess_y (deepgrp/preprocessing.py:9-48), the class index sets of
// _calc_indices (deepgrp/training.py:76-81) and the start positions of a batch drawn as (set, rank) pairs.  Byte kernels: the truth
// costs 2C - 1 bytes per base and one per painted position (C - 1 cleared, C - 1 read and one written for row 0), a class set
// 1 + T / 8192 bytes per base and pass and 8 per member.
#include "eval_paint.h"
#include "scan.h"
#include <vector>

namespace {

#define PREP_HEAD 256             // workspace head: [0] flag, [1] first bad row, [2] painted positions / members of the set
#define SET_BLOCK 8192            // window starts per workgroup: 256 lanes x 32 consecutive starts
#define SET_MAXT 4096             // longest window
#define SET_CHUNK ((SET_BLOCK + SET_MAXT) / 256)   // staged bytes per lane in the prefix pass (48: three 16-byte LDS reads)

// ------------------------------------------------------------------------------------------------------------------------- truth
// one lane per row: 0 <= start <= end and 1 <= label <= max_label, else g[0] |= 1 and g[1] = smallest bad row; g[2] += clipped length
__global__ void __launch_bounds__(256) truth_check_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                          int64_t nrec, const int64_t *__restrict__ len,
                                                          const int64_t *__restrict__ origin, int max_label,
                                                          unsigned long long *__restrict__ g)
{
    __shared__ unsigned long long s_tot;
    if (threadIdx.x == 0) s_tot = 0ull;
    __syncthreads();
    const int64_t i = row_off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < row_off[nrec]) {
        const dgrp_segment q = rows[i];
        if (q.start < 0 || q.end < q.start || q.label < 1 || q.label > max_label) {
            atomicOr(&g[0], 1ull);
            atomicMin(&g[1], (unsigned long long)i);
        } else {
            const int64_t r = dgrp_record_of(row_off, nrec, i);
            int64_t cs, cl;
            eval_clip(q, origin[r], len[r], cs, cl);
            if (cl) atomicAdd(&s_tot, (unsigned long long)cl);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_tot) atomicAdd(&g[2], s_tot);
}

// one lane per row j (= row row_off[0] + j): cl[j] = its clipped length, dst[j] = the position in d_truth of its first clipped base
// ON ITS LABEL'S ROW, so that one paint pass over all rows sets every class
__global__ void __launch_bounds__(256) truth_span_kernel(const dgrp_segment *__restrict__ rows, const int64_t *__restrict__ row_off,
                                                         int64_t nrec, const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                         const int64_t *__restrict__ origin, int64_t n_total, uint64_t *__restrict__ cl,
                                                         int64_t *__restrict__ dst)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = row_off[0] + j;
    if (i >= row_off[nrec]) return;
    const dgrp_segment q = rows[i];
    const int64_t r = dgrp_record_of(row_off, nrec, i);
    int64_t cs, n;
    eval_clip(q, origin[r], len[r], cs, n);
    cl[j] = (uint64_t)n;
    dst[j] = (int64_t)q.label * n_total + off[r] + cs;
}

// row 0 from the others: 1 where no class row holds a 1.  The class rows hold 0 or 1 only (cleared and painted above), so the
// bytes of four positions are tested in one word.  A class row starts at c * n, any alignment: its 16 bytes are read unaligned.
__global__ void __launch_bounds__(256) truth_row0_kernel(int8_t *__restrict__ truth, int64_t n, int C)
{
    for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16; i0 < n; i0 += (int64_t)gridDim.x * 4096) {
        if (i0 + 16 <= n) {
            uint4 acc = make_uint4(0u, 0u, 0u, 0u);
            for (int c = 1; c < C; ++c) {
                uint4 v;
                __builtin_memcpy(&v, truth + (int64_t)c * n + i0, 16);
                acc.x |= v.x; acc.y |= v.y; acc.z |= v.z; acc.w |= v.w;
            }
            const uint32_t one = 0x01010101u;
            *reinterpret_cast<uint4 *>(truth + i0) = make_uint4(~acc.x & one, ~acc.y & one, ~acc.z & one, ~acc.w & one);
        } else {
            for (int64_t i = i0; i < n; ++i) {
                int any = 0;
                for (int c = 1; c < C; ++c) any |= truth[(int64_t)c * n + i];
                truth[i] = any ? 0 : 1;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- class sets
// largest r < nrec with first[r] <= b
__device__ __forceinline__ int64_t set_record_of(const uint64_t *__restrict__ first, int64_t nrec, uint64_t b)
{
    int64_t lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// Workgroup b takes the starts s0 .. s1 (at most SET_BLOCK of 1 .. len - 1 - T) of its record: first[r] is the record's first
// workgroup.  The row's bytes s0 + 1 .. s1 + T -- all inside the record -- are staged in LDS and counted into a prefix P (P[i] = ones
// among the first i staged bytes), so that start s is a member when P[s - s0 + T] != P[s - s0]: a 1 in [s + 1, s + T].
// WRITE = false: count[b] = members of the workgroup.  WRITE = true: count[] holds the exclusive scan, the members go to out[] ascending
// as buffer positions off[r] + s.
template <bool WRITE>
__global__ void __launch_bounds__(256) class_starts_kernel(const int8_t *__restrict__ row, const uint64_t *__restrict__ first,
                                                           int64_t nrec, const int64_t *__restrict__ off,
                                                           const int64_t *__restrict__ len, int T, uint64_t *__restrict__ count,
                                                           int64_t *__restrict__ out)
{
    __shared__ __align__(16) uint8_t raw[SET_BLOCK + SET_MAXT];
    __shared__ __align__(4) uint16_t P[SET_BLOCK + SET_MAXT];
    __shared__ uint64_t lds[4];
    const int64_t r = set_record_of(first, nrec, blockIdx.x);
    const int64_t last = len[r] - 1 - T;                                       // the record's last start (>= 1: it has a workgroup)
    const int64_t s0 = 1 + (int64_t)(blockIdx.x - first[r]) * SET_BLOCK;
    const int64_t s1 = s0 + SET_BLOCK - 1 < last ? s0 + SET_BLOCK - 1 : last;
    const int starts = (int)(s1 - s0 + 1), staged = starts - 1 + T;            // staged <= SET_BLOCK + SET_MAXT - 1
    const int8_t *__restrict__ src = row + off[r] + s0 + 1;
    for (int i = threadIdx.x; i < SET_BLOCK + SET_MAXT; i += 256) raw[i] = i < staged ? (uint8_t)(src[i] != 0) : (uint8_t)0;
    __syncthreads();
    // the lane's SET_CHUNK staged bytes, their sum, the workgroup's scan of the sums, then the running count of every byte
    uint32_t w[SET_CHUNK / 4];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < SET_CHUNK / 16; ++k) {
        const uint4 v = *reinterpret_cast<const uint4 *>(raw + threadIdx.x * SET_CHUNK + 16 * k);
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < SET_CHUNK / 4; ++k) mine += __popc(w[k]);
    uint32_t run = (uint32_t)block_exclusive_scan((uint64_t)mine, nullptr, lds);
    uint32_t *__restrict__ P2 = reinterpret_cast<uint32_t *>(P) + threadIdx.x * (SET_CHUNK / 2);
#pragma unroll
    for (int k = 0; k < SET_CHUNK / 2; ++k) {
        const uint32_t a = (w[k >> 1] >> (16 * (k & 1))) & 1u, b = (w[k >> 1] >> (16 * (k & 1) + 8)) & 1u;
        P2[k] = run | ((run + a) << 16);
        run += a + b;
    }
    __syncthreads();
    // 32 consecutive starts per lane
    const int i0 = threadIdx.x * (SET_BLOCK / 256);
    uint32_t flags = 0;
#pragma unroll 8
    for (int k = 0; k < SET_BLOCK / 256; ++k) {
        const int i = i0 + k;
        if (i < starts && P[i + T] != P[i]) flags |= 1u << k;
    }
    uint64_t total;
    const uint64_t ex = block_exclusive_scan((uint64_t)__popc(flags), &total, lds);
    if (!WRITE) {
        if (threadIdx.x == 0) count[blockIdx.x] = total;
        return;
    }
    int64_t *__restrict__ dst = out + count[blockIdx.x] + ex;
    const int64_t pos0 = off[r] + s0 + i0;
    while (flags) {
        const int k = __ffs(flags) - 1;
        flags &= flags - 1;
        *dst++ = pos0 + k;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ resolve
// one lane per pick: (set, rank) -> start.  A set outside 0 .. nsets - 1, or an empty one, is the uniform part: rank k of [0, W) is
// start base[r] + k - wprefix[r] of the record r with wprefix[r] <= k < wprefix[r + 1].  Ranks are clamped into their range.
__global__ void __launch_bounds__(256) resolve_starts_kernel(const int64_t *__restrict__ picks, int64_t B,
                                                             const int64_t *const *__restrict__ set_ptr,
                                                             const int64_t *__restrict__ set_size, int nsets,
                                                             const int64_t *__restrict__ base, const int64_t *__restrict__ wprefix,
                                                             int64_t nrec, int64_t *__restrict__ starts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t set = picks[2 * i];
    int64_t k = picks[2 * i + 1];
    k = k < 0 ? 0 : k;
    if (set >= 0 && set < nsets) {
        const int64_t size = set_size[set];
        if (size > 0) {
            starts[i] = set_ptr[set][k < size ? k : size - 1];
            return;
        }
    }
    const int64_t W = wprefix[nrec];
    if (W <= 0) { starts[i] = 0; return; }
    k = k < W ? k : W - 1;
    int64_t lo = 0, hi = nrec;                                                 // largest r < nrec with wprefix[r] <= k
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (wprefix[mid] <= k) lo = mid; else hi = mid;
    }
    starts[i] = base[lo] + (k - wprefix[lo]);
}

// the records of an entry, checked: every one inside [0, n_total)
static int prep_records(const char *what, int64_t n_total, int64_t nrec, const int64_t *h_off, const int64_t *h_len)
{
    DGRP_REQUIRE(n_total >= 0 && nrec >= 0 && (nrec == 0 || (h_off && h_len)), "%s: bad arguments", what);
    for (int64_t r = 0; r < nrec; ++r)
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0 && h_off[r] <= n_total && h_len[r] <= n_total - h_off[r],
                     "%s: record %lld [%lld, +%lld) leaves the buffer of %lld bases", what, (long long)r, (long long)h_off[r],
                     (long long)h_len[r], (long long)n_total);
    return DGRP_OK;
}

static inline int64_t set_blocks_of(int64_t len, int T)
{
    const int64_t members = len - 1 - T;                                       // starts 1 .. len - 1 - T
    return members > 0 ? (members + SET_BLOCK - 1) / SET_BLOCK : 0;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_truth_workspace_bytes(int64_t nrec, int64_t nrows)
{
    if (nrec < 0 || nrows < 0) return 0;
    return PREP_HEAD + dgrp_align_up((4 * nrec + 1) * 8, 256) + dgrp_align_up((nrows + 1) * 8, 256) + dgrp_align_up(nrows * 8, 256) +
           dgrp_align_up(((nrows + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_truth_multihot_batch(int8_t *d_truth, int C, int64_t n_total, int64_t nrec, const int64_t *h_off,
                                          const int64_t *h_len, const int64_t *h_origin, const dgrp_segment *d_rows,
                                          const int64_t *h_row_off, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_truth_multihot_batch";
    DGRP_REQUIRE(C >= 2 && C <= DGRP_MAXC, "%s: %d classes outside 2..%d", what, C, DGRP_MAXC);
    int rc = prep_records(what, n_total, nrec, h_off, h_len);
    if (rc != DGRP_OK) return rc;
    DGRP_REQUIRE(nrec == 0 || (h_origin && h_row_off), "%s: bad arguments", what);
    DGRP_REQUIRE(nrec == 0 || h_row_off[0] >= 0, "%s: negative row offset", what);
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_origin[r] >= 0, "%s: negative origin (record %lld)", what, (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "%s: row offsets must ascend (record %lld)", what, (long long)r);
    }
    if (n_total == 0) return DGRP_OK;
    DGRP_REQUIRE(d_truth && ((uintptr_t)d_truth & 15) == 0, "%s: d_truth NULL or not 16-byte aligned", what);
    const int64_t nrows = nrec ? h_row_off[nrec] - h_row_off[0] : 0;
    uint64_t painted = 0;
    uint64_t *d_cl = nullptr, *d_tiles = nullptr;
    int64_t *d_tab = nullptr, *d_dst = nullptr;
    if (nrows > 0) {
        DGRP_REQUIRE(d_rows && d_work && ((uintptr_t)d_work & 255) == 0, "%s: rows or workspace NULL, or workspace not 256-byte aligned", what);
        if (work_bytes < dgrp_truth_workspace_bytes(nrec, nrows)) {
            dgrp_set_error("%s: workspace too small", what);
            return DGRP_ENOMEM;
        }
        std::vector<int64_t> tab((size_t)(4 * nrec + 1));
        for (int64_t r = 0; r < nrec; ++r) {
            tab[r] = h_off[r];
            tab[nrec + r] = h_len[r];
            tab[2 * nrec + r] = h_origin[r];
        }
        for (int64_t r = 0; r <= nrec; ++r) tab[3 * nrec + r] = h_row_off[r];
        unsigned long long *g = (unsigned long long *)d_work;
        char *p = (char *)d_work + PREP_HEAD;
        d_tab = (int64_t *)p;
        p += dgrp_align_up((4 * nrec + 1) * 8, 256);
        d_cl = (uint64_t *)p;
        p += dgrp_align_up((nrows + 1) * 8, 256);
        d_dst = (int64_t *)p;
        p += dgrp_align_up(nrows * 8, 256);
        d_tiles = (uint64_t *)p;
        const unsigned long long init[3] = { 0ull, ~0ull, 0ull };
        unsigned long long hg[3];
        dgrp_segment q;
        // the row check: one synchronisation, and nothing of d_truth is written before it has passed
        hipError_t e = hipMemcpyAsync(g, init, sizeof(init), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(truth_check_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, d_rows, d_tab + 3 * nrec,
                               nrec, d_tab + nrec, d_tab + 2 * nrec, C - 1, g);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(hg, g, sizeof(hg), hipMemcpyDeviceToHost, stream);
        const hipError_t e2 = hipStreamSynchronize(stream);                    // (also when a call above failed: `tab` dies on return)
        DGRP_HIP(e);
        DGRP_HIP(e2);
        if (hg[0]) {
            const int64_t i = (int64_t)hg[1];
            DGRP_HIP(hipMemcpyAsync(&q, d_rows + i, sizeof(q), hipMemcpyDeviceToHost, stream));
            DGRP_HIP(hipStreamSynchronize(stream));
            DGRP_REQUIRE(false, "%s: row %lld [%lld, %lld) label %d: rows need 0 <= start <= end and 1 <= label <= %d", what,
                         (long long)i, (long long)q.start, (long long)q.end, (int)q.label, C - 1);
        }
        painted = hg[2];
    }
    DGRP_HIP(hipMemsetAsync(d_truth + n_total, 0, (size_t)(C - 1) * (size_t)n_total, stream));
    if (painted == 0) {
        DGRP_HIP(hipMemsetAsync(d_truth, 1, (size_t)n_total, stream));
        return DGRP_OK;
    }
    hipLaunchKernelGGL(truth_span_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, d_rows, d_tab + 3 * nrec, nrec,
                       d_tab, d_tab + nrec, d_tab + 2 * nrec, n_total, d_cl, d_dst);
    DGRP_LAUNCH_CHECK();
    rc = device_exclusive_scan(d_cl, d_cl, nrows, d_tiles, d_cl + nrows, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(eval_paint_kernel, dim3((unsigned)((painted + EVAL_SLICE - 1) / EVAL_SLICE)), dim3(256), 0, stream, d_truth, d_cl,
                       d_dst, nrows, 1);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(truth_row0_kernel, dim3((unsigned)grid_for((n_total + 15) / 16, 256)), dim3(256), 0, stream, d_truth, n_total, C);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

static inline int64_t set_workspace_bytes(int64_t nrec, int64_t blocks)
{
    return PREP_HEAD + dgrp_align_up((3 * nrec + 1) * 8, 256) + dgrp_align_up((blocks + 1) * 8, 256) +
           dgrp_align_up(((blocks + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256);
}

DGRP_EXPORT int64_t dgrp_class_starts_workspace_bytes(int64_t nrec, int64_t n_total)
{
    if (nrec < 0 || n_total < 0) return 0;
    return set_workspace_bytes(nrec, n_total / SET_BLOCK + nrec);              // at least the workgroups of disjoint records, any T
}

DGRP_EXPORT int dgrp_class_window_starts(const int8_t *d_row, int64_t n_total, int64_t nrec, const int64_t *h_off,
                                         const int64_t *h_len, int T, int64_t *d_starts, int64_t cap, int64_t *h_count, void *d_work,
                                         int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_class_window_starts";
    DGRP_REQUIRE(h_count, "%s: NULL count", what);
    *h_count = 0;
    DGRP_REQUIRE(T >= 1 && T <= SET_MAXT, "%s: window of %d bases outside 1..%d", what, T, SET_MAXT);
    DGRP_REQUIRE(cap >= 0, "%s: negative capacity", what);
    int rc = prep_records(what, n_total, nrec, h_off, h_len);
    if (rc != DGRP_OK) return rc;
    std::vector<int64_t> tab((size_t)(3 * nrec + 1));                          // first workgroup [nrec + 1], off [nrec], len [nrec]
    int64_t blocks = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        tab[r] = blocks;
        tab[nrec + 1 + r] = h_off[r];
        tab[2 * nrec + 1 + r] = h_len[r];
        blocks += set_blocks_of(h_len[r], T);
    }
    if (nrec) tab[nrec] = blocks;
    if (blocks == 0) return DGRP_OK;
    DGRP_REQUIRE(blocks < (1ll << 31), "%s: too many bases", what);
    DGRP_REQUIRE(d_row && d_work && ((uintptr_t)d_work & 255) == 0, "%s: row or workspace NULL, or workspace not 256-byte aligned", what);
    if (work_bytes < set_workspace_bytes(nrec, blocks)) {                      // (records that overlap can need more than the companion says)
        dgrp_set_error("%s: workspace too small", what);
        return DGRP_ENOMEM;
    }
    uint64_t *d_total = (uint64_t *)d_work + 2;
    char *p = (char *)d_work + PREP_HEAD;
    int64_t *d_tab = (int64_t *)p;
    p += dgrp_align_up((3 * nrec + 1) * 8, 256);
    uint64_t *d_count = (uint64_t *)p;
    p += dgrp_align_up((blocks + 1) * 8, 256);
    uint64_t *d_tiles = (uint64_t *)p;
    const uint64_t *d_first = (const uint64_t *)d_tab;
    const int64_t *d_off = d_tab + nrec + 1, *d_len = d_tab + 2 * nrec + 1;
    uint64_t total = 0;
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(class_starts_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, d_row, d_first, nrec, d_off, d_len, T,
                           d_count, (int64_t *)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = device_exclusive_scan(d_count, d_count, blocks, d_tiles, d_total, stream);
    if (e == hipSuccess && rc == DGRP_OK) e = hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);                        // the one synchronisation (`tab` dies on return)
    DGRP_HIP(e);
    if (rc != DGRP_OK) return rc;
    DGRP_HIP(e2);
    *h_count = (int64_t)total;
    if (!d_starts || total == 0) return DGRP_OK;                               // count only
    if ((int64_t)total > cap) {
        dgrp_set_error("%s: %lld starts for a capacity of %lld", what, (long long)total, (long long)cap);
        return DGRP_ENOMEM;
    }
    hipLaunchKernelGGL(class_starts_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, d_row, d_first, nrec, d_off, d_len, T,
                       d_count, d_starts);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_train_resolve_starts(const int64_t *d_picks, int64_t B, const int64_t *const *d_set_ptr,
                                          const int64_t *d_set_size, int nsets, const int64_t *d_base, const int64_t *d_wprefix,
                                          int64_t nrec, int64_t *d_starts, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "dgrp_train_resolve_starts";
    DGRP_REQUIRE(B >= 1 && B <= (1 << 18), "%s: batch size %lld outside 1..2^18", what, (long long)B);
    DGRP_REQUIRE(nsets >= 0 && nsets <= DGRP_MAXC, "%s: %d sets outside 0..%d", what, nsets, DGRP_MAXC);
    DGRP_REQUIRE(nrec >= 1, "%s: no record", what);
    DGRP_REQUIRE(d_picks && d_base && d_wprefix && d_starts && (nsets == 0 || (d_set_ptr && d_set_size)), "%s: NULL pointer", what);
    hipLaunchKernelGGL(resolve_starts_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, d_picks, B, d_set_ptr, d_set_size,
                       nsets, d_base, d_wprefix, nrec, d_starts);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
