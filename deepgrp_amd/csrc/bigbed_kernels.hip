// predict --bed_bigbed: the scored rows of bed_kernels.hip (on the figures, writers and refusals of bed_rows.h) as the items of a
// bigBed file (deepgrp_amd/bigbed.py states the format).  Two entries, each a chain on the caller's stream with ONE read-back
// (totals and the check's flags) in front of the only kernel that writes an output:
//   * dgrp_bed_blocks_batch: rows (one thread per row: every check, whether the row is emitted, its item's size) -> scans of the
//     emitted flags and of the sizes (scan.h) -> per record, two binary searches over the rows' ascending records give its emitted
//     rows, hence its blocks (ceil(rows / 512)), scanned -> compaction (emitted ordinal -> row) -> write: one thread per emitted row
//     writes its item at its scanned offset; the thread of a block's first item finds the block's last one through the compaction
//     and writes the whole table row.
//   * dgrp_bed_zoom_batch: rows -> scans of the emitted flags and of the emitted rows' lengths -> compaction of (record, start),
//     (record, end) keys and the length prefix -> level 0, one thread per window of 1024 bases: two binary searches over the keys
//     give the rows that touch the window, the length prefix their bases, the two edge rows are clipped -> nine reductions four to
//     one, count of the covered windows per 256, one scan, records and block table: the ladder of bbi_zoom.h with one class, which
//     bigwig_kernels.hip shares.
// A row is refused when it starts below the END of the row in front of it in its record.  That is the rule "below the largest end
// of the rows in front of it": where every row passes the test against its neighbour, start[i] >= end[i-1] > start[i-1] >=
// end[i-2] ..., so the ends ascend and the neighbour's end is the largest; where a row fails against the largest end, the first
// such row fails against its neighbour, whose end is then still the largest.  Integers only, no atomics.
#include "dgrp_common.h"
#include "bbi_zoom.h"
#include "bed_rows.h"
#include "scan.h"
#include <string.h>
#include <vector>

namespace {

#define BB_BLOCK_ITEMS 512
#define BB_ITEM_MAX 60                     // see include/deepgrp_hip.h: 512 items are at most 30720 bytes
#define BB_MAX_END 0xffffffffll
#define BB_R0 1024                         // bases of a level-0 window

struct bb_in {
    const dgrp_segment *rows;
    const dgrp_row_score *scores;
    int64_t nrows;
    const int64_t *rec_end;                // device copy of the host table
    int64_t nrec;
    int by_contig;
    uint64_t min_score;
};

__device__ __forceinline__ int64_t bb_rec(const bb_in &A, const dgrp_segment &row) { return A.by_contig ? row.contig : 0; }

// One thread per row: every refusal raises its flag word; emit = 1, size = the item's bytes and len = the row's bases where the
// row is emitted, all 0 for a filtered row and for a row the check refuses (nothing it names is read).  size or len may be NULL.
__global__ void __launch_bounds__(256) bb_rows_kernel(bb_in A, uint32_t *__restrict__ flags, uint64_t *__restrict__ emit,
                                                      uint64_t *__restrict__ size, uint64_t *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_segment row = A.rows[i];
    const dgrp_row_score sc = A.scores[i];
    const int64_t r = bb_rec(A, row);
    bool ok = true;
    if (sc.bases <= 0) { flags[F_BASES] = 1; ok = false; }
    else if (!bed_scored(sc)) { flags[F_RANGE] = 1; ok = false; }
    if (row.start < 0 || row.start >= row.end) { flags[F_SPAN] = 1; ok = false; }
    if (r < 0 || r >= A.nrec || row.end > A.rec_end[r]) { flags[F_END] = 1; ok = false; }
    if (i > 0) {
        const dgrp_segment prev = A.rows[i - 1];
        const int64_t rp = bb_rec(A, prev);
        if (r < rp) flags[F_RECORDS] = 1;
        if (r == rp && row.start < prev.end) flags[F_OVERLAP] = 1;
    }
    uint64_t n = 0, l = 0;
    if (ok) {
        const bed_figs f = bed_figures(sc);
        if (f.score >= A.min_score) {
            // chromId, start, end; "class" label, score, ".", three "d.dddd" figures, five tabs and the zero byte
            n = 12 + 5 + int_chars(row.label) + dec_chars(f.score) + 1 + dec_chars(f.mean / 10000) + dec_chars(f.qmin / 10000) +
                dec_chars(f.agree / 10000) + 15 + 6;
            l = (uint64_t)(row.end - row.start);
        }
    }
    emit[i] = n != 0;
    if (size) size[i] = n;
    if (len) len[i] = l;
}

// the first row whose record is at least r (the records ascend with the rows)
__device__ __forceinline__ int64_t bb_first_row(const bb_in &A, int64_t r)
{
    int64_t lo = 0, hi = A.nrows;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (bb_rec(A, A.rows[mid]) < r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One thread per record (and one more): rec_e[r] = the emitted rows in front of record r (rec_e[nrec]: all of them), nblk[r] its
// blocks.
__global__ void __launch_bounds__(256) bb_records_kernel(bb_in A, const uint64_t *__restrict__ eidx, const uint64_t *__restrict__ items,
                                                         uint64_t *__restrict__ rec_e, uint64_t *__restrict__ nblk)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > A.nrec) return;
    const int64_t a = bb_first_row(A, r);
    const uint64_t ea = a < A.nrows ? eidx[a] : *items;
    rec_e[r] = ea;
    if (r == A.nrec) {
        nblk[r] = 0;
        return;
    }
    const int64_t b = bb_first_row(A, r + 1);
    const uint64_t eb = b < A.nrows ? eidx[b] : *items;
    nblk[r] = (eb - ea + BB_BLOCK_ITEMS - 1) / BB_BLOCK_ITEMS;
}

// One thread per row: emitted row i is the eidx[i]-th emitted row.
__global__ void __launch_bounds__(256) bb_order_kernel(int64_t nrows, const uint64_t *__restrict__ size, const uint64_t *__restrict__ eidx,
                                                       uint32_t *__restrict__ order)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nrows && size[i] != 0) order[eidx[i]] = (uint32_t)i;
}

__device__ __forceinline__ char *put_u32le(char *o, uint32_t v)
{
    o[0] = (char)v; o[1] = (char)(v >> 8); o[2] = (char)(v >> 16); o[3] = (char)(v >> 24);
    return o + 4;
}

// One thread per emitted row: its item at its offset; the first item of a block also writes the block's table row.
__global__ void __launch_bounds__(256) bb_write_kernel(bb_in A, const uint64_t *__restrict__ size, const uint64_t *__restrict__ off,
                                                       const uint64_t *__restrict__ eidx, const uint32_t *__restrict__ order,
                                                       const uint64_t *__restrict__ rec_e, const uint64_t *__restrict__ bpref, uint32_t chrom0,
                                                       char *__restrict__ out, dgrp_bed_block *__restrict__ table)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || size[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const bed_figs f = bed_figures(A.scores[i]);
    const int64_t r = bb_rec(A, row);
    char *o = out + off[i];
    o = put_u32le(o, chrom0 + (uint32_t)r);
    o = put_u32le(o, (uint32_t)row.start);
    o = put_u32le(o, (uint32_t)row.end);
    *o++ = 'c'; *o++ = 'l'; *o++ = 'a'; *o++ = 's'; *o++ = 's';
    o = put_int(o, row.label); *o++ = '\t';
    o = put_dec(o, f.score); *o++ = '\t';
    *o++ = '.'; *o++ = '\t';
    o = put_fixed4(o, f.mean); *o++ = '\t';
    o = put_fixed4(o, f.qmin); *o++ = '\t';
    o = put_fixed4(o, f.agree); *o++ = 0;
    const uint64_t j = eidx[i] - rec_e[r];                                 // the row's ordinal among its record's emitted rows
    if (j % BB_BLOCK_ITEMS != 0) return;
    const uint64_t left = rec_e[r + 1] - rec_e[r] - j, count = left < BB_BLOCK_ITEMS ? left : BB_BLOCK_ITEMS;
    const int64_t last = order[eidx[i] + count - 1];
    dgrp_bed_block b;
    b.off = (int64_t)off[i];
    b.bytes = (int64_t)(off[last] + size[last] - off[i]);
    b.rec = (int32_t)r;
    b.start = (uint32_t)row.start;
    b.end = (uint32_t)A.rows[last].end;
    b.items = (uint32_t)count;
    table[bpref[r] + j / BB_BLOCK_ITEMS] = b;
}

// ---- zoom ----------------------------------------------------------------------------------------------------------------------
struct bbz_win { uint32_t start, end, valid; };                           // a window's coverage; valid 0: none
struct bbz_rows {                          // the emitted rows, compacted: *count of them
    const uint64_t *count;
    uint64_t *skey, *ekey;                 // record << 32 | start, record << 32 | end: both ascend
    uint64_t *lpref;                       // bases of the emitted rows in front
};

// One thread per row: an emitted row becomes compacted row eidx[i].
__global__ void __launch_bounds__(256) bbz_compact_kernel(bb_in A, const uint64_t *__restrict__ len, const uint64_t *__restrict__ lsum,
                                                          const uint64_t *__restrict__ eidx, bbz_rows Rw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const uint64_t j = eidx[i], r = (uint64_t)bb_rec(A, row) << 32;
    Rw.skey[j] = r | (uint64_t)row.start;
    Rw.ekey[j] = r | (uint64_t)row.end;
    Rw.lpref[j] = lsum[i];
}

__device__ __forceinline__ bbz_win bbi_join(const bbz_win &a, const bbz_win &b)      // every base of b above every base of a
{
    if (a.valid == 0) return b;
    if (b.valid == 0) return a;
    bbz_win w;
    w.start = a.start; w.end = b.end; w.valid = a.valid + b.valid;
    return w;
}

struct bbz_start {                         // every record starts at base 0
    __device__ __forceinline__ int64_t operator()(int64_t) const { return 0; }
};

struct bbz_tail {                          // coverage: the value 1 on every covered base
    __device__ __forceinline__ uint4 operator()(const bbz_win &w) const
    {
        const uint32_t one = __float_as_uint(1.0f), sum = __float_as_uint((float)w.valid);
        uint4 b;
        b.x = one; b.y = one; b.z = sum; b.w = sum;
        return b;
    }
};

// level 0: one thread per window of 1024 bases.  The rows that touch [a, b) of record r are [lo, hi): lo the first row that ends
// above a, hi the first row that starts at or above b; their bases come from the length prefix, the two edge rows are clipped.
__global__ void __launch_bounds__(256) bbz_level0_kernel(bbz_rows Rw, const int64_t *__restrict__ rec_end, const int64_t *__restrict__ wpref,
                                                         int64_t nrec, bbi_levels Z, bbz_win *__restrict__ win)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bbz_win w = bbz_win();
    if (i < Z.W[0]) {
        const int64_t r = dgrp_record_of(wpref, nrec, i), m = (int64_t)*Rw.count;
        const uint64_t a = (uint64_t)(i - wpref[r]) * BB_R0, top = (uint64_t)rec_end[r];
        const uint64_t b = a + BB_R0 < top ? a + BB_R0 : top, key = (uint64_t)r << 32;
        const int64_t lo = lower_bound_u64(Rw.ekey, m, (key | a) + 1), hi = lower_bound_u64(Rw.skey, m, key | b);
        if (lo < hi) {
            const uint64_t s0 = Rw.skey[lo] & 0xffffffffull, e1 = Rw.ekey[hi - 1] & 0xffffffffull, s1 = Rw.skey[hi - 1] & 0xffffffffull;
            const uint64_t s = s0 > a ? s0 : a, e = e1 < b ? e1 : b;
            w.start = (uint32_t)s;
            w.end = (uint32_t)e;
            w.valid = (uint32_t)(Rw.lpref[hi - 1] + (e1 - s1) - Rw.lpref[lo] - (s - s0) - (e1 - e));
        }
    }
    win[Z.seg[0] + i] = w;
}

// ---- arguments and workspaces --------------------------------------------------------------------------------------------------
static bool bb_in_range(int64_t nrows, int64_t nrec, const int64_t *h_rec_end)
{
    if (nrows < 0 || nrows > BED_MAX_ROWS || nrec < 1 || nrec > (1ll << 31) - 1 || !h_rec_end) return false;
    for (int64_t r = 0; r < nrec; ++r)
        if (h_rec_end[r] < 1 || h_rec_end[r] > BB_MAX_END) return false;
    return true;
}

static int bb_check(const char *who, int by_contig, int64_t nrows, int64_t nrec, const int64_t *h_rec_end, int64_t chrom0, int64_t cap,
                    int64_t table_cap)
{
    DGRP_REQUIRE(nrows >= 0 && nrows <= BED_MAX_ROWS, "%s: bad nrows %lld", who, (long long)nrows);
    DGRP_REQUIRE(nrec >= 1 && nrec <= (1ll << 31) - 1 && h_rec_end, "%s: bad nrec %lld or no record ends", who, (long long)nrec);
    DGRP_REQUIRE(by_contig || nrec == 1, "%s: without by_contig every row belongs to record 0, so nrec must be 1, not %lld", who, (long long)nrec);
    for (int64_t r = 0; r < nrec; ++r)
        DGRP_REQUIRE(h_rec_end[r] >= 1 && h_rec_end[r] <= BB_MAX_END,
                     "%s: record %lld ends at %lld, outside 1..2^32 - 1 = 4294967295 (the largest coordinate of a bigBed)", who, (long long)r,
                     (long long)h_rec_end[r]);
    DGRP_REQUIRE(chrom0 >= 0 && chrom0 + nrec <= BB_MAX_END, "%s: bad first chromId %lld", who, (long long)chrom0);
    DGRP_REQUIRE(cap >= 0 && table_cap >= 0, "%s: bad cap/table_cap (%lld, %lld)", who, (long long)cap, (long long)table_cap);
    return DGRP_OK;
}

struct bb_layout { int64_t rec_end, eidx, size, off, order, tiles, rec_e, bpref, bytes; };

static void bb_carve(int64_t nrows, int64_t nrec, bb_layout *l)
{
    const int64_t col = dgrp_align_up(nrows * 8, 256), most = nrows > nrec + 1 ? nrows : nrec + 1;
    int64_t p = 256;                                           // totals and flags (bed_head)
    l->rec_end = p; p += dgrp_align_up(nrec * 8, 256);
    l->eidx = p; p += col;
    l->size = p; p += col;
    l->off = p; p += col;
    l->order = p; p += dgrp_align_up(nrows * 4, 256);
    l->tiles = p; p += dgrp_align_up((most + SCAN_TILE - 1) / SCAN_TILE * 8, 256);
    l->rec_e = p; p += dgrp_align_up((nrec + 1) * 8, 256);
    l->bpref = p; p += dgrp_align_up((nrec + 1) * 8, 256);
    l->bytes = p;
}

struct bbz_layout { bbi_levels Z; int64_t rec_end, wpref, eidx, len, lsum, skey, ekey, lpref, tiles, win, wtiles, grand, segb, bytes; };

static bool bbz_carve(int64_t nrows, int64_t nrec, const int64_t *h_rec_end, bbz_layout *l)
{
    const bbi_levels &Z = l->Z;
    if (!bbi_levels_of(BB_R0, 1, nrec, nullptr, h_rec_end, &l->Z)) return false;
    const int64_t col = dgrp_align_up(nrows * 8, 256);
    int64_t p = 256;                                           // totals and flags (bed_head)
    l->rec_end = p; p += dgrp_align_up(nrec * 8, 256);
    l->wpref = p; p += dgrp_align_up((nrec + 1) * BBI_LEVELS * 8, 256);
    l->eidx = p; p += col;
    l->len = p; p += col;
    l->lsum = p; p += col;
    l->skey = p; p += col;
    l->ekey = p; p += col;
    l->lpref = p; p += col;
    l->tiles = p; p += dgrp_align_up((nrows + SCAN_TILE - 1) / SCAN_TILE * 8, 256);
    l->win = p; p += dgrp_align_up(Z.seg[BBI_LEVELS] * (int64_t)sizeof(bbz_win), 256);
    l->wtiles = p; p += dgrp_align_up(Z.seg[BBI_LEVELS] / 256 * 8, 256);
    l->grand = p; p += 256;                                    // the records of all levels, the covered bases
    l->segb = p; p += dgrp_align_up(2 * (BBI_LEVELS + 1) * 8, 256);
    l->bytes = p;
    return true;
}

// The shared front on checked arguments: the record ends up (`tab` lives until the caller's synchronisation), totals and flags
// cleared, the rows kernel, the scan of the emitted flags (its total: head->lines).  No synchronisation.
static int bb_front(int by_contig, const dgrp_segment *d_rows, const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec,
                    const int64_t *h_rec_end, char *w, int64_t at_rec_end, int64_t at_eidx, int64_t at_size, int64_t at_len, int64_t at_tiles,
                    hipStream_t stream, std::vector<int64_t> &tab, bb_in *A)
{
    tab.assign(h_rec_end, h_rec_end + nrec);
    DGRP_HIP(hipMemcpyAsync(w + at_rec_end, tab.data(), (size_t)nrec * 8, hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemsetAsync(w, 0, 256, stream));
    bed_head *head = (bed_head *)w;
    A->rows = d_rows; A->scores = d_scores; A->nrows = nrows;
    A->rec_end = (const int64_t *)(w + at_rec_end);
    A->nrec = nrec; A->by_contig = by_contig != 0;
    A->min_score = (uint64_t)(min_score < 0 ? 0 : min_score);
    uint64_t *eidx = (uint64_t *)(w + at_eidx);
    hipLaunchKernelGGL(bb_rows_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, *A, head->flags, eidx,
                       at_size ? (uint64_t *)(w + at_size) : nullptr, at_len ? (uint64_t *)(w + at_len) : nullptr);
    DGRP_LAUNCH_CHECK();
    return device_exclusive_scan(eidx, eidx, nrows, (uint64_t *)(w + at_tiles), &head->lines, stream);
}

}   // namespace

DGRP_EXPORT int64_t dgrp_bed_blocks_workspace_bytes(int64_t nrows, int64_t nrec, const int64_t *h_rec_end)
{
    bb_layout l;
    if (!bb_in_range(nrows, nrec, h_rec_end)) return 0;
    bb_carve(nrows, nrec, &l);
    return l.bytes;
}

DGRP_EXPORT int dgrp_bed_blocks_batch(int by_contig, const dgrp_segment *d_rows, const dgrp_row_score *d_scores, int64_t nrows, int min_score,
                                      int64_t nrec, const int64_t *h_rec_end, int64_t chrom0, char *d_out, int64_t cap, int64_t *h_bytes,
                                      dgrp_bed_block *d_table, int64_t table_cap, int64_t *h_nblocks, int64_t *h_items, void *d_work,
                                      int64_t work_bytes, void *stream_)
{
    static const char who[] = "dgrp_bed_blocks_batch";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_bytes && h_nblocks && h_items, "%s: NULL h_bytes, h_nblocks or h_items", who);
    *h_bytes = *h_nblocks = *h_items = 0;
    const int rc = bb_check(who, by_contig, nrows, nrec, h_rec_end, chrom0, cap, table_cap);
    if (rc != DGRP_OK) return rc;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && (d_out || cap == 0) && (d_table || table_cap == 0), "%s: bad arguments (NULL rows, scores, output or table)",
                 who);
    DGRP_REQUIRE(((uintptr_t)d_table & 7) == 0, "%s: d_table must be 8-byte aligned", who);
    bb_layout l;
    bb_carve(nrows, nrec, &l);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<int64_t> tab;                                   // (alive until the synchronisation below)
    bb_in A;
    int rc2 = bb_front(by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end, w, l.rec_end, l.eidx, l.size, 0, l.tiles, stream, tab, &A);
    if (rc2 != DGRP_OK) return rc2;
    bed_head *d_head = (bed_head *)w;
    uint64_t *eidx = (uint64_t *)(w + l.eidx), *size = (uint64_t *)(w + l.size), *off = (uint64_t *)(w + l.off), *tiles = (uint64_t *)(w + l.tiles);
    uint64_t *rec_e = (uint64_t *)(w + l.rec_e), *bpref = (uint64_t *)(w + l.bpref);
    uint32_t *order = (uint32_t *)(w + l.order);
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    rc2 = device_exclusive_scan(size, off, nrows, tiles, &d_head->bytes, stream);
    if (rc2 != DGRP_OK) return rc2;
    hipLaunchKernelGGL(bb_records_kernel, dim3((unsigned)((nrec + 1 + 255) / 256)), block, 0, stream, A, (const uint64_t *)eidx,
                       (const uint64_t *)&d_head->lines, rec_e, bpref);
    DGRP_LAUNCH_CHECK();
    rc2 = device_exclusive_scan(bpref, bpref, nrec + 1, tiles, &d_head->chunks, stream);
    if (rc2 != DGRP_OK) return rc2;
    hipLaunchKernelGGL(bb_order_kernel, grid, block, 0, stream, nrows, (const uint64_t *)size, (const uint64_t *)eidx, order);
    DGRP_LAUNCH_CHECK();
    bed_head head;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    *h_bytes = (int64_t)head.bytes;
    *h_items = (int64_t)head.lines;
    *h_nblocks = (int64_t)head.chunks;
    if (head.lines == 0 || *h_bytes > cap || *h_nblocks > table_cap) return DGRP_OK;   // (too small: the caller retries with room for all of it)
    hipLaunchKernelGGL(bb_write_kernel, grid, block, 0, stream, A, (const uint64_t *)size, (const uint64_t *)off, (const uint64_t *)eidx,
                       (const uint32_t *)order, (const uint64_t *)rec_e, (const uint64_t *)bpref, (uint32_t)chrom0, d_out, d_table);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_bed_zoom_workspace_bytes(int64_t nrows, int64_t nrec, const int64_t *h_rec_end)
{
    bbz_layout l;
    if (!bb_in_range(nrows, nrec, h_rec_end)) return 0;
    return bbz_carve(nrows, nrec, h_rec_end, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_bed_zoom_batch(int by_contig, const dgrp_segment *d_rows, const dgrp_row_score *d_scores, int64_t nrows, int min_score,
                                    int64_t nrec, const int64_t *h_rec_end, int64_t chrom0, char *d_out, int64_t cap, int64_t *h_record_off,
                                    dgrp_track_zoom_block *d_table, int64_t table_cap, int64_t *h_block_off, dgrp_track_totals *h_totals,
                                    void *d_work, int64_t work_bytes, void *stream_)
{
    static const char who[] = "dgrp_bed_zoom_batch";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_record_off && h_block_off && h_totals, "%s: NULL h_record_off, h_block_off or h_totals", who);
    for (int s = 0; s <= BBI_LEVELS; ++s) h_record_off[s] = h_block_off[s] = 0;
    memset(h_totals, 0, sizeof *h_totals);
    const int rc = bb_check(who, by_contig, nrows, nrec, h_rec_end, chrom0, cap, table_cap);
    if (rc != DGRP_OK) return rc;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && (d_out || cap == 0) && (d_table || table_cap == 0), "%s: bad arguments (NULL rows, scores, output or table)",
                 who);
    DGRP_REQUIRE(((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_table & 7) == 0, "%s: d_out must be 16-byte and d_table 8-byte aligned", who);
    bbz_layout l;
    DGRP_REQUIRE(bbz_carve(nrows, nrec, h_rec_end, &l), "%s: too many zoom windows in one call", who);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    const bbi_levels &Z = l.Z;
    const std::vector<int64_t> wpref = bbi_wpref(Z, nrec, nullptr, h_rec_end);
    int64_t *d_wpref = (int64_t *)(w + l.wpref);
    DGRP_HIP(hipMemcpyAsync(d_wpref, wpref.data(), wpref.size() * 8, hipMemcpyHostToDevice, stream));
    std::vector<int64_t> tab;                                   // (both tables alive until the synchronisation below)
    bb_in A;
    int rc2 = bb_front(by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end, w, l.rec_end, l.eidx, 0, l.len, l.tiles, stream, tab, &A);
    if (rc2 != DGRP_OK) return rc2;
    bed_head *d_head = (bed_head *)w;
    uint64_t *eidx = (uint64_t *)(w + l.eidx), *len = (uint64_t *)(w + l.len), *tiles = (uint64_t *)(w + l.tiles);
    uint64_t *wtiles = (uint64_t *)(w + l.wtiles), *grand = (uint64_t *)(w + l.grand), *segb = (uint64_t *)(w + l.segb);
    bbz_win *win = (bbz_win *)(w + l.win);
    bbz_rows Rw;
    Rw.count = &d_head->lines;
    Rw.skey = (uint64_t *)(w + l.skey); Rw.ekey = (uint64_t *)(w + l.ekey); Rw.lpref = (uint64_t *)(w + l.lpref);
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    uint64_t *lsum = (uint64_t *)(w + l.lsum);
    rc2 = device_exclusive_scan(len, lsum, nrows, tiles, nullptr, stream);
    if (rc2 != DGRP_OK) return rc2;
    hipLaunchKernelGGL(bbz_compact_kernel, grid, block, 0, stream, A, (const uint64_t *)len, (const uint64_t *)lsum, (const uint64_t *)eidx, Rw);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bbz_level0_kernel, dim3((unsigned)((Z.seg[1] - Z.seg[0]) / 256)), block, 0, stream, Rw, A.rec_end, (const int64_t *)d_wpref,
                       nrec, Z, win);
    DGRP_LAUNCH_CHECK();
    for (int k = 1; k < BBI_LEVELS; ++k) {
        hipLaunchKernelGGL((bbi_reduce_kernel<bbz_win, bbz_start>), dim3((unsigned)((Z.seg[k + 1] - Z.seg[k]) / 256)), block, 0, stream, bbz_start(),
                           (const int64_t *)d_wpref, nrec, Z, k, win);
        DGRP_LAUNCH_CHECK();
    }
    const int64_t ntiles = Z.seg[BBI_LEVELS] / 256;
    hipLaunchKernelGGL(bbi_count_kernel<bbz_win>, dim3((unsigned)ntiles), block, 0, stream, (const bbz_win *)win, wtiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), block, 0, stream, wtiles, ntiles, grand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL((bbi_bounds_kernel<bbz_win, true>), dim3(1), block, 0, stream, (const bbz_win *)win, (const uint64_t *)wtiles,
                       (const uint64_t *)grand, Z, 1, segb, grand + 1);
    DGRP_LAUNCH_CHECK();
    bed_head head;
    uint64_t off[2 * (BBI_LEVELS + 1)], covered = 0;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(off, segb, sizeof off, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(&covered, grand + 1, 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    for (int s = 0; s <= BBI_LEVELS; ++s) {
        h_record_off[s] = (int64_t)off[s];
        h_block_off[s] = (int64_t)off[BBI_LEVELS + 1 + s];
    }
    if (covered) {
        h_totals->covered = h_totals->sum = h_totals->sumsq = covered;
        h_totals->qmin = h_totals->qmax = 1;
    }
    if (h_record_off[BBI_LEVELS] == 0 || 32 * h_record_off[BBI_LEVELS] > cap || h_block_off[BBI_LEVELS] > table_cap) return DGRP_OK;   // (the caller retries)
    hipLaunchKernelGGL((bbi_write_kernel<bbz_win, bbz_tail>), dim3((unsigned)ntiles), block, 0, stream, (const bbz_win *)win, (const int64_t *)d_wpref,
                       nrec, Z, bbz_tail(), (const uint64_t *)wtiles, (const uint64_t *)segb, 1, (uint32_t)chrom0, (uint4 *)d_out, d_table);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
