// predict --bed_rmout: the scored rows as the lines of a RepeatMasker `.out` listing, written on the device (dgrp_rmout_text_batch;
// deepgrp_amd/rmout.py states the format).  A line is
//   "%5d %5s %4s %4s  %-16s %9d %9d %11s +  %-12s %-16s %6d %6d %6s %6d\n" %
//       (score, "0.0", "0.0", "0.0", name, start + 1, end, "(rec_end - end)", repeat, class/family, 1, end - start, "(0)", ID)
// every field max(width, its digits or bytes) wide.  On the figures, decimal writers, refusals and workspace head of bed_rows.h;
// integers only, plain stores, no atomics.
//
// The chain.  check (one thread per row, a flag word per kind of refusal) -> emitted flag per row -> exclusive scan (scan.h: the
// ordinals; the emitted row in front of ordinal e is the row in front of the first index whose scan value reaches e, one binary
// search) -> head-of-ID flag per emitted row (another record, another label, a gap above join_gap, or no join at all) -> scan (the
// IDs) -> line length per row -> scan (the offsets) -> ONE read-back of totals and flags, the only synchronisation -> write, one
// thread per emitted row.  A row the check refuses is never emitted, so nothing it names is read behind the check.
#include "dgrp_common.h"
#include "bed_rows.h"
#include "scan.h"
#include <string.h>
#include <vector>

namespace {

#define RMOUT_MAX_END (1ll << 62)

struct rmout_in {
    const dgrp_segment *rows;
    const dgrp_row_score *scores;
    int64_t nrows;
    const int64_t *name_off;       // device copies of the host tables
    const char *names;
    int64_t nnames;
    const int64_t *cname_off;      // 2 entries per label: repeat, class/family
    const char *cnames;
    int64_t ncnames;               // labels
    const int64_t *rec_end;
    int64_t nrec;
    int by_contig;
    uint64_t min_score;
    int64_t join_gap;              // -1: every line its own ID
    uint64_t id0;
};

__device__ __forceinline__ int64_t rmout_rec(const rmout_in &A, const dgrp_segment &row) { return A.by_contig ? row.contig : 0; }

// whether everything the later kernels read for this row exists and is in range (what the check kernel refuses otherwise)
__device__ __forceinline__ bool rmout_sound(const rmout_in &A, const dgrp_segment &row, const dgrp_row_score &sc)
{
    const int64_t r = rmout_rec(A, row);
    return bed_scored(sc) && r >= 0 && r < A.nnames && r < A.nrec && row.label >= 1 && row.label <= A.ncnames && row.start >= 0 &&
           row.start < row.end && row.end <= A.rec_end[r];
}

// One thread per row: every refusal raises its flag word (plain stores of the same value).
__global__ void __launch_bounds__(256) rmout_check_kernel(rmout_in A, uint32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_segment row = A.rows[i];
    const dgrp_row_score sc = A.scores[i];
    const int64_t r = rmout_rec(A, row);
    if (sc.bases <= 0) flags[F_BASES] = 1;
    else if (!bed_scored(sc)) flags[F_RANGE] = 1;
    if (r < 0 || r >= A.nnames) flags[F_NAME] = 1;
    if (row.label < 1 || row.label > A.ncnames) flags[F_LABEL] = 1;
    if (row.start < 0 || row.start >= row.end) flags[F_SPAN] = 1;
    if (r < 0 || r >= A.nrec || row.end > A.rec_end[r]) flags[F_END] = 1;
    if (i > 0 && r < rmout_rec(A, A.rows[i - 1])) flags[F_RECORDS] = 1;
}

// One thread per row: 1 where the row gets a line.
__global__ void __launch_bounds__(256) rmout_emit_kernel(rmout_in A, uint64_t *__restrict__ emit)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_row_score sc = A.scores[i];
    emit[i] = rmout_sound(A, A.rows[i], sc) && bed_figures(sc).score >= A.min_score;
}

// One thread per row: 1 where an emitted row opens an ID, 0 where it takes the ID of the emitted row in front of it (and for a
// row without a line).  eidx is the exclusive scan of emit: it rises by one behind every emitted row, so the emitted row of ordinal
// e - 1 stands directly in front of the first index whose value is e.
__global__ void __launch_bounds__(256) rmout_heads_kernel(rmout_in A, const uint64_t *__restrict__ emit, const uint64_t *__restrict__ eidx,
                                                          uint64_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    uint64_t h = 0;
    if (emit[i]) {
        const uint64_t e = eidx[i];
        h = 1;
        if (e > 0 && A.join_gap >= 0) {
            const int64_t p = lower_bound_u64(eidx, i + 1, e) - 1;      // (0 <= p < i: eidx[0] = 0 < e and eidx[i] = e)
            const dgrp_segment row = A.rows[i], prev = A.rows[p];
            if (rmout_rec(A, row) == rmout_rec(A, prev) && row.label == prev.label && row.start - prev.end <= A.join_gap) h = 0;
        }
    }
    head[i] = h;
}

__device__ __forceinline__ uint64_t wider(uint64_t width, uint64_t n) { return n > width ? n : width; }

// the ID of an emitted row: the heads in front of it, itself included
__device__ __forceinline__ uint64_t rmout_id(const rmout_in &A, const uint64_t *head, const uint64_t *hidx, int64_t i)
{
    return A.id0 + hidx[i] + head[i];
}

// the two fixed spans of a line: " %5s %4s %4s  " of three "0.0" behind the score, " +  " behind (left)
#define RMOUT_ZEROS "   0.0  0.0  0.0  "
#define RMOUT_STRAND " +  "

template <int N> __device__ __forceinline__ char *put_lit(char *o, const char (&s)[N])
{
#pragma unroll
    for (int k = 0; k < N - 1; ++k) o[k] = s[k];
    return o + (N - 1);
}

__device__ __forceinline__ char *put_spaces(char *o, int64_t n)
{
    for (int64_t k = 0; k < n; ++k) o[k] = ' ';
    return o + (n > 0 ? n : 0);
}

// "%<width>d" of a value that is not negative
__device__ __forceinline__ char *put_right(char *o, uint64_t v, int width)
{
    o = put_spaces(o, width - dec_chars(v));
    return put_dec(o, v);
}

// "%-<width>s"
__device__ __forceinline__ char *put_left(char *o, const char *s, int64_t n, int width)
{
    for (int64_t k = 0; k < n; ++k) o[k] = s[k];
    return put_spaces(o + n, width - n);
}

// One thread per row: the line's length from its fields, 0 for a row without a line.
__global__ void __launch_bounds__(256) rmout_rows_kernel(rmout_in A, const uint64_t *__restrict__ emit, const uint64_t *__restrict__ head,
                                                         const uint64_t *__restrict__ hidx, uint64_t *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    uint64_t n = 0;
    if (emit[i]) {
        const dgrp_segment row = A.rows[i];
        const bed_figs f = bed_figures(A.scores[i]);
        const int64_t r = rmout_rec(A, row), c = 2 * (int64_t)(row.label - 1);
        n = wider(5, dec_chars(f.score)) + (sizeof(RMOUT_ZEROS) - 1) + wider(16, (uint64_t)(A.name_off[r + 1] - A.name_off[r])) + 1 +
            wider(9, dec_chars((uint64_t)row.start + 1)) + 1 + wider(9, dec_chars((uint64_t)row.end)) + 1 +
            wider(11, 2 + dec_chars((uint64_t)(A.rec_end[r] - row.end))) + (sizeof(RMOUT_STRAND) - 1) +
            wider(12, (uint64_t)(A.cname_off[c + 1] - A.cname_off[c])) + 1 + wider(16, (uint64_t)(A.cname_off[c + 2] - A.cname_off[c + 1])) + 1 +
            6 + 1 + wider(6, dec_chars((uint64_t)(row.end - row.start))) + 1 + 6 + 1 + wider(6, dec_chars(rmout_id(A, head, hidx, i))) + 1;
    }
    len[i] = n;
}

// One thread per emitted row: its line at its offset, field by field from left to right.
__global__ void __launch_bounds__(256) rmout_write_kernel(rmout_in A, const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                          const uint64_t *__restrict__ head, const uint64_t *__restrict__ hidx,
                                                          char *__restrict__ text)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const bed_figs f = bed_figures(A.scores[i]);
    const int64_t r = rmout_rec(A, row), c = 2 * (int64_t)(row.label - 1);
    const uint64_t left = (uint64_t)(A.rec_end[r] - row.end);
    char *o = text + off[i];
    o = put_right(o, f.score, 5);
    o = put_lit(o, RMOUT_ZEROS);
    o = put_left(o, A.names + A.name_off[r], A.name_off[r + 1] - A.name_off[r], 16); *o++ = ' ';
    o = put_right(o, (uint64_t)row.start + 1, 9); *o++ = ' ';
    o = put_right(o, (uint64_t)row.end, 9); *o++ = ' ';
    o = put_spaces(o, 11 - 2 - dec_chars(left));
    *o++ = '('; o = put_dec(o, left); *o++ = ')';
    o = put_lit(o, RMOUT_STRAND);
    o = put_left(o, A.cnames + A.cname_off[c], A.cname_off[c + 1] - A.cname_off[c], 12); *o++ = ' ';
    o = put_left(o, A.cnames + A.cname_off[c + 1], A.cname_off[c + 2] - A.cname_off[c + 1], 16); *o++ = ' ';
    o = put_lit(o, "     1 ");
    o = put_right(o, (uint64_t)(row.end - row.start), 6); *o++ = ' ';
    o = put_lit(o, "   (0) ");
    o = put_right(o, rmout_id(A, head, hidx, i), 6); *o++ = '\n';
}

// ---- the workspace -------------------------------------------------------------------------------------------------------------
struct rmout_layout {
    int64_t name_off, cname_off, rec_end, names, cnames, tables_bytes;         // inside the uploaded tables
    int64_t tables, emit, eidx, head, hidx, len, off, tiles;
    int64_t bytes;
};

static bool rmout_carve(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes, int64_t nrec,
                        rmout_layout *l)
{
    const int64_t top = (1ll << 31) - 1;
    if (nrows < 0 || nrows >= BED_MAX_ROWS || nnames < 1 || nnames > top || names_bytes < 0 || names_bytes > (1ll << 40)) return false;
    if (ncnames < 1 || ncnames > top / 2 || cnames_bytes < 0 || cnames_bytes > (1ll << 40) || nrec < 1 || nrec > top) return false;
    l->name_off = 0;
    l->cname_off = l->name_off + (nnames + 1) * 8;
    l->rec_end = l->cname_off + (2 * ncnames + 1) * 8;
    l->names = l->rec_end + nrec * 8;
    l->cnames = l->names + names_bytes;
    l->tables_bytes = l->cnames + cnames_bytes;
    const int64_t ntiles = (nrows + SCAN_TILE - 1) / SCAN_TILE, col = dgrp_align_up(nrows * 8, 256);
    int64_t p = 256;                                           // totals and flags
    l->tables = p; p += dgrp_align_up(l->tables_bytes, 256);
    l->emit = p; p += col;
    l->eidx = p; p += col;
    l->head = p; p += col;
    l->hidx = p; p += col;
    l->len = p; p += col;
    l->off = p; p += col;
    l->tiles = p; p += dgrp_align_up(ntiles * 8, 256);
    l->bytes = p;
    return true;
}

static int rmout_check_table(const char *who, const char *what, const char *bytes, const int64_t *off, int64_t n)
{
    DGRP_REQUIRE(bytes && off, "%s: bad arguments (%s)", who, what);
    DGRP_REQUIRE(off[0] >= 0, "%s: %s offsets must start at or above 0", who, what);
    for (int64_t i = 0; i < n; ++i) DGRP_REQUIRE(off[i + 1] >= off[i], "%s: %s offsets must ascend", who, what);
    return DGRP_OK;
}

}   // namespace

DGRP_EXPORT int64_t dgrp_rmout_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes,
                                                    int64_t nrec)
{
    rmout_layout l;
    return rmout_carve(nrows, nnames, names_bytes, ncnames, cnames_bytes, nrec, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_rmout_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                                      const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                                      int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end, int64_t join_gap, int64_t id0,
                                      char *d_text, int64_t cap, int64_t *h_bytes, int64_t *h_lines, int64_t *h_ids, void *d_work,
                                      int64_t work_bytes, void *stream_)
{
    const char *who = "dgrp_rmout_text_batch";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_bytes && h_lines && h_ids && nrows >= 0 && cap >= 0, "%s: bad arguments", who);
    DGRP_REQUIRE(nrows < BED_MAX_ROWS, "%s: too many rows (%lld, at or above 2^31 - 256)", who, (long long)nrows);
    DGRP_REQUIRE(nnames >= 1 && nnames <= (1ll << 31) - 1, "%s: bad name count %lld", who, (long long)nnames);
    int rc = rmout_check_table(who, "name", names, name_off, nnames);
    if (rc != DGRP_OK) return rc;
    DGRP_REQUIRE(ncnames >= 1 && ncnames <= ((1ll << 31) - 1) / 2, "%s: bad class-name count %lld (one pair per label, at least one)", who,
                 (long long)ncnames);
    rc = rmout_check_table(who, "class-name", cnames, cname_off, 2 * ncnames);
    if (rc != DGRP_OK) return rc;
    DGRP_REQUIRE(id0 >= 0 && id0 <= (1ll << 62), "%s: id0 %lld outside 0..2^62 (the IDs in front of this text)", who, (long long)id0);
    DGRP_REQUIRE(join_gap >= -1, "%s: join_gap %lld below -1 (-1: no join)", who, (long long)join_gap);
    DGRP_REQUIRE(nrec >= 1 && nrec <= (1ll << 31) - 1 && h_rec_end, "%s: bad nrec %lld or no record ends", who, (long long)nrec);
    DGRP_REQUIRE(by_contig || nrec == 1, "%s: without by_contig every row belongs to record 0, so nrec must be 1, not %lld", who, (long long)nrec);
    for (int64_t r = 0; r < nrec; ++r)
        DGRP_REQUIRE(h_rec_end[r] >= 1 && h_rec_end[r] <= RMOUT_MAX_END, "%s: record %lld ends at %lld, outside 1..2^62", who, (long long)r,
                     (long long)h_rec_end[r]);
    *h_bytes = *h_lines = *h_ids = 0;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && (d_text || cap == 0), "%s: bad arguments (NULL rows, scores or text)", who);
    rmout_layout l;
    DGRP_REQUIRE(rmout_carve(nrows, nnames, name_off[nnames], ncnames, cname_off[2 * ncnames], nrec, &l),
                 "%s: too many rows, names or records (%lld, %lld, %lld)", who, (long long)nrows, (long long)nnames, (long long)nrec);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<char> tab((size_t)l.tables_bytes, 0);           // (alive until the synchronisation below)
    memcpy(tab.data() + l.name_off, name_off, (size_t)(nnames + 1) * 8);
    memcpy(tab.data() + l.cname_off, cname_off, (size_t)(2 * ncnames + 1) * 8);
    memcpy(tab.data() + l.rec_end, h_rec_end, (size_t)nrec * 8);
    if (name_off[nnames] > 0) memcpy(tab.data() + l.names, names, (size_t)name_off[nnames]);
    if (cname_off[2 * ncnames] > 0) memcpy(tab.data() + l.cnames, cnames, (size_t)cname_off[2 * ncnames]);
    DGRP_HIP(hipMemcpyAsync(w + l.tables, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemsetAsync(w, 0, 256, stream));
    bed_head *d_head = (bed_head *)w;                           // (chunks: the IDs used)
    rmout_in A;
    A.rows = d_rows; A.scores = d_scores; A.nrows = nrows;
    A.name_off = (const int64_t *)(w + l.tables + l.name_off);
    A.names = w + l.tables + l.names;
    A.nnames = nnames;
    A.cname_off = (const int64_t *)(w + l.tables + l.cname_off);
    A.cnames = w + l.tables + l.cnames;
    A.ncnames = ncnames;
    A.rec_end = (const int64_t *)(w + l.tables + l.rec_end);
    A.nrec = nrec;
    A.by_contig = by_contig != 0;
    A.min_score = (uint64_t)(min_score < 0 ? 0 : min_score);
    A.join_gap = join_gap; A.id0 = (uint64_t)id0;
    uint64_t *emit = (uint64_t *)(w + l.emit), *eidx = (uint64_t *)(w + l.eidx), *head = (uint64_t *)(w + l.head);
    uint64_t *hidx = (uint64_t *)(w + l.hidx), *len = (uint64_t *)(w + l.len), *off = (uint64_t *)(w + l.off), *tiles = (uint64_t *)(w + l.tiles);
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    hipLaunchKernelGGL(rmout_check_kernel, grid, block, 0, stream, A, d_head->flags);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(rmout_emit_kernel, grid, block, 0, stream, A, emit);
    DGRP_LAUNCH_CHECK();
    rc = device_exclusive_scan(emit, eidx, nrows, tiles, &d_head->lines, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(rmout_heads_kernel, grid, block, 0, stream, A, (const uint64_t *)emit, (const uint64_t *)eidx, head);
    DGRP_LAUNCH_CHECK();
    rc = device_exclusive_scan(head, hidx, nrows, tiles, &d_head->chunks, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(rmout_rows_kernel, grid, block, 0, stream, A, (const uint64_t *)emit, (const uint64_t *)head, (const uint64_t *)hidx, len);
    DGRP_LAUNCH_CHECK();
    rc = device_exclusive_scan(len, off, nrows, tiles, &d_head->bytes, stream);
    if (rc != DGRP_OK) return rc;
    bed_head h;
    DGRP_HIP(hipMemcpyAsync(&h, w, sizeof h, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc = bed_refusal(who, h);
    if (rc != DGRP_OK) return rc;
    *h_bytes = (int64_t)h.bytes;
    *h_lines = (int64_t)h.lines;
    *h_ids = (int64_t)h.chunks;
    if (h.bytes == 0 || (int64_t)h.bytes > cap) return DGRP_OK;                 // (too small: the caller retries with room for all of it)
    hipLaunchKernelGGL(rmout_write_kernel, grid, block, 0, stream, A, (const uint64_t *)len, (const uint64_t *)off, (const uint64_t *)head,
                       (const uint64_t *)hidx, d_text);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
