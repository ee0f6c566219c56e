// Rows as text -> arrays, on the device: the four-column table `evaluation.read_annotation` reads (contig, begin, end, number) and
// the TSV `predict` writes (file, header, start, end, label).  The text is in HBM (uploaded, or inflated there); what leaves it are
// the rows in file order with their name token as a span of the text, their line, and the first row of every run of one name.
// The grammar of each form is stated in include/deepgrp_hip.h (dgrp_rows_parse) and, as Python, in deepgrp_amd/compare.py; a file
// with a byte or a number that statement does not cover raises a flag and is parsed on the host.
//
// Work split: that of dgrp_rm_parse (text_lines.h) -- a workgroup takes a tile of RM_TILE bytes, a lane a chunk of 128 consecutive
// bytes and every line that STARTS in its chunk, walked byte by byte in global memory; a count pass and a write pass around the
// scans give every row its place.  Bytes and integers only; the only atomics are the OR of the flag and the min of the first
// malformed line's position, so the same call gives the same bytes.
#include "text_lines.h"

namespace {

#define ROWS_MIN_LINE 8                  // shortest row: `a 1 2 3` or two empty fields and `1 2 3` between tabs, and the line end
#define ROWS_MAX_DIGITS 18               // a number of more digits is left to the host
#define ROWS_NO_LINE (~0ull)             // g[1]: no malformed line yet

enum { ROWS_SKIP = 0, ROWS_ROW = 1, ROWS_SHORT = 2 };

struct rows_row {
    int64_t begin, end, number, name_pos, file_pos;
    int32_t name_len, file_len;
};

// [b, e) as 1..18 plain decimal digits, else `bad`
__host__ __device__ __forceinline__ int64_t rows_number(const uint8_t *__restrict__ t, int64_t b, int64_t e, bool &bad)
{
    if (e - b < 1 || e - b > ROWS_MAX_DIGITS) { bad = true; return 0; }
    int64_t val = 0;
    for (int64_t p = b; p < e; ++p) {
        const uint8_t c = t[p];
        if (c < '0' || c > '9') { bad = true; return 0; }
        val = val * 10 + (c - '0');
    }
    return val;
}

// The table line that starts at s: tokens between runs of blanks.  No token, or a first token that opens with '#': skipped; fewer
// than four tokens: short; else a row of tokens 0..3.
__host__ __device__ int rows_table_line(const uint8_t *__restrict__ t, int64_t s, int64_t n, rows_row &row, bool &bad)
{
    int64_t p = s, tb[4], te[4];
    for (int k = 0; k < 4; ++k) {
        while (p < n && rm_blank(t[p])) ++p;
        if (p >= n || rm_eol(t[p])) return k == 0 ? ROWS_SKIP : ROWS_SHORT;
        tb[k] = p;
        while (p < n && !rm_blank(t[p]) && !rm_eol(t[p])) ++p;
        te[k] = p;
        if (k == 0 && t[tb[0]] == '#') return ROWS_SKIP;
    }
    row.begin = rows_number(t, tb[1], te[1], bad);
    row.end = rows_number(t, tb[2], te[2], bad);
    row.number = rows_number(t, tb[3], te[3], bad);
    if (te[0] - tb[0] > 0x7fffffffll) bad = true;                           // (a name the int32 length cannot state)
    row.name_pos = tb[0];
    row.name_len = (int32_t)(te[0] - tb[0]);
    row.file_pos = tb[0];
    row.file_len = 0;
    return ROWS_ROW;
}

// The TSV line that starts at s: fields between single tabs.  Empty: skipped; fewer than five fields: short; else the first field
// is the file, the last three are start, end and label, and what lies between (tabs included) is the header.
__host__ __device__ int rows_tsv_line(const uint8_t *__restrict__ t, int64_t s, int64_t n, rows_row &row, bool &bad)
{
    int64_t p = s, first = -1, t1 = -1, t2 = -1, t3 = -1;                    // the first tab and the last three
    int tabs = 0;
    for (; p < n && !rm_eol(t[p]); ++p)
        if (t[p] == '\t') {
            if (tabs == 0) first = p;
            t1 = t2; t2 = t3; t3 = p;
            if (tabs < 4) ++tabs;
        }
    const int64_t e = p;
    if (e == s) return ROWS_SKIP;
    if (tabs < 4) return ROWS_SHORT;
    row.begin = rows_number(t, t1 + 1, t2, bad);
    row.end = rows_number(t, t2 + 1, t3, bad);
    row.number = rows_number(t, t3 + 1, e, bad);
    const int64_t fb = s, fe = first;
    int64_t nb, ne;
    if (fe - fb >= 4 && t[fe - 4] == '.' && t[fe - 3] == 'n' && t[fe - 2] == 'p' && t[fe - 1] == 'z') {
        nb = fb;                                                             // the basename up to its first '.'
        for (int64_t q = fb; q < fe; ++q)
            if (t[q] == '/') nb = q + 1;
        for (ne = nb; t[ne] != '.'; ++ne) {}
    } else {
        nb = first + 1;                                                      // the first word of the header
        while (nb < t1 && rm_blank(t[nb])) ++nb;
        for (ne = nb; ne < t1 && !rm_blank(t[ne]); ++ne) {}
    }
    if (ne - nb > 0x7fffffffll || fe - fb > 0x7fffffffll) bad = true;
    row.name_pos = nb;
    row.name_len = (int32_t)(ne - nb);
    row.file_pos = fb;
    row.file_len = (int32_t)(fe - fb);
    return ROWS_ROW;
}

struct rows_out {
    int64_t *begin, *end, *number, *name_pos;
    int32_t *name_len;
    int64_t *file_pos;                   // NULL for a table
    int32_t *file_len;
    int64_t *line;
    int64_t cap;
};

// The lines that start in the chunk [c0, c0 + RM_CHUNK) with the line feeds lo / hi: -> how many are rows; `shortest`: the smallest
// (start << 2 | reason) of its malformed lines.  WRITE: they are rows place, place + 1, ... and line0 line feeds lie in front of
// the chunk.
template <bool WRITE>
__host__ __device__ uint32_t rows_chunk_lines(const uint8_t *__restrict__ t, int64_t c0, int64_t n, int format, uint64_t lo, uint64_t hi,
                                              bool &bad, uint64_t &shortest, uint64_t place, uint64_t line0, const rows_out &out)
{
    const int64_t c1 = c0 + RM_CHUNK < n ? c0 + RM_CHUNK : n;
    uint32_t kept = 0, seen = 0;
    int64_t s = (c0 == 0 || t[c0 - 1] == '\n') ? c0 : -1;
    for (;;) {
        if (s < 0) {
            int k;
            if (lo) { k = __builtin_ctzll(lo); lo &= lo - 1; }
            else if (hi) { k = 64 + __builtin_ctzll(hi); hi &= hi - 1; }
            else break;
            ++seen;
            s = c0 + k + 1;
            if (s >= c1) break;                                              // the next chunk's line (or the end of the text)
        }
        rows_row row;
        const int what = format == 1 ? rows_tsv_line(t, s, n, row, bad) : rows_table_line(t, s, n, row, bad);
        if (what == ROWS_SHORT) {
            const uint64_t code = ((uint64_t)s << 2) | (uint64_t)(format == 1 ? 2 : 1);
            if (code < shortest) shortest = code;
        } else if (what == ROWS_ROW) {
            if (WRITE) {
                const int64_t i = (int64_t)(place + kept);
                if (i < out.cap) {
                    out.begin[i] = row.begin;
                    out.end[i] = row.end;
                    out.number[i] = row.number;
                    out.name_pos[i] = row.name_pos;
                    out.name_len[i] = row.name_len;
                    out.line[i] = (int64_t)(line0 + seen) + 1;
                    if (out.file_pos) {
                        out.file_pos[i] = row.file_pos;
                        out.file_len[i] = row.file_len;
                    }
                }
            }
            ++kept;
        }
        s = -1;
    }
    return kept;
}

// WRITE = false: lane_keep[chunk] = rows that start in the chunk, nl[tile] / keep[tile] = line feeds / rows of the tile, g[0] |= 1 for
// a file that is not decided here, g[1] = min over the malformed lines of (start << 2 | reason).  WRITE = true: nl[] and keep[] hold
// their exclusive scans, the rows go to their places.
template <bool WRITE>
__global__ void __launch_bounds__(256) rows_lines_kernel(const uint8_t *__restrict__ t, int64_t n, int format,
                                                         uint8_t *__restrict__ lane_keep, uint64_t *__restrict__ nl,
                                                         uint64_t *__restrict__ keep, unsigned long long *__restrict__ g, rows_out out)
{
    __shared__ uint64_t lds[4];
    const int64_t chunk = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t c0 = chunk * RM_CHUNK;
    const bool aligned = ((uintptr_t)t & 15) == 0;
    uint64_t lo = 0, hi = 0;
    bool bad = false;
    if (c0 < n) rm_scan_chunk(t, c0, n, aligned, lo, hi, bad);
    const uint32_t my_nl = (uint32_t)(__builtin_popcountll(lo) + __builtin_popcountll(hi));
    uint64_t place = 0, line0 = 0;
    if (WRITE) {
        const uint32_t my_keep = c0 < n ? lane_keep[chunk] : 0u;
        const uint64_t ex = block_exclusive_scan(((uint64_t)my_nl << 32) | my_keep, nullptr, lds);
        place = keep[blockIdx.x] + (ex & 0xffffffffull);
        line0 = nl[blockIdx.x] + (ex >> 32);
    }
    uint64_t shortest = ROWS_NO_LINE;
    const uint32_t kept = c0 < n ? rows_chunk_lines<WRITE>(t, c0, n, format, lo, hi, bad, shortest, place, line0, out) : 0u;
    if (!WRITE) {
        if (c0 < n) lane_keep[chunk] = (uint8_t)kept;                        // (at most RM_CHUNK / ROWS_MIN_LINE + 1)
        if (bad) atomicOr(&g[0], 1ull);
        if (shortest != ROWS_NO_LINE) atomicMin(&g[1], (unsigned long long)shortest);
        uint64_t total;
        block_exclusive_scan(((uint64_t)my_nl << 32) | kept, &total, lds);
        if (threadIdx.x == 0) {
            nl[blockIdx.x] = total >> 32;
            keep[blockIdx.x] = total & 0xffffffffull;
        }
    }
}

// g[2] = the line (from 1) of the malformed line g[1] states: the line feeds in front of its tile (nl[], scanned) plus those of the
// tile in front of its first byte.  One workgroup.
__global__ void __launch_bounds__(256) rows_bad_line_kernel(const uint8_t *__restrict__ t, const uint64_t *__restrict__ nl,
                                                            unsigned long long *__restrict__ g)
{
    __shared__ uint64_t lds[4];
    const unsigned long long code = g[1];
    if (code == ROWS_NO_LINE) return;                                        // (uniform: every lane reads the same word)
    const int64_t pos = (int64_t)(code >> 2), tile = pos / RM_TILE;
    const int64_t c0 = tile * RM_TILE + (int64_t)threadIdx.x * RM_CHUNK;
    const int64_t c1 = c0 + RM_CHUNK < pos ? c0 + RM_CHUNK : pos;
    uint64_t feeds = 0;
    for (int64_t p = c0; p < c1; ++p) feeds += t[p] == '\n';
    uint64_t total;
    block_exclusive_scan(feeds, &total, lds);
    if (threadIdx.x == 0) g[2] = nl[tile] + total + 1;
}

static inline int64_t rows_bound(int64_t n) { return n / ROWS_MIN_LINE + 1; }

}   // namespace

DGRP_EXPORT int64_t dgrp_rows_parse_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    const int64_t tiles = rm_tiles_of(n), rows = rows_bound(n);
    const int64_t scanned = tiles > rows ? tiles : rows;
    return RM_HEAD + 2 * dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up(((scanned + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256) +
           dgrp_align_up(tiles * 256, 256) + dgrp_align_up((rows + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_rows_parse(const uint8_t *d_text, int64_t n, int format, int64_t *d_begin, int64_t *d_end, int64_t *d_number,
                                int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_file_pos, int32_t *d_file_len, int64_t *d_line,
                                int64_t *d_run_first, int64_t cap, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    const char *what = "dgrp_rows_parse";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_counts, "%s: NULL counts", what);
    for (int k = 0; k < 6; ++k) h_counts[k] = 0;
    DGRP_REQUIRE(n >= 0, "%s: negative size", what);
    DGRP_REQUIRE(d_text || n == 0, "%s: NULL text of %lld bytes", what, (long long)n);
    DGRP_REQUIRE(format == 0 || format == 1, "%s: format %d: 0 (table) or 1 (tsv)", what, format);
    DGRP_REQUIRE(cap >= 0, "%s: negative capacity", what);
    DGRP_REQUIRE(cap == 0 || (d_begin && d_end && d_number && d_name_pos && d_name_len && d_line && d_run_first), "%s: NULL output", what);
    DGRP_REQUIRE(cap == 0 || format == 0 || (d_file_pos && d_file_len), "%s: NULL output", what);
    if (n == 0) return DGRP_OK;
    const int64_t tiles = rm_tiles_of(n), bound = rows_bound(n);
    DGRP_REQUIRE(tiles < (1ll << 31), "%s: too many bytes", what);
    DGRP_REQUIRE(d_work && ((uintptr_t)d_work & 255) == 0, "%s: workspace NULL or not 256-byte aligned", what);
    if (work_bytes < dgrp_rows_parse_workspace_bytes(n)) {
        dgrp_set_error("%s: workspace too small", what);
        return DGRP_ENOMEM;
    }
    unsigned long long *g = (unsigned long long *)d_work;
    char *p = (char *)d_work + RM_HEAD;
    uint64_t *d_nl = (uint64_t *)p;
    p += dgrp_align_up((tiles + 1) * 8, 256);
    uint64_t *d_keep = (uint64_t *)p;
    p += dgrp_align_up((tiles + 1) * 8, 256);
    uint64_t *d_tiles = (uint64_t *)p;
    p += dgrp_align_up((((tiles > bound ? tiles : bound) + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256);
    uint8_t *d_lane = (uint8_t *)p;
    p += dgrp_align_up(tiles * 256, 256);
    uint64_t *d_run = (uint64_t *)p;
    const bool tsv = format == 1;
    const rows_out none = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    const rows_out out = { d_begin, d_end, d_number, d_name_pos, d_name_len, tsv ? d_file_pos : nullptr, tsv ? d_file_len : nullptr, d_line, cap };

    // count pass, the two scans, the line of the first malformed line, and the figures the host decides on: one synchronisation
    DGRP_HIP(hipMemsetAsync(g, 0, RM_HEAD, stream));
    DGRP_HIP(hipMemsetAsync(g + 1, 0xff, 8, stream));
    hipLaunchKernelGGL(rows_lines_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, format, d_lane, d_nl, d_keep, g, none);
    DGRP_LAUNCH_CHECK();
    int rc = device_exclusive_scan(d_nl, d_nl, tiles, d_tiles, d_nl + tiles, stream);
    if (rc != DGRP_OK) return rc;
    rc = device_exclusive_scan(d_keep, d_keep, tiles, d_tiles, d_keep + tiles, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(rows_bad_line_kernel, dim3(1), dim3(256), 0, stream, d_text, d_nl, g);
    DGRP_LAUNCH_CHECK();
    unsigned long long head[3] = { 0, 0, 0 }, feeds = 0, kept = 0;
    uint8_t last = 0;
    hipError_t e = hipMemcpyAsync(head, g, 24, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&feeds, d_nl + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&kept, d_keep + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last, d_text + n - 1, 1, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);                      // (also after a failed copy: the targets die on return)
    DGRP_HIP(e);
    DGRP_HIP(e2);
    h_counts[0] = (int64_t)feeds + (last != '\n' ? 1 : 0);
    h_counts[1] = (int64_t)kept;
    h_counts[3] = head[0] ? 1 : 0;
    if (head[0]) return DGRP_OK;                                             // not decided: the host parses this file
    if (head[1] != ROWS_NO_LINE) {                                           // malformed: the caller raises, no row is written
        h_counts[4] = (int64_t)head[2];
        h_counts[5] = (int64_t)(head[1] & 3ull);
        return DGRP_OK;
    }
    if (kept == 0) return DGRP_OK;
    if ((int64_t)kept > cap) {
        dgrp_set_error("%s: %lld rows for a capacity of %lld", what, (long long)kept, (long long)cap);
        return DGRP_ENOMEM;
    }
    const int64_t rows = (int64_t)kept;                                      // (<= bound: every row has ROWS_MIN_LINE bytes)
    hipLaunchKernelGGL(rows_lines_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, format, d_lane, d_nl, d_keep, g, out);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(rm_run_flag_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, d_text, (const int64_t *)d_name_pos,
                       (const int32_t *)d_name_len, (const int64_t *)out.file_pos, (const int32_t *)out.file_len, rows, d_run);
    DGRP_LAUNCH_CHECK();
    rc = device_exclusive_scan(d_run, d_run, rows, d_tiles, d_run + rows, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(rm_run_first_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, d_run, rows, d_run_first);
    DGRP_LAUNCH_CHECK();
    unsigned long long runs = 0;
    e = hipMemcpyAsync(&runs, d_run + rows, 8, hipMemcpyDeviceToHost, stream);
    const hipError_t e3 = hipStreamSynchronize(stream);
    DGRP_HIP(e);
    DGRP_HIP(e3);
    h_counts[2] = (int64_t)runs;
    return DGRP_OK;
}
