// GFF3 as text -> arrays, on the device: the feature lines of a GFF3 file (what `predict --bed_gff3` writes, and what repeat finders
// and genome portals ship) as the rows dgrp_rows_parse returns for a table -- begin, end, number, the seqid as a span of the text, the
// line, and the first row of every run of one seqid.  The number of a row is looked up by NAME: its label string (the type column,
// or the value of one attribute key, %XX decoded during the comparison) against a table of alternatives.  The grammar is stated in
// include/deepgrp_hip.h (dgrp_gff_parse) and, as Python, in deepgrp_amd/gffin.py; the line function is gff_line.h.
//
// Work split: that of dgrp_rows_parse (text_lines.h) -- a workgroup takes a tile of RM_TILE bytes, a lane a chunk of 128 consecutive
// bytes and every line that STARTS in its chunk, walked byte by byte in global memory; a count pass and a write pass around the
// scans.  One step is new: the features end at E, the first line that is `##FASTA` or opens with '>', a property of the file.  A
// kernel in front takes the minimum over such line starts into the workspace head; the passes READ it there (kernels of one stream
// are ordered: no synchronisation is needed for it) and walk the text as if it had E bytes -- E is a line start, so that text ends
// in a line feed and every rule of the siblings' walk holds.  The host reads E with the counts, at the synchronisation it has anyway.
// Bytes and integers only; the only atomics are the OR of the flag and the two minima, so the same call gives the same bytes.
#include "text_lines.h"
#include "gff_line.h"

namespace {

#define GFF_NO_LINE (~0ull)              // g[1]: no malformed line yet; g[3]: no end of features yet

// The per-chunk row count is a uint8: at most RM_CHUNK / GFF_MIN_LINE + 1 lines of a chunk can be rows.
static_assert(RM_CHUNK / GFF_MIN_LINE + 1 <= 255, "rows of a chunk fit a byte");

struct gff_out {
    int64_t *begin, *end, *number, *name_pos;
    int32_t *name_len;
    int64_t *line;
    int64_t cap;
};

// g[3] = min over the line starts s of the text with gff_ends_features(s): a lane looks at the line starts of its chunk
__global__ void __launch_bounds__(256) gff_end_kernel(const uint8_t *__restrict__ t, int64_t n, unsigned long long *__restrict__ g)
{
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * RM_CHUNK;
    if (c0 >= n) return;
    const int64_t c1 = c0 + RM_CHUNK < n ? c0 + RM_CHUNK : n;
    uint64_t lo, hi;
    bool bad = false;                                                        // (not this kernel's to report)
    rm_scan_chunk(t, c0, n, ((uintptr_t)t & 15) == 0, lo, hi, bad);
    int64_t s = (c0 == 0 || t[c0 - 1] == '\n') ? c0 : -1;
    for (;;) {
        if (s < 0) {
            int k;
            if (lo) { k = __builtin_ctzll(lo); lo &= lo - 1; }
            else if (hi) { k = 64 + __builtin_ctzll(hi); hi &= hi - 1; }
            else break;
            s = c0 + k + 1;
            if (s >= c1) break;                                              // the next chunk's line (or the end of the text)
        }
        if (gff_ends_features(t, s, n)) {
            atomicMin(&g[3], (unsigned long long)s);
            break;                                                           // (a later line of the chunk cannot be smaller)
        }
        s = -1;
    }
}

// The lines that start in the chunk [c0, c0 + RM_CHUNK) of a text of n bytes with the line feeds lo / hi: -> how many are rows;
// `shortest`: the smallest (start << 2 | 3) of its malformed lines.  WRITE: they are rows place, place + 1, ... and line0 line feeds
// lie in front of the chunk.
template <bool WRITE>
__device__ uint32_t gff_chunk_lines(const uint8_t *__restrict__ t, int64_t c0, int64_t n, const gff_table &tab, uint64_t lo, uint64_t hi,
                                    bool &bad, uint64_t &shortest, uint64_t place, uint64_t line0, const gff_out &out)
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
            if (s >= c1) break;
        }
        gff_row row;
        const int what = gff_line(t, s, n, tab, WRITE, row, bad);
        if (what == GFF_SHORT) {
            const uint64_t code = ((uint64_t)s << 2) | 3ull;
            if (code < shortest) shortest = code;
        } else if (what == GFF_ROW) {
            if (WRITE) {
                const int64_t i = (int64_t)(place + kept);
                if (i < out.cap) {
                    out.begin[i] = row.begin;
                    out.end[i] = row.end;
                    out.number[i] = row.number;
                    out.name_pos[i] = row.name_pos;
                    out.name_len[i] = row.name_len;
                    out.line[i] = (int64_t)(line0 + seen) + 1;
                }
            }
            ++kept;
        }
        s = -1;
    }
    return kept;
}

// rows_lines_kernel of dgrp_rows_parse on the text in front of E = min(g[3], n_all), read from the workspace head.  WRITE = false:
// lane_keep[chunk] = rows that start in the chunk, nl[tile] / keep[tile] = line feeds / rows of the tile, g[0] |= 1 for a file that
// is not decided here, g[1] = min over the malformed lines of (start << 2 | 3).  WRITE = true: nl[] and keep[] hold their exclusive
// scans, the rows go to their places.
template <bool WRITE>
__global__ void __launch_bounds__(256) gff_lines_kernel(const uint8_t *__restrict__ t, int64_t n_all, gff_table tab,
                                                        uint8_t *__restrict__ lane_keep, uint64_t *__restrict__ nl,
                                                        uint64_t *__restrict__ keep, unsigned long long *__restrict__ g, gff_out out)
{
    __shared__ uint64_t lds[4];
    const unsigned long long found = g[3];                                   // (written by the kernel in front, read-only from here on)
    const int64_t n = found < (unsigned long long)n_all ? (int64_t)found : n_all;
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
    uint64_t shortest = GFF_NO_LINE;
    const uint32_t kept = c0 < n ? gff_chunk_lines<WRITE>(t, c0, n, tab, lo, hi, bad, shortest, place, line0, out) : 0u;
    if (!WRITE) {
        if (c0 < n) lane_keep[chunk] = (uint8_t)kept;                        // (at most RM_CHUNK / GFF_MIN_LINE + 1)
        if (bad) atomicOr(&g[0], 1ull);
        if (shortest != GFF_NO_LINE) atomicMin(&g[1], (unsigned long long)shortest);
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
__global__ void __launch_bounds__(256) gff_bad_line_kernel(const uint8_t *__restrict__ t, const uint64_t *__restrict__ nl,
                                                           unsigned long long *__restrict__ g)
{
    __shared__ uint64_t lds[4];
    const unsigned long long code = g[1];
    if (code == GFF_NO_LINE) return;                                         // (uniform: every lane reads the same word)
    const int64_t pos = (int64_t)(code >> 2), tile = pos / RM_TILE;
    const int64_t c0 = tile * RM_TILE + (int64_t)threadIdx.x * RM_CHUNK;
    const int64_t c1 = c0 + RM_CHUNK < pos ? c0 + RM_CHUNK : pos;
    uint64_t feeds = 0;
    for (int64_t p = c0; p < c1; ++p) feeds += t[p] == '\n';
    uint64_t total;
    block_exclusive_scan(feeds, &total, lds);
    if (threadIdx.x == 0) g[2] = nl[tile] + total + 1;
}

static inline int64_t gff_bound(int64_t n) { return n / GFF_MIN_LINE + 1; }

}   // namespace

DGRP_EXPORT int64_t dgrp_gff_parse_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    const int64_t tiles = rm_tiles_of(n), rows = gff_bound(n);
    const int64_t scanned = tiles > rows ? tiles : rows;
    return RM_HEAD + 2 * dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up(((scanned + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256) +
           dgrp_align_up(tiles * 256, 256) + dgrp_align_up((rows + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_gff_parse(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off,
                               const int32_t *d_name_number, int nnames, const uint8_t *d_key, int key_len, int64_t *d_begin,
                               int64_t *d_end, int64_t *d_number, int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line,
                               int64_t *d_run_first, int64_t cap, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    const char *what = "dgrp_gff_parse";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_counts, "%s: NULL counts", what);
    for (int k = 0; k < 7; ++k) h_counts[k] = 0;
    DGRP_REQUIRE(n >= 0, "%s: negative size", what);
    DGRP_REQUIRE(d_text || n == 0, "%s: NULL text of %lld bytes", what, (long long)n);
    DGRP_REQUIRE(nnames >= 0 && nnames <= GFF_MAX_NAMES, "%s: %d alternatives: 0..%d", what, nnames, GFF_MAX_NAMES);
    DGRP_REQUIRE(nnames == 0 || (d_names && d_name_off && d_name_number), "%s: NULL names table of %d alternatives", what, nnames);
    DGRP_REQUIRE(key_len >= 0 && key_len <= GFF_MAX_KEY, "%s: a key of %d bytes: 0..%d", what, key_len, GFF_MAX_KEY);
    DGRP_REQUIRE(d_key || key_len == 0, "%s: NULL key of %d bytes", what, key_len);
    DGRP_REQUIRE(cap >= 0, "%s: negative capacity", what);
    DGRP_REQUIRE(cap == 0 || (d_begin && d_end && d_number && d_name_pos && d_name_len && d_line && d_run_first), "%s: NULL output", what);
    if (n == 0) return DGRP_OK;
    const int64_t tiles = rm_tiles_of(n), bound = gff_bound(n);
    DGRP_REQUIRE(tiles < (1ll << 31), "%s: too many bytes", what);
    DGRP_REQUIRE(d_work && ((uintptr_t)d_work & 255) == 0, "%s: workspace NULL or not 256-byte aligned", what);
    if (work_bytes < dgrp_gff_parse_workspace_bytes(n)) {
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
    const gff_table tab = { d_names, d_name_off, d_name_number, nnames, d_key, key_len };
    const gff_out none = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    const gff_out out = { d_begin, d_end, d_number, d_name_pos, d_name_len, d_line, cap };

    // the end of the features, the count pass in front of it, the two scans, the line of the first malformed line, and the figures
    // the host decides on: one synchronisation
    DGRP_HIP(hipMemsetAsync(g, 0, RM_HEAD, stream));
    DGRP_HIP(hipMemsetAsync(g + 1, 0xff, 8, stream));
    DGRP_HIP(hipMemsetAsync(g + 3, 0xff, 8, stream));
    hipLaunchKernelGGL(gff_end_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, g);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(gff_lines_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, tab, d_lane, d_nl, d_keep, g, none);
    DGRP_LAUNCH_CHECK();
    int rc = device_exclusive_scan(d_nl, d_nl, tiles, d_tiles, d_nl + tiles, stream);
    if (rc != DGRP_OK) return rc;
    rc = device_exclusive_scan(d_keep, d_keep, tiles, d_tiles, d_keep + tiles, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(gff_bad_line_kernel, dim3(1), dim3(256), 0, stream, d_text, d_nl, g);
    DGRP_LAUNCH_CHECK();
    unsigned long long head[4] = { 0, 0, 0, 0 }, feeds = 0, kept = 0;
    uint8_t last = 0;
    hipError_t e = hipMemcpyAsync(head, g, 32, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&feeds, d_nl + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&kept, d_keep + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last, d_text + n - 1, 1, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);                      // (also after a failed copy: the targets die on return)
    DGRP_HIP(e);
    DGRP_HIP(e2);
    const int64_t end_at = head[3] < (unsigned long long)n ? (int64_t)head[3] : n;
    h_counts[0] = (int64_t)feeds + (end_at == n && last != '\n' ? 1 : 0);    // (E < n: the byte in front of E is a line feed)
    h_counts[1] = (int64_t)kept;
    h_counts[3] = head[0] ? 1 : 0;
    h_counts[6] = end_at;
    if (head[0]) return DGRP_OK;                                             // not decided: the host parses this file
    if (head[1] != GFF_NO_LINE) {                                            // malformed: the caller raises, no row is written
        h_counts[4] = (int64_t)head[2];
        h_counts[5] = (int64_t)(head[1] & 3ull);
        return DGRP_OK;
    }
    if (kept == 0) return DGRP_OK;
    if ((int64_t)kept > cap) {
        dgrp_set_error("%s: %lld rows for a capacity of %lld", what, (long long)kept, (long long)cap);
        return DGRP_ENOMEM;
    }
    const int64_t rows = (int64_t)kept;                                      // (<= bound: every row has GFF_MIN_LINE bytes)
    hipLaunchKernelGGL(gff_lines_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, tab, d_lane, d_nl, d_keep, g, out);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(rm_run_flag_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, d_text, (const int64_t *)d_name_pos,
                       (const int32_t *)d_name_len, (const int64_t *)nullptr, (const int32_t *)nullptr, rows, d_run);
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
