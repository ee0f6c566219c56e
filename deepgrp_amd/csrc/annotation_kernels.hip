// RepeatMasker listings (`genome.fa.out`, UCSC `rmsk.txt`) -> the numbered rows of `parse_rm`, on the device: the text is in HBM
// (uploaded, or inflated there), and what leaves it are row arrays in file order and the first row of every run of one contig name.
// The grammar is the token statement of the two regular expressions of deepgrp_amd/_scripts/parse_rm.py; a file with a
// byte or a number that statement does not cover raises a flag and is parsed by that script's own code on the host.
//
// Work split: a workgroup takes a tile of RM_TILE bytes, a lane a chunk of RM_CHUNK = 128 consecutive bytes (one cache line) of it and
// every line that STARTS in its chunk -- about one for a `.out` listing.  The lane walks its lines byte by byte in global memory: the
// bytes were just read by the same workgroup, and a line of any length needs no staging limit.  Bytes and integers only, no atomics
// but the OR of the flag; a count pass and a write pass around one scan give every row its place, so the same call gives the same bytes.
// dgrp_rm_parse_all is one more mode of the same two passes: every line that matches a pattern is a row, numbered or not, and the
// span (or the two spans) of its family token travels with it.
#include "text_lines.h"                  // tiles, chunks, the chunk scan and the run starts: shared with dgrp_rows_parse

namespace {

#define RM_MIN_LINE 22                   // shortest line that can match: 11 tokens of one byte, 10 separators, the line end
#define RM_MAX_DIGITS 18                 // a coordinate of more digits is left to the host

struct rm_tables {
    const uint8_t *names;                // the numbered names back to back
    const int64_t *name_off;             // [nnames + 1]
    int nnames;
    const uint8_t *pent;                 // [1024] by 2-bit packed 5-mer: 0 neither, 1 exact, 2 one substitution away
    int unit_number;
};

struct rm_row {
    int64_t begin, end, name_pos;
    int32_t number, name_len;
    int64_t div_b, div_e;                // the divergence token: `.out` token 1 (percent), `rmsk` field 2 (tenths of a percent)
    bool div_rmsk;
    int64_t fam_pos, fam2_pos;           // the family token: `.out` token 10; `rmsk` field 11 and, where it differs, field 12 behind it
    int32_t fam_len, fam2_len;           // (fam2_len = 0: the token is the first span alone)
};

// a token, or two of them read as `A/B`
struct rm_str {
    int64_t ab, ae, bb, be;
    bool joined;
    __host__ __device__ int64_t len() const { return (ae - ab) + (joined ? 1 + (be - bb) : 0); }
    __host__ __device__ uint8_t at(const uint8_t *__restrict__ t, int64_t j) const
    {
        const int64_t la = ae - ab;
        return j < la ? t[ab + j] : (j == la ? (uint8_t)'/' : t[bb + (j - la - 1)]);
    }
};

__host__ __device__ bool rm_equals(const uint8_t *__restrict__ t, const rm_str &s, const uint8_t *__restrict__ word, int64_t wlen)
{
    if (s.len() != wlen) return false;
    for (int64_t j = 0; j < wlen; ++j)
        if (s.at(t, j) != word[j]) return false;
    return true;
}

__host__ __device__ int rm_number_of(const uint8_t *__restrict__ t, const rm_str &s, const rm_tables &T)
{
    for (int i = 0; i < T.nnames; ++i)
        if (rm_equals(t, s, T.names + T.name_off[i], T.name_off[i + 1] - T.name_off[i])) return i + 1;
    return 0;
}

// `(` [ACGT]+ `)n` at the head of the token, the unit a multiple of five long, every 5-mer exact or one off, one exact at least
__host__ __device__ bool rm_unit_rule(const uint8_t *__restrict__ t, int64_t rb, int64_t re, const uint8_t *__restrict__ pent)
{
    if (re - rb < 4 || t[rb] != '(') return false;
    int64_t q = rb + 1;
    uint32_t code = 0;
    int in5 = 0;
    bool all = true, exact = false;
    for (; q < re; ++q) {
        const uint8_t c = t[q];
        uint32_t b;
        if (c == 'A') b = 0; else if (c == 'C') b = 1; else if (c == 'G') b = 2; else if (c == 'T') b = 3; else break;
        code = (code << 2) | b;
        if (++in5 == 5) {
            const uint8_t v = pent[code & 1023u];
            all = all && v != 0;
            exact = exact || v == 1;
            in5 = 0;
            code = 0;
        }
    }
    if (q == rb + 1 || q + 1 >= re || t[q] != ')' || t[q + 1] != 'n') return false;
    return in5 == 0 && all && exact;
}

// The line that starts at s: true and `row` when it is a numbered repeat -- with `all`, when it matches a pattern at all (its number
// is then 0 where the rule finds none).  `big`: a coordinate of more than RM_MAX_DIGITS digits.
__host__ __device__ bool rm_parse_line(const uint8_t *__restrict__ t, int64_t s, int64_t n, const rm_tables &T, rm_row &row, bool &big,
                                       bool all = false)
{
    const uint8_t simple[13] = { 'S', 'i', 'm', 'p', 'l', 'e', '_', 'r', 'e', 'p', 'e', 'a', 't' };
    const uint8_t satellite[9] = { 'S', 'a', 't', 'e', 'l', 'l', 'i', 't', 'e' };
    int64_t cb = 0, ce = 0, rb = 0, re = 0, v5 = 0, v6 = 0, db = 0, de = 0;
    bool rmsk = false;
    rm_str fam = { 0, 0, 0, 0, false };
    bool ok = true;
    // ---- `.out`: tokens between runs of blanks
    {
        int64_t p = s;
        for (int k = 0; k < 11 && ok; ++k) {
            while (p < n && rm_blank(t[p])) ++p;
            if (p >= n || rm_eol(t[p])) { ok = false; break; }
            const int64_t b = p;
            const uint8_t first = t[p];
            bool dig = true;
            int nd = 0;
            int64_t val = 0;
            for (; p < n; ++p) {
                const uint8_t c = t[p];
                if (rm_blank(c) || rm_eol(c)) break;
                if (c >= '0' && c <= '9') {
                    if (nd < RM_MAX_DIGITS) val = val * 10 + (c - '0');
                    ++nd;
                } else {
                    dig = false;
                }
            }
            if (k == 0) ok = dig;
            else if (k == 1) { db = b; de = p; }
            else if (k == 4) { cb = b; ce = p; }
            else if (k == 5 || k == 6) {
                ok = dig;
                if (dig && nd > RM_MAX_DIGITS) big = true;
                if (k == 5) v5 = val - 1; else v6 = val;
            }
            else if (k == 8) ok = p - b == 1 && (first == '+' || first == 'C');
            else if (k == 9) { rb = b; re = p; }
            else if (k == 10) { fam.ab = b; fam.ae = p; }
        }
    }
    if (!ok) {
        // ---- `rmsk`: fields between single tabs from column 0
        ok = true;
        int64_t p = s;
        for (int k = 0; k < 13 && ok; ++k) {
            const int64_t b = p;
            const uint8_t first = p < n ? t[p] : (uint8_t)'\n';
            bool dig = true, space = false;
            int nd = 0;
            int64_t val = 0;
            for (; p < n; ++p) {
                const uint8_t c = t[p];
                if (c == '\t' || rm_eol(c) || (k == 12 && c == ' ')) break;
                if (c >= '0' && c <= '9') {
                    if (nd < RM_MAX_DIGITS) val = val * 10 + (c - '0');
                    ++nd;
                } else {
                    dig = false;
                    space = space || c == ' ';
                }
            }
            if (p == b) { ok = false; break; }
            if (k <= 4) {
                ok = dig;
                if (k == 2) { db = b; de = p; }
            }
            else if (k == 6 || k == 7) {
                ok = dig;
                if (dig && nd > RM_MAX_DIGITS) big = true;
                if (k == 6) v5 = val; else v6 = val;
            }
            else if (k == 9) ok = p - b == 1 && (first == '+' || first == '-');
            else {
                ok = !space;
                if (k == 5) { cb = b; ce = p; }
                else if (k == 10) { rb = b; re = p; }
                else if (k == 11) { fam.ab = b; fam.ae = p; }
                else if (k == 12) { fam.bb = b; fam.be = p; }
            }
            if (ok && k < 12) {
                if (p >= n || t[p] != '\t') ok = false;
                ++p;
            }
        }
        if (ok) {
            // family = class when both agree, else class/family -- compared in place
            bool same = fam.ae - fam.ab == fam.be - fam.bb;
            for (int64_t j = 0; same && j < fam.ae - fam.ab; ++j) same = t[fam.ab + j] == t[fam.bb + j];
            fam.joined = !same;
            rmsk = true;
        }
    }
    if (!ok) return false;
    const rm_str rep = { rb, re, 0, 0, false };
    int number = rm_number_of(t, fam, T);
    if (number == 0) number = rm_number_of(t, rep, T);
    if (number == 0 && (rm_equals(t, fam, simple, 13) || rm_equals(t, fam, satellite, 9)) && rm_unit_rule(t, rb, re, T.pent))
        number = T.unit_number;
    if (number <= 0 && !all) return false;
    if (number < 0) number = 0;
    if (ce - cb > 0x7fffffffll) big = true;                                  // (a name the int32 length cannot state)
    if (all && (fam.ae - fam.ab > 0x7fffffffll || fam.be - fam.bb > 0x7fffffffll)) big = true;
    row.fam_pos = fam.ab;
    row.fam_len = (int32_t)(fam.ae - fam.ab);
    row.fam2_pos = fam.joined ? fam.bb : fam.ab;
    row.fam2_len = fam.joined ? (int32_t)(fam.be - fam.bb) : 0;
    row.begin = v5;
    row.end = v6;
    row.name_pos = cb;
    row.name_len = (int32_t)(ce - cb);
    row.number = number;
    row.div_b = db;
    row.div_e = de;
    row.div_rmsk = rmsk;
    return true;
}

// The divergence of a kept row in tenths of a percent, -1 where the token does not state one (include/deepgrp_hip.h).  `rmsk`: the
// field is digits already (the pattern asked for them) and already in tenths.  `.out`: D, `D.` or `D.d...` with 1..6 digits D and
// digits only behind the point -> 10 D + the first of them; further digits are dropped.
__host__ __device__ int32_t rm_millidiv(const uint8_t *__restrict__ t, const rm_row &row)
{
    int64_t p = row.div_b;
    const int64_t e = row.div_e;
    int32_t val = 0;
    int nd = 0;
    for (; p < e && t[p] >= '0' && t[p] <= '9'; ++p) {
        if (nd < 7) val = val * 10 + (t[p] - '0');
        ++nd;
    }
    if (row.div_rmsk) return p == e && nd >= 1 && nd <= 7 ? val : -1;
    if (nd < 1 || nd > 6) return -1;
    if (p == e) return 10 * val;
    if (t[p] != '.') return -1;
    ++p;
    int32_t first = 0;
    for (int64_t q = p; q < e; ++q) {
        if (t[q] < '0' || t[q] > '9') return -1;
        if (q == p) first = t[q] - '0';
    }
    return 10 * val + first;
}

struct rm_out {
    int64_t *begin, *end;
    int32_t *number;
    int64_t *name_pos;
    int32_t *name_len;
    int64_t *line;
    int32_t *millidiv;                   // NULL: not asked for (dgrp_rm_parse)
    int64_t *fam_pos;                    // NULL: not asked for; else every matching line is a row (dgrp_rm_parse_all)
    int32_t *fam_len;
    int64_t *fam2_pos;
    int32_t *fam2_len;
    int64_t cap;
};

// The lines that start in the chunk [c0, c0 + RM_CHUNK) with the line feeds lo / hi: -> how many are numbered repeats.  WRITE: they are
// rows place, place + 1, ... and line0 line feeds lie in front of the chunk.
template <bool WRITE>
__host__ __device__ uint32_t rm_chunk_lines(const uint8_t *__restrict__ t, int64_t c0, int64_t n, const rm_tables &T, uint64_t lo,
                                            uint64_t hi, bool &bad, uint64_t place, uint64_t line0, const rm_out &out, bool all)
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
        rm_row row;
        if (rm_parse_line(t, s, n, T, row, bad, all)) {
            if (WRITE) {
                const int64_t i = (int64_t)(place + kept);
                if (i < out.cap) {
                    out.begin[i] = row.begin;
                    out.end[i] = row.end;
                    out.number[i] = row.number;
                    out.name_pos[i] = row.name_pos;
                    out.name_len[i] = row.name_len;
                    out.line[i] = (int64_t)(line0 + seen) + 1;
                    if (out.millidiv) out.millidiv[i] = rm_millidiv(t, row);
                    if (out.fam_pos) {
                        out.fam_pos[i] = row.fam_pos;
                        out.fam_len[i] = row.fam_len;
                        out.fam2_pos[i] = row.fam2_pos;
                        out.fam2_len[i] = row.fam2_len;
                    }
                }
            }
            ++kept;
        }
        s = -1;
    }
    return kept;
}

// WRITE = false: lane_keep[chunk] = numbered lines that start in the chunk, nl[tile] / keep[tile] = line feeds / numbered lines of the
// tile, g[0] |= 1 for a file that is not plain.  WRITE = true: nl[] and keep[] hold their exclusive scans, the rows go to their places.
template <bool WRITE>
__global__ void __launch_bounds__(256) rm_lines_kernel(const uint8_t *__restrict__ t, int64_t n, rm_tables T,
                                                       uint8_t *__restrict__ lane_keep, uint64_t *__restrict__ nl,
                                                       uint64_t *__restrict__ keep, unsigned long long *__restrict__ g,
                                                       int64_t *__restrict__ o_begin, int64_t *__restrict__ o_end,
                                                       int32_t *__restrict__ o_number, int64_t *__restrict__ o_name_pos,
                                                       int32_t *__restrict__ o_name_len, int64_t *__restrict__ o_line,
                                                       int32_t *__restrict__ o_millidiv, int64_t *__restrict__ o_fam_pos,
                                                       int32_t *__restrict__ o_fam_len, int64_t *__restrict__ o_fam2_pos,
                                                       int32_t *__restrict__ o_fam2_len, bool all, int64_t cap)
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
    const rm_out out = { o_begin, o_end, o_number, o_name_pos, o_name_len, o_line, o_millidiv, o_fam_pos, o_fam_len, o_fam2_pos, o_fam2_len, cap };
    const uint32_t kept = c0 < n ? rm_chunk_lines<WRITE>(t, c0, n, T, lo, hi, bad, place, line0, out, all) : 0u;
    if (!WRITE) {
        if (c0 < n) lane_keep[chunk] = (uint8_t)kept;                        // (at most RM_CHUNK / RM_MIN_LINE + 1)
        if (bad) atomicOr(&g[0], 1ull);
        uint64_t total;
        block_exclusive_scan(((uint64_t)my_nl << 32) | kept, &total, lds);
        if (threadIdx.x == 0) {
            nl[blockIdx.x] = total >> 32;
            keep[blockIdx.x] = total & 0xffffffffull;
        }
    }
}

static inline int64_t rm_rows_bound(int64_t n) { return n / RM_MIN_LINE + 1; }

}   // namespace

DGRP_EXPORT int64_t dgrp_rm_parse_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    const int64_t tiles = rm_tiles_of(n), rows = rm_rows_bound(n);
    const int64_t scanned = tiles > rows ? tiles : rows;
    return RM_HEAD + 2 * dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up(((scanned + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256) +
           dgrp_align_up(tiles * 256, 256) + dgrp_align_up((rows + 1) * 8, 256);
}

namespace {

struct rm_fam_out {
    int64_t *pos;
    int32_t *len;
    int64_t *pos2;
    int32_t *len2;
};

// the three entries: d_millidiv NULL (dgrp_rm_parse) writes no divergence; fam non-NULL (dgrp_rm_parse_all) keeps every matching line
int rm_parse_run(const char *what, bool fields, const rm_fam_out *fam, const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off,
                 int nnames, const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                 int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int32_t *d_millidiv, int64_t *d_run_first, int64_t cap,
                 int64_t *h_counts, void *d_work, int64_t work_bytes, hipStream_t stream)
{
    DGRP_REQUIRE(h_counts, "%s: NULL counts", what);
    h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
    DGRP_REQUIRE(n >= 0, "%s: negative size", what);
    DGRP_REQUIRE(d_text || n == 0, "%s: NULL text of %lld bytes", what, (long long)n);
    DGRP_REQUIRE(d_names && d_name_off && d_pentamers, "%s: NULL table", what);
    DGRP_REQUIRE(nnames >= 1 && nnames <= 127 && unit_number >= 1 && unit_number <= 127, "%s: %d names, unit number %d: 1..127 each",
                 what, nnames, unit_number);
    DGRP_REQUIRE(cap >= 0, "%s: negative capacity", what);
    DGRP_REQUIRE(cap == 0 || (d_begin && d_end && d_number && d_name_pos && d_name_len && d_line && d_run_first), "%s: NULL output", what);
    DGRP_REQUIRE(cap == 0 || !fields || d_millidiv, "%s: NULL output", what);
    DGRP_REQUIRE(cap == 0 || !fam || (fam->pos && fam->len && fam->pos2 && fam->len2), "%s: NULL output", what);
    const bool all = fam != nullptr;
    const rm_fam_out fo = all ? *fam : rm_fam_out{ nullptr, nullptr, nullptr, nullptr };
    if (n == 0) return DGRP_OK;
    const int64_t tiles = rm_tiles_of(n), bound = rm_rows_bound(n);
    DGRP_REQUIRE(tiles < (1ll << 31), "%s: too many bytes", what);
    DGRP_REQUIRE(d_work && ((uintptr_t)d_work & 255) == 0, "%s: workspace NULL or not 256-byte aligned", what);
    if (work_bytes < dgrp_rm_parse_workspace_bytes(n)) {
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
    const rm_tables T = { d_names, d_name_off, nnames, d_pentamers, unit_number };

    // count pass, the two scans, and the figures the host decides on: one synchronisation
    DGRP_HIP(hipMemsetAsync(g, 0, RM_HEAD, stream));
    hipLaunchKernelGGL(rm_lines_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, T, d_lane, d_nl, d_keep, g,
                       (int64_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr,
                       (int64_t *)nullptr, (int32_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr, (int64_t *)nullptr,
                       (int32_t *)nullptr, all, (int64_t)0);
    DGRP_LAUNCH_CHECK();
    int rc = device_exclusive_scan(d_nl, d_nl, tiles, d_tiles, d_nl + tiles, stream);
    if (rc != DGRP_OK) return rc;
    rc = device_exclusive_scan(d_keep, d_keep, tiles, d_tiles, d_keep + tiles, stream);
    if (rc != DGRP_OK) return rc;
    unsigned long long flag = 0, feeds = 0, kept = 0;
    uint8_t last = 0;
    hipError_t e = hipMemcpyAsync(&flag, g, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&feeds, d_nl + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&kept, d_keep + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last, d_text + n - 1, 1, hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream);                      // (also after a failed copy: the targets die on return)
    DGRP_HIP(e);
    DGRP_HIP(e2);
    h_counts[0] = (int64_t)feeds + (last != '\n' ? 1 : 0);
    h_counts[1] = (int64_t)kept;
    h_counts[3] = flag ? 1 : 0;
    if (flag || kept == 0) return DGRP_OK;                                   // not plain: the host decides this file
    if ((int64_t)kept > cap) {
        dgrp_set_error("%s: %lld rows for a capacity of %lld", what, (long long)kept, (long long)cap);
        return DGRP_ENOMEM;
    }
    const int64_t rows = (int64_t)kept;                                      // (<= bound: every numbered line has RM_MIN_LINE bytes)
    hipLaunchKernelGGL(rm_lines_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, stream, d_text, n, T, d_lane, d_nl, d_keep, g, d_begin,
                       d_end, d_number, d_name_pos, d_name_len, d_line, fields ? d_millidiv : (int32_t *)nullptr, fo.pos, fo.len, fo.pos2,
                       fo.len2, all, cap);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(rm_run_flag_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, d_text, d_name_pos, d_name_len,
                       (const int64_t *)nullptr, (const int32_t *)nullptr, rows, d_run);
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

}   // namespace

DGRP_EXPORT int dgrp_rm_parse(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                              const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                              int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int64_t cap,
                              int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    return rm_parse_run("dgrp_rm_parse", false, nullptr, d_text, n, d_names, d_name_off, nnames, d_pentamers, unit_number, d_begin, d_end, d_number,
                        d_name_pos, d_name_len, d_line, nullptr, d_run_first, cap, h_counts, d_work, work_bytes, (hipStream_t)stream_);
}

DGRP_EXPORT int dgrp_rm_parse_fields(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                                     const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                                     int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int32_t *d_millidiv,
                                     int64_t cap, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    return rm_parse_run("dgrp_rm_parse_fields", true, nullptr, d_text, n, d_names, d_name_off, nnames, d_pentamers, unit_number, d_begin, d_end,
                        d_number, d_name_pos, d_name_len, d_line, d_millidiv, d_run_first, cap, h_counts, d_work, work_bytes,
                        (hipStream_t)stream_);
}

DGRP_EXPORT int64_t dgrp_rm_parse_all_workspace_bytes(int64_t n) { return dgrp_rm_parse_workspace_bytes(n); }

DGRP_EXPORT int dgrp_rm_parse_all(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                                  const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                                  int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int32_t *d_millidiv,
                                  int64_t *d_fam_pos, int32_t *d_fam_len, int64_t *d_fam2_pos, int32_t *d_fam2_len, int64_t cap,
                                  int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream_)
{
    const rm_fam_out fam = { d_fam_pos, d_fam_len, d_fam2_pos, d_fam2_len };
    return rm_parse_run("dgrp_rm_parse_all", true, &fam, d_text, n, d_names, d_name_off, nnames, d_pentamers, unit_number, d_begin, d_end,
                        d_number, d_name_pos, d_name_len, d_line, d_millidiv, d_run_first, cap, h_counts, d_work, work_bytes,
                        (hipStream_t)stream_);
}
