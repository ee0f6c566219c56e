// FASTA of the predicted repeats (predict --seq_dir): the sequence bytes under the TSV rows of plain record bodies, gathered into one
// compact text -- per kept row a header line and the bases of [A, B), `width` per line.  Stage 1 is mask_kernels.hip's count pass
// (sequence bytes per body tile, scanned) plus the count in front of every 16-byte word of a tile; the rows are checked and sized
// by one lane each, the sizes scanned; the text is then written by OUTPUT: one workgroup per EXTRACT_TILE bytes of text, 16 bytes
// per lane, every lane finding its row (binary search over the scanned sizes) and its first source byte (binary search over the
// record's tile prefix, then over the words of the tile) on its own.  Bytes and integers only.  See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "body_tiles.h"
#include "scan.h"
#include <vector>

namespace {

#define EXTRACT_TILE 4096         // bytes of output text per workgroup: 256 lanes x 16
#define BODY_WORDS (BODY_TILE / 16)

// stage 1: sequence bytes per tile and, per 16-byte word of the tile, the sequence bytes of the tile in front of it
__global__ void __launch_bounds__(256) extract_count_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ tile0,
                                                            const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                            int64_t nrec, uint64_t *__restrict__ tilecnt, uint16_t *__restrict__ wordpre)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_rec;
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) s_rec = dgrp_record_of(tile0, nrec, t);
    __syncthreads();
    const int64_t r = s_rec;
    const body_span s = body_lane_span(off[r], len[r], t - tile0[r]);
    alignas(16) uint8_t b[16];
    body_load(raw, s, b);
    uint64_t c = 0;
    for (int j = 0; j < 16; ++j) c += body_lineend(b[j]) ? 0 : 1;
    uint64_t tot;
    const uint64_t ex = block_exclusive_scan(c, &tot, lds);
    wordpre[t * BODY_WORDS + threadIdx.x] = (uint16_t)ex;
    if (threadIdx.x == 0) tilecnt[t] = tot;
}

// (no division: a lane states five of these per row, and a 64-bit division is a long routine)
__device__ __forceinline__ int dec_digits(int64_t v)
{
    int d = 1;
    uint64_t p = 10;
#pragma unroll 1
    for (int k = 1; k < 19 && (uint64_t)v >= p; ++k, p *= 10) ++d;
    return d;
}

// the j-th of the d decimal digits of v: one division by a power of ten, in 32 bits where v has them
__device__ __forceinline__ uint8_t dec_digit(int64_t v, int d, int j)
{
    uint64_t p = 1;
#pragma unroll 1
    for (int k = d - 1 - j; k > 0; --k) p *= 10;
    if (((uint64_t)v >> 32) == 0) return (uint8_t)('0' + (uint32_t)v / (uint32_t)p % 10u);
    return (uint8_t)('0' + (uint64_t)v / p % 10u);
}

struct extract_tables {
    const int64_t *tile0, *off, *len, *row_off, *name_off;      // [nrec + 1], [nrec], [nrec], [nrec + 1], [nrec + 1]
    const uint64_t *ex;                                         // [ntiles + 1]: sequence bytes in front of every tile
    const uint16_t *wordpre;                                    // [ntiles * BODY_WORDS]
    const dgrp_segment *rows;
    const uint8_t *names;
    int64_t nrec, flank, width;
    uint64_t class_mask;
};

struct row_layout {
    int64_t rec, start, end, label, A, B, bases, size;          // size: header + bases + line feeds
    int name_len, dA, dB, dL, dS, dE, hdr;
    bool kept;
};

// the text of row i (an index into rows): ">NAME:A-B class<label>[ core=<start>-<end>]LF", then the bases `width` per line
__device__ __forceinline__ row_layout extract_row_layout(const extract_tables &T, int64_t i)
{
    row_layout L;
    L.rec = dgrp_record_of(T.row_off, T.nrec, i);
    const int64_t seqlen = (int64_t)(T.ex[T.tile0[L.rec + 1]] - T.ex[T.tile0[L.rec]]);
    const dgrp_segment q = T.rows[i];
    L.start = q.start; L.end = q.end; L.label = q.label;
    L.kept = q.label >= 0 && q.label < 64 && ((T.class_mask >> q.label) & 1);
    L.A = q.start - (T.flank < q.start ? T.flank : q.start);
    L.B = q.end + (T.flank < seqlen - q.end ? T.flank : seqlen - q.end);
    L.bases = L.B - L.A;
    L.name_len = (int)(T.name_off[L.rec + 1] - T.name_off[L.rec]);
    L.dA = dec_digits(L.A); L.dB = dec_digits(L.B); L.dL = dec_digits(L.label < 0 ? 0 : L.label);
    L.dS = dec_digits(L.start); L.dE = dec_digits(L.end);
    L.hdr = 1 + L.name_len + 1 + L.dA + 1 + L.dB + 6 + L.dL + (T.flank > 0 ? 6 + L.dS + 1 + L.dE : 0) + 1;
    L.size = L.hdr + L.bases + (L.bases + T.width - 1) / T.width;
    return L;
}

__device__ __forceinline__ uint8_t extract_header_byte(const extract_tables &T, const row_layout &L, int q)
{
    if (q == 0) return '>';
    q -= 1;
    if (q < L.name_len) return T.names[T.name_off[L.rec] + q];
    q -= L.name_len;
    if (q == 0) return ':';
    q -= 1;
    if (q < L.dA) return dec_digit(L.A, L.dA, q);
    q -= L.dA;
    if (q == 0) return '-';
    q -= 1;
    if (q < L.dB) return dec_digit(L.B, L.dB, q);
    q -= L.dB;
    if (q < 6) return (uint8_t)" class"[q];
    q -= 6;
    if (q < L.dL) return dec_digit(L.label, L.dL, q);
    q -= L.dL;
    if (T.flank > 0) {
        if (q < 6) return (uint8_t)" core="[q];
        q -= 6;
        if (q < L.dS) return dec_digit(L.start, L.dS, q);
        q -= L.dS;
        if (q == 0) return '-';
        q -= 1;
        if (q < L.dE) return dec_digit(L.end, L.dE, q);
    }
    return '\n';
}

// one lane per row (and one behind the last): the row check of mask_kernels.hip -- 0 <= start < end <= sequence length, the rows
// of a record ascending and disjoint; g[0] |= 1 on a bad row, g[1] = smallest bad row index -- and the row's text bytes and
// kept flag, 0 for a row outside the class mask (and for the lane behind the last row: the scans then end in the totals)
__global__ void __launch_bounds__(256) extract_size_kernel(extract_tables T, unsigned long long *__restrict__ g,
                                                           uint64_t *__restrict__ rowpos, uint64_t *__restrict__ kidx)
{
    const int64_t first = T.row_off[0], nrows = T.row_off[T.nrec] - first;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nrows) return;
    if (k == nrows) {
        rowpos[k] = 0;
        kidx[k] = 0;
        return;
    }
    const int64_t i = first + k;
    const int64_t r = dgrp_record_of(T.row_off, T.nrec, i);
    const int64_t seqlen = (int64_t)(T.ex[T.tile0[r + 1]] - T.ex[T.tile0[r]]);
    const int64_t st = T.rows[i].start, en = T.rows[i].end;
    bool bad = st < 0 || en <= st || en > seqlen;
    if (i + 1 < T.row_off[r + 1] && T.rows[i + 1].start < en) bad = true;
    if (bad) {
        atomicOr(&g[0], 1ull);
        atomicMin(&g[1], (unsigned long long)i);
        rowpos[k] = 0;
        kidx[k] = 0;
        return;
    }
    const row_layout L = extract_row_layout(T, i);
    rowpos[k] = L.kept ? (uint64_t)L.size : 0;
    kidx[k] = L.kept ? 1 : 0;
}

__global__ void __launch_bounds__(256) extract_entries_kernel(extract_tables T, const uint64_t *__restrict__ rowpos,
                                                              const uint64_t *__restrict__ kidx, dgrp_extract_entry *__restrict__ entries)
{
    const int64_t first = T.row_off[0], nrows = T.row_off[T.nrec] - first;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrows || kidx[k + 1] == kidx[k]) return;
    const row_layout L = extract_row_layout(T, first + k);
    dgrp_extract_entry e;
    e.text_off = (int64_t)rowpos[k];
    e.base_off = e.text_off + L.hdr;
    e.bases = L.bases;
    entries[kidx[k]] = e;
}

// A reader of the sequence bytes of one record from sequence position p on: 16-byte words as body_load gives them (bytes outside
// the record read as line feeds), the line ends skipped.
struct seq_cursor {
    int64_t word, end;            // address of the loaded word; end of the record
    uint64_t lo, hi;              // its 16 bytes
    int j;                        // next byte of the word
};

__device__ __forceinline__ void cursor_load(const uint8_t *__restrict__ raw, int64_t off, seq_cursor &c)
{
    alignas(16) uint8_t b[16];
    if (c.word >= off && c.word + 16 <= c.end) {
        *(uint4 *)b = *(const uint4 *)(raw + c.word);
    } else {
        for (int j = 0; j < 16; ++j) b[j] = (c.word + j >= off && c.word + j < c.end) ? raw[c.word + j] : (uint8_t)'\n';
    }
    c.lo = ((const uint64_t *)b)[0];
    c.hi = ((const uint64_t *)b)[1];
}

__device__ __forceinline__ uint32_t cursor_byte(const seq_cursor &c, int j)
{
    return (uint32_t)((j < 8 ? c.lo >> (8 * j) : c.hi >> (8 * (j - 8))) & 0xff);
}

// (a position at or beyond the sequence's end reads as line feeds: the row check keeps every row inside its sequence)
__device__ __forceinline__ uint8_t cursor_next(const uint8_t *__restrict__ raw, int64_t off, seq_cursor &c)
{
    for (;;) {
        if (c.j == 16) {
            if (c.word + 16 >= c.end) return '\n';
            c.word += 16;
            c.j = 0;
            cursor_load(raw, off, c);
        }
        const uint32_t x = cursor_byte(c, c.j++);
        if (!body_lineend(x)) return (uint8_t)x;
    }
}

__device__ __forceinline__ seq_cursor cursor_open(const uint8_t *__restrict__ raw, const extract_tables &T, int64_t r, int64_t p)
{
    const int64_t t0 = T.tile0[r], t1 = T.tile0[r + 1], off = T.off[r];
    const uint64_t base = T.ex[t0];
    int64_t lo = t0, hi = t1;                     // the tile of p: the largest t < t1 with ex[t] - base <= p
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(T.ex[mid] - base) <= p) lo = mid; else hi = mid;
    }
    const int64_t rem = p - (int64_t)(T.ex[lo] - base);
    const uint16_t *wp = T.wordpre + lo * BODY_WORDS;
    int a = 0, b = BODY_WORDS;                    // the word of p: the largest w with wp[w] <= rem
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if ((int64_t)wp[mid] <= rem) a = mid; else b = mid;
    }
    seq_cursor c;
    c.end = off + T.len[r];
    c.word = (off & ~(int64_t)15) + (lo - t0) * BODY_TILE + (int64_t)a * 16;
    c.j = 0;
    cursor_load(raw, off, c);
    int skip = (int)(rem - wp[a]);                // sequence bytes of the word in front of p
    while (c.j < 16) {
        if (!body_lineend(cursor_byte(c, c.j))) {
            if (skip == 0) break;
            --skip;
        }
        ++c.j;
    }
    return c;
}

// the write: lane l of workgroup g owns the text bytes [g * EXTRACT_TILE + 16 l, + 16)
__global__ void __launch_bounds__(256) extract_write_kernel(const uint8_t *__restrict__ raw, extract_tables T,
                                                            const uint64_t *__restrict__ rowpos, int64_t total,
                                                            uint8_t *__restrict__ text)
{
    const int64_t o = (int64_t)blockIdx.x * EXTRACT_TILE + (int64_t)threadIdx.x * 16;
    if (o >= total) return;
    const int n = total - o < 16 ? (int)(total - o) : 16;
    const int64_t first = T.row_off[0], nrows = T.row_off[T.nrec] - first;
    int64_t k = dgrp_record_of((const int64_t *)rowpos, nrows, o);         // the row of byte o: the largest k with rowpos[k] <= o
    uint64_t w0 = 0, w1 = 0;
    auto put = [&](int at, uint8_t x) {
        if (at < 8) w0 |= (uint64_t)x << (8 * at); else w1 |= (uint64_t)x << (8 * (at - 8));
    };
    int at = 0;
    while (at < n) {
        const int at0 = at;
        const row_layout L = extract_row_layout(T, first + k);
        int64_t q = o + at - (int64_t)rowpos[k];
        while (at < n && q < L.hdr) put(at++, extract_header_byte(T, L, (int)q++));
        if (at < n && q < L.size) {
            const int64_t qb = q - L.hdr, line = qb / (T.width + 1);
            int64_t col = qb - line * (T.width + 1), b = line * T.width + col;
            seq_cursor c = {};
            bool open = false;
            while (at < n && q < L.size) {
                if (col == T.width || b == L.bases) {
                    put(at++, '\n');
                    col = 0;
                } else {
                    if (!open) {
                        c = cursor_open(raw, T, L.rec, L.A + b);
                        open = true;
                    }
                    put(at++, cursor_next(raw, T.off[L.rec], c));
                    ++b;
                    ++col;
                }
                ++q;
            }
        }
        if (at == at0) break;                         // (cannot happen: the scanned sizes are this layout's)
        if (at < n) k = dgrp_record_of((const int64_t *)rowpos, nrows, o + at);    // the next kept row (o + at < total: there is one)
    }
    if (n == 16 && ((uintptr_t)(text + o) & 15) == 0) {
        uint4 v;
        v.x = (uint32_t)w0; v.y = (uint32_t)(w0 >> 32); v.z = (uint32_t)w1; v.w = (uint32_t)(w1 >> 32);
        *(uint4 *)(text + o) = v;
    } else {
        for (int j = 0; j < n; ++j) text[o + j] = (uint8_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xff);
    }
}

static inline int64_t extract_scan_tiles(int64_t nrows) { return (nrows + 1 + SCAN_TILE - 1) / SCAN_TILE; }

}   // namespace

DGRP_EXPORT int64_t dgrp_fasta_extract_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows)
{
    if (nrec < 0 || total_bytes < 0 || nrows < 0) return 0;
    const int64_t tiles = body_tile_bound(nrec, total_bytes);
    return 256 + dgrp_align_up((tiles + 1) * 8, 256) + dgrp_align_up(tiles * BODY_WORDS * 2, 256) + dgrp_align_up((5 * nrec + 3) * 8, 256) +
           2 * dgrp_align_up((nrows + 1) * 8, 256) + 2 * dgrp_align_up(extract_scan_tiles(nrows) * 8, 256);
}

DGRP_EXPORT int dgrp_fasta_extract_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                                         const dgrp_segment *d_rows, const int64_t *h_row_off, const uint8_t *d_names,
                                         const int64_t *h_name_off, int64_t flank, int width, uint64_t class_mask, uint8_t *d_text,
                                         int64_t text_cap, int64_t *h_text_bytes, dgrp_extract_entry *d_entries, int64_t *h_kept,
                                         void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    // ---- host tables and scalars
    DGRP_REQUIRE(h_text_bytes && h_kept, "dgrp_fasta_extract_batch: h_text_bytes and h_kept must not be NULL");
    DGRP_REQUIRE(nrec >= 0 && (nrec == 0 || (h_off && h_len && h_row_off && h_name_off)), "dgrp_fasta_extract_batch: bad arguments");
    DGRP_REQUIRE(width >= 1 && width <= (1 << 30), "dgrp_fasta_extract_batch: width must lie in 1..2^30, got %d", width);
    DGRP_REQUIRE(flank >= 0, "dgrp_fasta_extract_batch: negative flank %lld", (long long)flank);
    DGRP_REQUIRE(text_cap >= 0 && work_bytes >= 0, "dgrp_fasta_extract_batch: negative size");
    *h_text_bytes = 0;
    *h_kept = 0;
    if (nrec == 0) return DGRP_OK;
    int64_t total = 0;
    // tile0[nrec + 1], off[nrec], len[nrec], row_off[nrec + 1], name_off[nrec + 1]
    std::vector<int64_t> tab((size_t)(5 * nrec + 3));
    int64_t *tile0 = tab.data(), *off = tile0 + nrec + 1, *len = off + nrec, *row_off = len + nrec, *name_off = row_off + nrec + 1;
    DGRP_REQUIRE(h_row_off[0] >= 0, "dgrp_fasta_extract_batch: negative row offset");
    DGRP_REQUIRE(h_name_off[0] >= 0, "dgrp_fasta_extract_batch: negative name offset");
    tile0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0, "dgrp_fasta_extract_batch: negative range (record %lld)", (long long)r);
        DGRP_REQUIRE(r == 0 || h_off[r] >= h_off[r - 1] + h_len[r - 1],
                     "dgrp_fasta_extract_batch: record ranges must ascend and not overlap (record %lld)", (long long)r);
        DGRP_REQUIRE(h_row_off[r + 1] >= h_row_off[r], "dgrp_fasta_extract_batch: row offsets must ascend (record %lld)", (long long)r);
        DGRP_REQUIRE(h_name_off[r + 1] >= h_name_off[r] && h_name_off[r + 1] - h_name_off[r] <= (1 << 20),
                     "dgrp_fasta_extract_batch: name offsets must ascend, a name has at most 2^20 bytes (record %lld)", (long long)r);
        total += h_len[r];
        off[r] = h_off[r];
        len[r] = h_len[r];
        tile0[r + 1] = tile0[r] + body_tiles_of(h_off[r], h_len[r]);
    }
    for (int64_t r = 0; r <= nrec; ++r) {
        row_off[r] = h_row_off[r];
        name_off[r] = h_name_off[r];
    }
    const int64_t ntiles = tile0[nrec], nrows = row_off[nrec] - row_off[0];
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(nrows < ((int64_t)1 << 31), "dgrp_fasta_extract_batch: more than 2^31 - 1 rows");
    // ---- the workspace
    if (work_bytes < dgrp_fasta_extract_workspace_bytes(nrec, total, nrows)) {
        dgrp_set_error("dgrp_fasta_extract_batch: workspace too small");
        return DGRP_ENOMEM;
    }
    // ---- device pointers
    DGRP_REQUIRE(d_work && d_rows && (ntiles == 0 || d_raw) && (name_off[nrec] == name_off[0] || d_names) && (text_cap == 0 || d_text),
                 "dgrp_fasta_extract_batch: NULL device pointer");
    DGRP_REQUIRE(((uintptr_t)d_raw & 15) == 0, "dgrp_fasta_extract_batch: d_raw must be 16-byte aligned");
    DGRP_REQUIRE(((uintptr_t)d_entries & 7) == 0 && ((uintptr_t)d_rows & 7) == 0 && ((uintptr_t)d_work & 255) == 0,
                 "dgrp_fasta_extract_batch: d_rows and d_entries must be 8-byte aligned, d_work 256-byte aligned");
    char *w = (char *)d_work;
    unsigned long long *g = (unsigned long long *)w;                       // bad flag, bad row, text bytes, kept rows
    w += 256;
    uint64_t *ex = (uint64_t *)w;                                           // per tile: sequence bytes, then their exclusive scan
    w += dgrp_align_up((body_tile_bound(nrec, total) + 1) * 8, 256);
    uint16_t *wordpre = (uint16_t *)w;
    w += dgrp_align_up(body_tile_bound(nrec, total) * BODY_WORDS * 2, 256);
    int64_t *d_tab = (int64_t *)w;
    w += dgrp_align_up((5 * nrec + 3) * 8, 256);
    uint64_t *rowpos = (uint64_t *)w;                                       // per row: text bytes, then their exclusive scan
    w += dgrp_align_up((nrows + 1) * 8, 256);
    uint64_t *kidx = (uint64_t *)w;                                         // per row: kept, then its exclusive scan
    w += dgrp_align_up((nrows + 1) * 8, 256);
    uint64_t *scan_a = (uint64_t *)w;
    w += dgrp_align_up(extract_scan_tiles(nrows) * 8, 256);
    uint64_t *scan_b = (uint64_t *)w;
    extract_tables T;
    T.tile0 = d_tab; T.off = d_tab + nrec + 1; T.len = T.off + nrec; T.row_off = T.len + nrec; T.name_off = T.row_off + nrec + 1;
    T.ex = ex; T.wordpre = wordpre; T.rows = d_rows; T.names = d_names;
    T.nrec = nrec; T.flank = flank; T.width = width; T.class_mask = class_mask;
    const unsigned long long init[4] = { 0ull, ~0ull, 0ull, 0ull };
    DGRP_HIP(hipMemcpyAsync(g, init, sizeof(init), hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    if (ntiles > 0) {
        hipLaunchKernelGGL(extract_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, T.tile0, T.off, T.len, nrec, ex,
                           wordpre);
        DGRP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, ex, ntiles, ex + ntiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(extract_size_kernel, dim3((unsigned)((nrows + 1 + 255) / 256)), dim3(256), 0, stream, T, g, rowpos, kidx);
    DGRP_LAUNCH_CHECK();
    int rc = device_exclusive_scan(rowpos, rowpos, nrows + 1, scan_a, (uint64_t *)(g + 2), stream);
    if (rc != DGRP_OK) return rc;
    rc = device_exclusive_scan(kidx, kidx, nrows + 1, scan_b, (uint64_t *)(g + 3), stream);
    if (rc != DGRP_OK) return rc;
    unsigned long long hg[4];
    DGRP_HIP(hipMemcpyAsync(hg, g, sizeof(hg), hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));            // the entry's one synchronisation (the host tables above were copied by now)
    if (hg[0]) {
        const int64_t i = (int64_t)hg[1];
        int64_t r = 0;
        while (r + 1 < nrec && row_off[r + 1] <= i) ++r;
        dgrp_segment q;
        uint64_t e[2];
        DGRP_HIP(hipMemcpyAsync(&q, d_rows + i, sizeof(q), hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipMemcpyAsync(&e[0], ex + tile0[r], 8, hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipMemcpyAsync(&e[1], ex + tile0[r + 1], 8, hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipStreamSynchronize(stream));        // (the error path only: fetches the offending row for the message)
        DGRP_REQUIRE(false, "dgrp_fasta_extract_batch: row %lld [%lld, %lld) of record %lld is empty, out of order or beyond its "
                            "sequence of %lld characters", (long long)i, (long long)q.start, (long long)q.end, (long long)r,
                     (long long)(e[1] - e[0]));
    }
    const int64_t text_bytes = (int64_t)hg[2];
    *h_text_bytes = text_bytes;
    *h_kept = (int64_t)hg[3];
    if (text_bytes > text_cap) {
        dgrp_set_error("dgrp_fasta_extract_batch: the text has %lld bytes, d_text holds %lld", (long long)text_bytes, (long long)text_cap);
        return DGRP_ENOMEM;
    }
    if (text_bytes == 0) return DGRP_OK;
    DGRP_REQUIRE((text_bytes + EXTRACT_TILE - 1) / EXTRACT_TILE < ((int64_t)1 << 31), "dgrp_fasta_extract_batch: more than 2^43 bytes of text");
    if (d_entries) {
        hipLaunchKernelGGL(extract_entries_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, T, rowpos, kidx,
                           d_entries);
        DGRP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(extract_write_kernel, dim3((unsigned)((text_bytes + EXTRACT_TILE - 1) / EXTRACT_TILE)), dim3(256), 0, stream,
                       d_raw, T, rowpos, text_bytes, d_text);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
