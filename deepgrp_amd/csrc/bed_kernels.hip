// predict --bed_gzip, --bed_index: the scored BED lines written on the device (dgrp_bed_text_batch: the bytes of the host formatter
// dgrp_format_bed_rows) and the tabix pieces of that text (dgrp_bed_index_batch: chunks and linear index in text offsets, the
// rules of deepgrp_amd/tabix.py).  Everything is integer arithmetic and plain stores: no floating point, no atomics.
// predict --bed_bigbed: the same rows as bigBed item blocks and coverage zoom records (dgrp_bed_blocks_batch, dgrp_bed_zoom_batch:
// the second half of this file, on the figures and the put_* helpers of the first).
//
// The chain.  check (one thread per row, raises a flag word per kind of refusal) -> rows (the line's length, 0 when filtered; for
// the index also whether it is emitted) -> exclusive scan (scan.h) -> one read-back of the totals and the flags (the only
// synchronisation) -> write.  The index compacts the emitted lines first (a second scan), marks the line that opens a chunk (a
// third), and finds a window's line by a binary search over the running maximum of (record, end) keys: records ascend with the
// lines, so the maximum of record << 32 | end over a prefix is the last record's running maximum of ends.
#include "dgrp_common.h"
#include "scan.h"
#include "tabix_bins.h"
#include <string.h>
#include <vector>

namespace {

#define BED_ONE (1ull << 24)               // q(1.0)
#define BED_MAX_BASES (1ll << 40)          // the envelope of the 64-bit rounding below
#define BED_MAX_ROWS ((1ll << 31) - 256)   // one thread per row, 256 a workgroup

enum { F_BASES, F_NAME, F_RANGE, F_SPAN, F_END, F_RECORDS, F_STARTS, F_OVERLAP, F_COUNT };
static const char *const FLAG_TEXT[F_COUNT] = {
    "a row has no scored base (bases <= 0)",
    "a row names a record outside the names (by_contig: contig not in 0..nnames-1)",
    "a row's figures lie outside the envelope (bases < 2^40, sum <= bases * 2^24, 0 <= agree <= bases)",
    "a row has start < 0 or start >= end",
    "a row lies outside the records or ends behind its record's end",
    "the records do not ascend with the rows",
    "the starts descend inside a record (tabix needs sorted rows)",
    "a row starts below the end of a row in front of it in its record (bigBed rows ascend and do not overlap)",
};

struct bed_in {
    const dgrp_segment *rows;
    const dgrp_row_score *scores;
    int64_t nrows;
    const int64_t *name_off;       // device copies of the host tables
    const char *names;
    int64_t nnames;
    int by_contig;
    uint64_t min_score;
};

// The four figures, R(num, den, k) = floor((2 k num + den) / (2 den)) of the header without a 128-bit division: with
// sum = a * bases + r (0 <= r < bases), R(sum, bases * 2^24, k) = (2 k a + 2^24 + floor(2 k r / bases)) >> 25, every term below
// 2^64 for k <= 10000, bases < 2^40 and a <= 2^24.
struct bed_figs { uint64_t score, mean, qmin, agree; };

__device__ __forceinline__ bool bed_scored(const dgrp_row_score &sc)
{
    return sc.bases > 0 && sc.bases < BED_MAX_BASES && sc.sum <= ((uint64_t)sc.bases << 24) && sc.agree >= 0 && sc.agree <= sc.bases;
}

__device__ __forceinline__ bed_figs bed_figures(const dgrp_row_score &sc)
{
    const uint64_t bases = (uint64_t)sc.bases, a = sc.sum / bases, r = sc.sum - a * bases;
    bed_figs f;
    f.score = (2000 * a + BED_ONE + 2000 * r / bases) >> 25;
    f.mean = (20000 * a + BED_ONE + 20000 * r / bases) >> 25;
    f.qmin = (20000ull * sc.qmin + BED_ONE) >> 25;
    f.agree = (20000 * (uint64_t)sc.agree + bases) / (2 * bases);
    return f;
}

__device__ __forceinline__ int dec_chars(uint64_t u)
{
    int d = 1;
    while (u >= 10) { u /= 10; ++d; }
    return d;
}

__device__ __forceinline__ int int_chars(long long v)
{
    return v < 0 ? 1 + dec_chars(0ull - (unsigned long long)v) : dec_chars((unsigned long long)v);
}

__device__ __forceinline__ char *put_dec(char *o, uint64_t u)
{
    const int d = dec_chars(u);
    for (int k = d - 1; k >= 0; --k) { o[k] = (char)('0' + u % 10); u /= 10; }
    return o + d;
}

__device__ __forceinline__ char *put_int(char *o, long long v)
{
    if (v < 0) { *o++ = '-'; return put_dec(o, 0ull - (unsigned long long)v); }
    return put_dec(o, (unsigned long long)v);
}

__device__ __forceinline__ char *put_fixed4(char *o, uint64_t v)          // v / 10^4 as "d.dddd"
{
    o = put_dec(o, v / 10000);
    const unsigned f = (unsigned)(v % 10000);
    *o++ = '.';
    *o++ = (char)('0' + f / 1000);
    *o++ = (char)('0' + f / 100 % 10);
    *o++ = (char)('0' + f / 10 % 10);
    *o++ = (char)('0' + f % 10);
    return o;
}

// the name index of a row, or -1 where it has none
__device__ __forceinline__ int64_t bed_name(const bed_in &A, const dgrp_segment &row)
{
    const int64_t c = A.by_contig ? row.contig : 0;
    return c >= 0 && c < A.nnames ? c : -1;
}

// One thread per row: every refusal raises its flag word (plain stores of the same value).  rec_end == nullptr: the text entry's
// two checks only.
__global__ void __launch_bounds__(256) bed_check_kernel(bed_in A, const int64_t *__restrict__ rec_end, int64_t nrec,
                                                        uint32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_segment row = A.rows[i];
    const dgrp_row_score sc = A.scores[i];
    if (sc.bases <= 0) flags[F_BASES] = 1;
    else if (!bed_scored(sc)) flags[F_RANGE] = 1;
    if (bed_name(A, row) < 0) flags[F_NAME] = 1;
    if (!rec_end) return;
    const int64_t r = A.by_contig ? row.contig : 0;
    if (row.start < 0 || row.start >= row.end) flags[F_SPAN] = 1;
    if (r < 0 || r >= nrec || row.end > rec_end[r]) flags[F_END] = 1;
    if (i > 0) {
        const dgrp_segment prev = A.rows[i - 1];
        const int64_t rp = A.by_contig ? prev.contig : 0;
        if (r < rp) flags[F_RECORDS] = 1;
        if (r == rp && row.start < prev.start) flags[F_STARTS] = 1;
    }
}

// One thread per row: the line's length, 0 for a filtered row (and for a row the check refuses: nothing it names is read);
// emit (the index): 1 where the line is written.
__global__ void __launch_bounds__(256) bed_rows_kernel(bed_in A, uint64_t *__restrict__ len, uint64_t *__restrict__ emit)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_segment row = A.rows[i];
    const dgrp_row_score sc = A.scores[i];
    const int64_t c = bed_name(A, row);
    uint64_t n = 0;
    if (c >= 0 && bed_scored(sc)) {
        const bed_figs f = bed_figures(sc);
        if (f.score >= A.min_score) {
            // name, start, end, "class" label, score, ".", three "d.dddd" figures, eight tabs and the line feed
            n = (uint64_t)(A.name_off[c + 1] - A.name_off[c]) + int_chars(row.start) + int_chars(row.end) + 5 + int_chars(row.label) +
                dec_chars(f.score) + 1 + dec_chars(f.mean / 10000) + dec_chars(f.qmin / 10000) + dec_chars(f.agree / 10000) + 15 + 9;
        }
    }
    len[i] = n;
    if (emit) emit[i] = n != 0;
}

// One thread per emitted row: its line at its offset.
__global__ void __launch_bounds__(256) bed_write_kernel(bed_in A, const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                        char *__restrict__ text)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const bed_figs f = bed_figures(A.scores[i]);
    const int64_t c = bed_name(A, row);
    char *o = text + off[i];
    const char *nm = A.names + A.name_off[c];
    const int64_t nlen = A.name_off[c + 1] - A.name_off[c];
    for (int64_t k = 0; k < nlen; ++k) o[k] = nm[k];
    o += nlen;
    *o++ = '\t';
    o = put_int(o, row.start); *o++ = '\t';
    o = put_int(o, row.end); *o++ = '\t';
    *o++ = 'c'; *o++ = 'l'; *o++ = 'a'; *o++ = 's'; *o++ = 's';
    o = put_int(o, row.label); *o++ = '\t';
    o = put_dec(o, f.score); *o++ = '\t';
    *o++ = '.'; *o++ = '\t';
    o = put_fixed4(o, f.mean); *o++ = '\t';
    o = put_fixed4(o, f.qmin); *o++ = '\t';
    o = put_fixed4(o, f.agree); *o++ = '\n';
}

// ---- the index -----------------------------------------------------------------------------------------------------------------
struct bed_lines {                 // the emitted lines, compacted: m = *count of them
    const uint64_t *count;
    int64_t *beg, *end;            // text offsets: the line's first byte, the byte behind it
    uint64_t *key;                 // record << 32 | the row's end
    uint32_t *bin;
};

// One thread per row: an emitted row becomes line eidx[i].
__global__ void __launch_bounds__(256) bed_compact_kernel(bed_in A, const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                          const uint64_t *__restrict__ eidx, bed_lines Ln)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const uint64_t j = eidx[i];
    Ln.beg[j] = (int64_t)off[i];
    Ln.end[j] = (int64_t)(off[i] + len[i]);
    Ln.key[j] = (uint64_t)(uint32_t)(A.by_contig ? row.contig : 0) << 32 | (uint64_t)(row.end & 0xffffffffll);
    Ln.bin[j] = tabix_reg2bin(row.start, row.end);
}

// One thread per slot: 1 where line j opens a chunk (the first line, another record, another bin), 0 elsewhere and behind the lines.
__global__ void __launch_bounds__(256) bed_opens_kernel(bed_lines Ln, int64_t nrows, uint64_t *__restrict__ opens)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nrows) return;
    uint64_t f = 0;
    if ((uint64_t)j < *Ln.count) f = j == 0 || Ln.key[j] >> 32 != Ln.key[j - 1] >> 32 || Ln.bin[j] != Ln.bin[j - 1];
    opens[j] = f;
}

// One thread per line: the line that opens chunk c writes its begin, record and bin, the line that closes it its end.
__global__ void __launch_bounds__(256) bed_chunks_kernel(bed_lines Ln, int64_t nrows, const uint64_t *__restrict__ opens,
                                                         const uint64_t *__restrict__ cidx, dgrp_track_chunk *__restrict__ chunks)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t m = (int64_t)*Ln.count;
    if (j >= nrows || j >= m) return;
    const uint64_t c = cidx[j] + opens[j] - 1;
    if (opens[j]) {
        chunks[c].beg = Ln.beg[j];
        chunks[c].rec = (int32_t)(Ln.key[j] >> 32);
        chunks[c].bin = Ln.bin[j];
    }
    if (j == m - 1 || opens[j + 1]) chunks[c].end = Ln.end[j];
}

// Inclusive maximum scan of the lines' keys in tiles of SCAN_TILE: tile maxima, their exclusive scan in one workgroup, apply.
__device__ __forceinline__ uint64_t block_exclusive_max(uint64_t v, uint64_t *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o);
        if (lane >= o && y > x) x = y;
    }
    if (lane == 63) lds[wave] = x;
    uint64_t ex = __shfl_up(x, 1);
    if (lane == 0) ex = 0;
    __syncthreads();
    for (int w = 0; w < wave; ++w) if (lds[w] > ex) ex = lds[w];
    __syncthreads();
    return ex;
}

__global__ void __launch_bounds__(256) bed_tilemax_kernel(bed_lines Ln, uint64_t *__restrict__ tilemax)
{
    __shared__ uint64_t lds[4];
    const int64_t m = (int64_t)*Ln.count, base = (int64_t)blockIdx.x * SCAN_TILE;
    uint64_t s = 0;
    for (int k = 0; k < 8; ++k) {
        const int64_t j = base + k * 256 + threadIdx.x;
        if (j < m && Ln.key[j] > s) s = Ln.key[j];
    }
    for (int o = 32; o > 0; o >>= 1) { const uint64_t y = __shfl_xor(s, o); if (y > s) s = y; }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) if (lds[w] > s) s = lds[w];
        tilemax[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) bed_tilemax_scan_kernel(uint64_t *__restrict__ tilemax, int64_t ntiles)
{
    __shared__ uint64_t lds[4];
    uint64_t carry = 0;
    for (int64_t base = 0; base < ntiles; base += 256) {
        const int64_t t = base + threadIdx.x;
        const uint64_t v = t < ntiles ? tilemax[t] : 0;
        uint64_t ex = block_exclusive_max(v, lds);
        if (carry > ex) ex = carry;
        if (t < ntiles) tilemax[t] = ex;
        const uint64_t incl = v > ex ? v : ex;            // thread 255 holds the maximum up to the end of this round
        if (threadIdx.x == 255) lds[0] = incl;
        __syncthreads();
        carry = lds[0];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) bed_runmax_kernel(bed_lines Ln, const uint64_t *__restrict__ tilemax, uint64_t *__restrict__ runmax)
{
    __shared__ uint64_t lds[4];
    const int64_t m = (int64_t)*Ln.count, base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * 8;
    uint64_t v[8], s = 0;
    for (int k = 0; k < 8; ++k) {
        v[k] = base + k < m ? Ln.key[base + k] : 0;
        if (v[k] > s) s = v[k];
    }
    uint64_t run = block_exclusive_max(s, lds);
    if (tilemax[blockIdx.x] > run) run = tilemax[blockIdx.x];
    for (int k = 0; k < 8; ++k) {
        if (v[k] > run) run = v[k];
        if (base + k < m) runmax[base + k] = run;
    }
}

__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t *a, int64_t n, uint64_t x)      // the first index with a[i] >= x
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One thread per window of the linear index: the record by a search over the window prefix, the line by a search over the running
// maximum.  The thread of a record's window 0 also states the end of the record's last line (0: the record has none).
__global__ void __launch_bounds__(256) bed_linear_kernel(bed_lines Ln, const uint64_t *__restrict__ runmax, const int64_t *__restrict__ wpref,
                                                         int64_t nrec, int64_t *__restrict__ linear, int64_t *__restrict__ rec_last)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= wpref[nrec]) return;
    int64_t lo = 0, hi = nrec;                                 // the last record r with wpref[r] <= g
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (wpref[mid] <= g) lo = mid; else hi = mid;
    }
    const uint64_t r = (uint64_t)lo, w = (uint64_t)(g - wpref[lo]);
    const int64_t m = (int64_t)*Ln.count;
    const int64_t j = lower_bound_u64(runmax, m, r << 32 | ((w << 14) + 1));
    linear[g] = j < m && runmax[j] >> 32 == r ? Ln.beg[j] : -1;
    if (w == 0 && rec_last) {
        const int64_t e = lower_bound_u64(runmax, m, (r + 1) << 32);
        rec_last[r] = e > 0 && Ln.key[e - 1] >> 32 == r ? (int64_t)(Ln.key[e - 1] & 0xffffffffull) : 0;
    }
}

// ---- the workspace -------------------------------------------------------------------------------------------------------------
struct bed_layout {
    int64_t name_off, rec_end, wpref, names, tables_bytes;     // inside the uploaded tables
    int64_t tables, len, off, tiles;                           // both entries
    int64_t emit, eidx, lbeg, lend, key, lbin, runmax, opens, cidx, tilemax;      // the index
    int64_t bytes;
};

static bool bed_carve(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec, bool index, bed_layout *l)
{
    if (nrows < 0 || nrows > BED_MAX_ROWS || nnames < 1 || nnames > (1ll << 31) - 1 || names_bytes < 0 || names_bytes > (1ll << 40)) return false;
    if (index && (nrec < 1 || nrec > (1ll << 31) - 1)) return false;
    l->name_off = 0;
    l->rec_end = l->name_off + (nnames + 1) * 8;
    l->wpref = l->rec_end + (index ? nrec * 8 : 0);
    l->names = l->wpref + (index ? (nrec + 1) * 8 : 0);
    l->tables_bytes = l->names + names_bytes;
    const int64_t ntiles = (nrows + SCAN_TILE - 1) / SCAN_TILE, col = dgrp_align_up(nrows * 8, 256);
    int64_t p = 256;                                           // totals and flags
    l->tables = p; p += dgrp_align_up(l->tables_bytes, 256);
    l->len = p; p += col;
    l->off = p; p += col;
    l->tiles = p; p += dgrp_align_up(ntiles * 8, 256);
    l->emit = l->eidx = l->lbeg = l->lend = l->key = l->lbin = l->runmax = l->opens = l->cidx = l->tilemax = 0;
    if (index) {
        l->emit = p; p += col;
        l->eidx = p; p += col;
        l->lbeg = p; p += col;
        l->lend = p; p += col;
        l->key = p; p += col;
        l->lbin = p; p += dgrp_align_up(nrows * 4, 256);
        l->runmax = p; p += col;
        l->opens = p; p += col;
        l->cidx = p; p += col;
        l->tilemax = p; p += dgrp_align_up(ntiles * 8, 256);
    }
    l->bytes = p;
    return true;
}

// header of the workspace: three totals, then the flag words
struct bed_head { uint64_t bytes, lines, chunks, pad; uint32_t flags[8]; };

static int bed_check_names(const char *who, const char *names, const int64_t *name_off, int64_t nnames)
{
    DGRP_REQUIRE(nnames >= 1 && names && name_off, "%s: bad arguments (names)", who);
    DGRP_REQUIRE(name_off[0] >= 0, "%s: name offsets must start at or above 0", who);
    for (int64_t i = 0; i < nnames; ++i) DGRP_REQUIRE(name_off[i + 1] >= name_off[i], "%s: name offsets must ascend", who);
    return DGRP_OK;
}

static int bed_refusal(const char *who, const bed_head &h)
{
    for (int k = 0; k < F_COUNT; ++k) {
        if (h.flags[k]) {
            dgrp_set_error("%s: %s", who, FLAG_TEXT[k]);
            return DGRP_EINVAL;
        }
    }
    return DGRP_OK;
}

// The shared front on checked arguments: tables up (`tab` lives until the caller's synchronisation), flags cleared, check, lengths,
// offsets.  No synchronisation.
static int bed_front(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                     const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                     const int64_t *h_wpref, char *w, const bed_layout &l, hipStream_t stream, std::vector<char> &tab, bed_in *A)
{
    tab.assign((size_t)l.tables_bytes, 0);
    memcpy(tab.data() + l.name_off, name_off, (size_t)(nnames + 1) * 8);
    if (h_rec_end) {
        memcpy(tab.data() + l.rec_end, h_rec_end, (size_t)nrec * 8);
        memcpy(tab.data() + l.wpref, h_wpref, (size_t)(nrec + 1) * 8);
    }
    if (name_off[nnames] > 0) memcpy(tab.data() + l.names, names, (size_t)name_off[nnames]);
    DGRP_HIP(hipMemcpyAsync(w + l.tables, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipMemsetAsync(w, 0, 256, stream));
    bed_head *head = (bed_head *)w;
    A->rows = d_rows; A->scores = d_scores; A->nrows = nrows;
    A->name_off = (const int64_t *)(w + l.tables + l.name_off);
    A->names = w + l.tables + l.names;
    A->nnames = nnames; A->by_contig = by_contig != 0;
    A->min_score = (uint64_t)(min_score < 0 ? 0 : min_score);
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    hipLaunchKernelGGL(bed_check_kernel, grid, block, 0, stream, *A, h_rec_end ? (const int64_t *)(w + l.tables + l.rec_end) : nullptr, nrec,
                       head->flags);
    DGRP_LAUNCH_CHECK();
    uint64_t *len = (uint64_t *)(w + l.len);
    hipLaunchKernelGGL(bed_rows_kernel, grid, block, 0, stream, *A, len, h_rec_end ? (uint64_t *)(w + l.emit) : nullptr);
    DGRP_LAUNCH_CHECK();
    return device_exclusive_scan(len, (uint64_t *)(w + l.off), nrows, (uint64_t *)(w + l.tiles), &head->bytes, stream);
}

}   // namespace

DGRP_EXPORT int64_t dgrp_bed_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes)
{
    bed_layout l;
    return bed_carve(nrows, nnames, names_bytes, 0, false, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_bed_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                                    const dgrp_row_score *d_scores, int64_t nrows, int min_score, char *d_text, int64_t cap,
                                    int64_t *h_bytes, void *d_work, int64_t work_bytes, void *stream_)
{
    static const char who[] = "dgrp_bed_text_batch";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_bytes && nrows >= 0 && cap >= 0, "%s: bad arguments", who);
    const int rc = bed_check_names(who, names, name_off, nnames);
    if (rc != DGRP_OK) return rc;
    *h_bytes = 0;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && (d_text || cap == 0), "%s: bad arguments (NULL rows, scores or text)", who);
    bed_layout l;
    DGRP_REQUIRE(bed_carve(nrows, nnames, name_off[nnames], 0, false, &l), "%s: too many rows or names (%lld, %lld)", who, (long long)nrows,
                 (long long)nnames);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<char> tab;                                      // (alive until the synchronisation below)
    bed_in A;
    int rc2 = bed_front(names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, 0, nullptr, nullptr, w, l, stream, tab, &A);
    if (rc2 != DGRP_OK) return rc2;
    bed_head head;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    *h_bytes = (int64_t)head.bytes;
    if (head.bytes == 0 || (int64_t)head.bytes > cap) return DGRP_OK;          // (too small: the caller retries with room for all of it)
    hipLaunchKernelGGL(bed_write_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, stream, A, (const uint64_t *)(w + l.len),
                       (const uint64_t *)(w + l.off), d_text);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_bed_index_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec)
{
    bed_layout l;
    return bed_carve(nrows, nnames, names_bytes, nrec, true, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_bed_index_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                                     const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                                     dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear,
                                     int64_t linear_cap, int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream_)
{
    static const char who[] = "dgrp_bed_index_batch";
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_nchunks && nrows >= 0 && chunk_cap >= 0 && linear_cap >= 0, "%s: bad arguments", who);
    const int rc = bed_check_names(who, names, name_off, nnames);
    if (rc != DGRP_OK) return rc;
    DGRP_REQUIRE(nrec >= 1 && nrec <= (1ll << 31) - 1 && h_rec_end, "%s: bad nrec %lld or no record ends", who, (long long)nrec);
    DGRP_REQUIRE(by_contig || nrec == 1, "%s: without by_contig every row belongs to record 0, so nrec must be 1, not %lld", who, (long long)nrec);
    std::vector<int64_t> wpref((size_t)nrec + 1, 0);
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_rec_end[r] >= 1 && h_rec_end[r] <= TABIX_MAX_END,
                     "%s: record %lld ends at %lld, outside 1..2^29 (the largest coordinate of a tabix index)", who, (long long)r,
                     (long long)h_rec_end[r]);
        wpref[(size_t)r + 1] = wpref[(size_t)r] + ((h_rec_end[r] - 1) >> 14) + 1;
    }
    const int64_t W = wpref[(size_t)nrec];
    DGRP_REQUIRE(W <= (1ll << 38), "%s: %lld windows in one call", who, (long long)W);
    *h_nchunks = 0;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && d_linear && (d_chunks || chunk_cap == 0), "%s: bad arguments (NULL rows, scores, chunks or linear index)", who);
    DGRP_REQUIRE(linear_cap >= W, "%s: linear_cap %lld below the %lld windows of the records", who, (long long)linear_cap, (long long)W);
    bed_layout l;
    DGRP_REQUIRE(bed_carve(nrows, nnames, name_off[nnames], nrec, true, &l), "%s: too many rows, names or records", who);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<char> tab;                                      // (alive until the synchronisation below)
    bed_in A;
    int rc2 = bed_front(names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end, wpref.data(), w, l, stream,
                        tab, &A);
    if (rc2 != DGRP_OK) return rc2;
    bed_head *d_head = (bed_head *)w;
    const uint64_t *len = (const uint64_t *)(w + l.len), *off = (const uint64_t *)(w + l.off);
    uint64_t *tiles = (uint64_t *)(w + l.tiles), *eidx = (uint64_t *)(w + l.eidx), *opens = (uint64_t *)(w + l.opens);
    uint64_t *cidx = (uint64_t *)(w + l.cidx), *tilemax = (uint64_t *)(w + l.tilemax), *runmax = (uint64_t *)(w + l.runmax);
    bed_lines Ln;
    Ln.count = &d_head->lines;
    Ln.beg = (int64_t *)(w + l.lbeg); Ln.end = (int64_t *)(w + l.lend); Ln.key = (uint64_t *)(w + l.key); Ln.bin = (uint32_t *)(w + l.lbin);
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    const int64_t ntiles = (nrows + SCAN_TILE - 1) / SCAN_TILE;
    rc2 = device_exclusive_scan((const uint64_t *)(w + l.emit), eidx, nrows, tiles, &d_head->lines, stream);
    if (rc2 != DGRP_OK) return rc2;
    hipLaunchKernelGGL(bed_compact_kernel, grid, block, 0, stream, A, len, off, (const uint64_t *)eidx, Ln);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bed_opens_kernel, grid, block, 0, stream, Ln, nrows, opens);
    DGRP_LAUNCH_CHECK();
    rc2 = device_exclusive_scan(opens, cidx, nrows, tiles, &d_head->chunks, stream);
    if (rc2 != DGRP_OK) return rc2;
    bed_head head;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    *h_nchunks = (int64_t)head.chunks;
    if ((int64_t)head.chunks > chunk_cap) return DGRP_OK;       // (too small: the caller retries with room for all of them)
    hipLaunchKernelGGL(bed_tilemax_kernel, dim3((unsigned)ntiles), block, 0, stream, Ln, tilemax);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bed_tilemax_scan_kernel, dim3(1), block, 0, stream, tilemax, ntiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bed_runmax_kernel, dim3((unsigned)ntiles), block, 0, stream, Ln, (const uint64_t *)tilemax, runmax);
    DGRP_LAUNCH_CHECK();
    if (head.chunks > 0) {
        hipLaunchKernelGGL(bed_chunks_kernel, grid, block, 0, stream, Ln, nrows, (const uint64_t *)opens, (const uint64_t *)cidx, d_chunks);
        DGRP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bed_linear_kernel, dim3((unsigned)((W + 255) / 256)), block, 0, stream, Ln, (const uint64_t *)runmax,
                       (const int64_t *)(w + l.tables + l.wpref), nrec, d_linear, d_rec_last);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// ================================================================================================================================
// predict --bed_bigbed: the same rows as the items of a bigBed file (deepgrp_amd/bigbed.py states the format).  Two entries, each a
// chain on the caller's stream with ONE read-back (totals and the check's flags) in front of the only kernel that writes an output:
//   * dgrp_bed_blocks_batch: rows (one thread per row: every check, whether the row is emitted, its item's size) -> scans of the
//     emitted flags and of the sizes (scan.h) -> per record, two binary searches over the rows' ascending records give its emitted
//     rows, hence its blocks (ceil(rows / 512)), scanned -> compaction (emitted ordinal -> row) -> write: one thread per emitted row
//     writes its item at its scanned offset; the thread of a block's first item finds the block's last one through the compaction
//     and writes the whole table row.
//   * dgrp_bed_zoom_batch: rows -> scans of the emitted flags and of the emitted rows' lengths -> compaction of (record, start),
//     (record, end) keys and the length prefix -> level 0, one thread per window of 1024 bases: two binary searches over the keys
//     give the rows that touch the window, the length prefix their bases, the two edge rows are clipped -> nine reductions four to
//     one -> count of the covered windows per 256, one scan -> records and block table.  Every (level) segment of the window space
//     starts at a multiple of 256 windows, so the scanned tile counts at the segment starts are the segment boundaries.
// A row is refused when it starts below the END of the row in front of it in its record.  That is the rule "below the largest end
// of the rows in front of it": where every row passes the test against its neighbour, start[i] >= end[i-1] > start[i-1] >=
// end[i-2] ..., so the ends ascend and the neighbour's end is the largest; where a row fails against the largest end, the first
// such row fails against its neighbour, whose end is then still the largest.  Integers only, no atomics.
namespace {

#define BB_BLOCK_ITEMS 512
#define BB_ITEM_MAX 60                     // see include/deepgrp_hip.h: 512 items are at most 30720 bytes
#define BB_MAX_END 0xffffffffll
#define BB_LEVELS DGRP_TRACK_ZOOM_LEVELS
#define BB_R0 1024                         // bases of a level-0 window
#define BB_ZOOM_BLOCK 1024                 // zoom records of a block

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
struct bbz_levels {
    int64_t R[BB_LEVELS];                  // window width in bases
    int64_t W[BB_LEVELS];                  // windows of all records
    int64_t seg[BB_LEVELS + 1];            // where the level's windows start in the window space (multiples of 256); [10]: its size
};
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

// the record of flat window g: the last r with pref[r] <= g
__device__ __forceinline__ int64_t bb_record_of(const int64_t *__restrict__ pref, int64_t nrec, int64_t g)
{
    int64_t lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (pref[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bbz_win bbz_join(const bbz_win &a, const bbz_win &b)      // every base of b above every base of a
{
    if (a.valid == 0) return b;
    if (b.valid == 0) return a;
    bbz_win w;
    w.start = a.start; w.end = b.end; w.valid = a.valid + b.valid;
    return w;
}

// level 0: one thread per window of 1024 bases.  The rows that touch [a, b) of record r are [lo, hi): lo the first row that ends
// above a, hi the first row that starts at or above b; their bases come from the length prefix, the two edge rows are clipped.
__global__ void __launch_bounds__(256) bbz_level0_kernel(bbz_rows Rw, const int64_t *__restrict__ rec_end, const int64_t *__restrict__ wpref,
                                                         int64_t nrec, bbz_levels Z, bbz_win *__restrict__ win)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bbz_win w;
    w.start = w.end = w.valid = 0;
    if (i < Z.W[0]) {
        const int64_t r = bb_record_of(wpref, nrec, i), m = (int64_t)*Rw.count;
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

// level l >= 1 from level l - 1, four windows at a time
__global__ void __launch_bounds__(256) bbz_reduce_kernel(const int64_t *__restrict__ wpref_all, int64_t nrec, bbz_levels Z, int l,
                                                         bbz_win *__restrict__ win)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t *wp = wpref_all + (int64_t)l * (nrec + 1), *wc = wp - (nrec + 1);
    bbz_win w;
    w.start = w.end = w.valid = 0;
    if (i < Z.W[l]) {
        const int64_t r = bb_record_of(wp, nrec, i), wi = i - wp[r], nc = wc[r + 1] - wc[r];
        const bbz_win *child = win + Z.seg[l - 1] + wc[r];
        for (int64_t c = 4 * wi; c < 4 * wi + 4 && c < nc; ++c) w = bbz_join(w, child[c]);
    }
    win[Z.seg[l] + i] = w;
}

// covered windows per tile of 256 windows
__global__ void __launch_bounds__(256) bbz_count_kernel(const bbz_win *__restrict__ win, uint64_t *__restrict__ tilecount)
{
    __shared__ uint64_t lds[4];
    uint64_t s = win[(int64_t)blockIdx.x * 256 + threadIdx.x].valid != 0;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tilecount[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// One workgroup: the records and the blocks in front of every level, segb [2][11], and the covered bases from the top level.
__global__ void __launch_bounds__(256) bbz_bounds_kernel(const bbz_win *__restrict__ win, const uint64_t *__restrict__ tileoff,
                                                         const uint64_t *__restrict__ grand, bbz_levels Z, uint64_t *__restrict__ segb,
                                                         uint64_t *__restrict__ covered)
{
    __shared__ uint64_t lds[4];
    uint64_t c = 0;
    for (int64_t i = threadIdx.x; i < Z.W[BB_LEVELS - 1]; i += 256) c += win[Z.seg[BB_LEVELS - 1] + i].valid;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x != 0) return;
    *covered = lds[0] + lds[1] + lds[2] + lds[3];
    uint64_t blocks = 0;
    for (int s = 0; s <= BB_LEVELS; ++s) {
        const uint64_t at = s < BB_LEVELS ? tileoff[Z.seg[s] / 256] : *grand;
        segb[s] = at;
        if (s > 0) blocks += (at - segb[s - 1] + BB_ZOOM_BLOCK - 1) / BB_ZOOM_BLOCK;
        segb[BB_LEVELS + 1 + s] = blocks;
    }
}

// the zoom records (32 bytes, two 16-byte stores) back to back in level order, and the block table
__global__ void __launch_bounds__(256) bbz_write_kernel(const bbz_win *__restrict__ win, const int64_t *__restrict__ wpref_all, int64_t nrec,
                                                        bbz_levels Z, const uint64_t *__restrict__ tileoff, const uint64_t *__restrict__ segb,
                                                        uint32_t chrom0, uint4 *__restrict__ out, dgrp_track_zoom_block *__restrict__ table)
{
    __shared__ uint64_t lds[4];
    const int64_t t0 = (int64_t)blockIdx.x * 256;
    int l = 0;
    while (l + 1 < BB_LEVELS && Z.seg[l + 1] <= t0) ++l;
    const int64_t i = t0 - Z.seg[l] + threadIdx.x;                        // the window in its level
    const bbz_win w = win[t0 + threadIdx.x];
    const uint64_t ex = block_exclusive_scan(w.valid != 0, nullptr, lds);
    if (w.valid == 0) return;
    const uint64_t at = tileoff[blockIdx.x] + ex, j = at - segb[l], n = segb[l + 1] - segb[l];
    const int64_t r = bb_record_of(wpref_all + (int64_t)l * (nrec + 1), nrec, i);
    const uint32_t one = __float_as_uint(1.0f), sum = __float_as_uint((float)w.valid);
    uint4 a, b;
    a.x = chrom0 + (uint32_t)r; a.y = w.start; a.z = w.end; a.w = w.valid;
    b.x = one; b.y = one; b.z = sum; b.w = sum;
    out[2 * at] = a;
    out[2 * at + 1] = b;
    dgrp_track_zoom_block *row = table + segb[BB_LEVELS + 1 + l] + j / BB_ZOOM_BLOCK;
    if (j % BB_ZOOM_BLOCK == 0) {
        const uint64_t left = n - j, count = left < BB_ZOOM_BLOCK ? left : BB_ZOOM_BLOCK;
        row->off = (int64_t)(32 * at);
        row->bytes = (int64_t)(32 * count);
        row->cls = 0;
        row->level = l;
        row->rec0 = (int32_t)r;
        row->start = w.start;
    }
    if (j % BB_ZOOM_BLOCK == BB_ZOOM_BLOCK - 1 || j == n - 1) {
        row->rec1 = (int32_t)r;
        row->end = w.end;
    }
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

struct bbz_layout { bbz_levels Z; int64_t rec_end, wpref, eidx, len, lsum, skey, ekey, lpref, tiles, win, wtiles, grand, segb, bytes; };

static bool bbz_carve(int64_t nrows, int64_t nrec, const int64_t *h_rec_end, bbz_layout *l)
{
    bbz_levels &Z = l->Z;
    Z.seg[0] = 0;
    for (int k = 0; k < BB_LEVELS; ++k) {
        Z.R[k] = (int64_t)BB_R0 << (2 * k);
        Z.W[k] = 0;
        for (int64_t r = 0; r < nrec; ++r) Z.W[k] += (h_rec_end[r] - 1) / Z.R[k] + 1;
        Z.seg[k + 1] = Z.seg[k] + dgrp_align_up(Z.W[k], 256);
    }
    if (Z.seg[BB_LEVELS] / 256 >= (1ll << 31)) return false;
    const int64_t col = dgrp_align_up(nrows * 8, 256);
    int64_t p = 256;                                           // totals and flags (bed_head)
    l->rec_end = p; p += dgrp_align_up(nrec * 8, 256);
    l->wpref = p; p += dgrp_align_up((nrec + 1) * BB_LEVELS * 8, 256);
    l->eidx = p; p += col;
    l->len = p; p += col;
    l->lsum = p; p += col;
    l->skey = p; p += col;
    l->ekey = p; p += col;
    l->lpref = p; p += col;
    l->tiles = p; p += dgrp_align_up((nrows + SCAN_TILE - 1) / SCAN_TILE * 8, 256);
    l->win = p; p += dgrp_align_up(Z.seg[BB_LEVELS] * (int64_t)sizeof(bbz_win), 256);
    l->wtiles = p; p += dgrp_align_up(Z.seg[BB_LEVELS] / 256 * 8, 256);
    l->grand = p; p += 256;                                    // the records of all levels, the covered bases
    l->segb = p; p += dgrp_align_up(2 * (BB_LEVELS + 1) * 8, 256);
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
    for (int s = 0; s <= BB_LEVELS; ++s) h_record_off[s] = h_block_off[s] = 0;
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
    const bbz_levels &Z = l.Z;
    std::vector<int64_t> wpref((size_t)(nrec + 1) * BB_LEVELS, 0);        // windows in front of every record, level by level
    for (int k = 0; k < BB_LEVELS; ++k) {
        int64_t *wp = wpref.data() + (size_t)k * (size_t)(nrec + 1);
        for (int64_t r = 0; r < nrec; ++r) wp[r + 1] = wp[r] + (h_rec_end[r] - 1) / Z.R[k] + 1;
    }
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
    for (int k = 1; k < BB_LEVELS; ++k) {
        hipLaunchKernelGGL(bbz_reduce_kernel, dim3((unsigned)((Z.seg[k + 1] - Z.seg[k]) / 256)), block, 0, stream, (const int64_t *)d_wpref, nrec, Z,
                           k, win);
        DGRP_LAUNCH_CHECK();
    }
    const int64_t ntiles = Z.seg[BB_LEVELS] / 256;
    hipLaunchKernelGGL(bbz_count_kernel, dim3((unsigned)ntiles), block, 0, stream, (const bbz_win *)win, wtiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), block, 0, stream, wtiles, ntiles, grand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bbz_bounds_kernel, dim3(1), block, 0, stream, (const bbz_win *)win, (const uint64_t *)wtiles, (const uint64_t *)grand, Z, segb,
                       grand + 1);
    DGRP_LAUNCH_CHECK();
    bed_head head;
    uint64_t off[2 * (BB_LEVELS + 1)], covered = 0;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(off, segb, sizeof off, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(&covered, grand + 1, 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    for (int s = 0; s <= BB_LEVELS; ++s) {
        h_record_off[s] = (int64_t)off[s];
        h_block_off[s] = (int64_t)off[BB_LEVELS + 1 + s];
    }
    if (covered) {
        h_totals->covered = h_totals->sum = h_totals->sumsq = covered;
        h_totals->qmin = h_totals->qmax = 1;
    }
    if (h_record_off[BB_LEVELS] == 0 || 32 * h_record_off[BB_LEVELS] > cap || h_block_off[BB_LEVELS] > table_cap) return DGRP_OK;   // (the caller retries)
    hipLaunchKernelGGL(bbz_write_kernel, dim3((unsigned)ntiles), block, 0, stream, (const bbz_win *)win, (const int64_t *)d_wpref, nrec, Z,
                       (const uint64_t *)wtiles, (const uint64_t *)segb, (uint32_t)chrom0, (uint4 *)d_out, d_table);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
