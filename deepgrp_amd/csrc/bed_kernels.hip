// predict --bed_gzip, --bed_index: the scored BED lines written on the device (dgrp_bed_text_batch: the bytes of the host formatter
// dgrp_format_bed_rows) and the tabix pieces of that text (dgrp_bed_index_batch: chunks and linear index in text offsets, the
// rules of deepgrp_amd/tabix.py).  Everything is integer arithmetic and plain stores: no floating point, no atomics.
// (The same rows as a bigBed file: bigbed_kernels.hip, on the figures, writers and refusals of bed_rows.h.)
//
// The chain.  check (one thread per row, raises a flag word per kind of refusal) -> rows (the line's length, 0 when filtered; for
// the index also whether it is emitted) -> exclusive scan (scan.h) -> one read-back of the totals and the flags (the only
// synchronisation) -> write.  The index compacts the emitted lines first (a second scan), marks the line that opens a chunk (a
// third), and finds a window's line by a binary search over the running maximum of (record, end) keys: records ascend with the
// lines, so the maximum of record << 32 | end over a prefix is the last record's running maximum of ends.
//
// predict --bed_gff3: the same rows as GFF3 feature lines (dgrp_gff_text_batch, dgrp_gff_index_batch; deepgrp_amd/gff.py states the
// format).  The entries of both formats are one body each (text_entry, index_entry); a format has its own rows and write kernels,
// and everything behind the line lengths -- offsets, compaction, chunks, running maximum, linear index -- is shared as it is.
#include "dgrp_common.h"
#include "bed_rows.h"
#include "scan.h"
#include "tabix_bins.h"
#include <string.h>
#include <vector>

namespace {

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

// What a GFF3 line has beyond a BED line (dgrp_gff_text_batch): the class-name table (ncnames == 0: "class<label>") and the
// number of lines the file holds in front of this text, the base of the ID ordinals.
struct gff_in {
    const int64_t *cname_off;
    const char *cnames;
    int64_t ncnames;
    uint64_t id0;
};

// the name index of a row, or -1 where it has none
__device__ __forceinline__ int64_t bed_name(const bed_in &A, const dgrp_segment &row)
{
    const int64_t c = A.by_contig ? row.contig : 0;
    return c >= 0 && c < A.nnames ? c : -1;
}

// One thread per row: every refusal raises its flag word (plain stores of the same value).  rec_end == nullptr: the text entry's
// two checks only.  ncnames > 0 (GFF3 with a class-name table): the label must name an entry.
__global__ void __launch_bounds__(256) bed_check_kernel(bed_in A, const int64_t *__restrict__ rec_end, int64_t nrec, int64_t ncnames,
                                                        uint32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_segment row = A.rows[i];
    const dgrp_row_score sc = A.scores[i];
    if (sc.bases <= 0) flags[F_BASES] = 1;
    else if (!bed_scored(sc)) flags[F_RANGE] = 1;
    if (bed_name(A, row) < 0) flags[F_NAME] = 1;
    if (ncnames > 0 && (row.label < 1 || row.label > ncnames)) flags[F_LABEL] = 1;
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

// ---- GFF3 (dgrp_gff_text_batch, dgrp_gff_index_batch) ---------------------------------------------------------------------------
// seqid \t deepgrp \t repeat_region \t start+1 \t end \t mean \t . \t . \t ID=r<j>;Name=<cname>;label=<L>;score=<score>;min=<min>;agree=<agree> \n
// A line's length depends on its ordinal j = id0 + (emitted rows in front of it) + 1, so the emitted flags are scanned before the
// lengths are.  Behind the lengths the chain is the BED's: offsets, compaction, chunks and linear index work from len and off alone.
#define GFF_SOURCE "\tdeepgrp\trepeat_region\t"
#define GFF_ID "\t.\t.\tID=r"
#define GFF_NAME ";Name="
#define GFF_LABEL ";label="
#define GFF_SCORE ";score="
#define GFF_MIN ";min="
#define GFF_AGREE ";agree="
// the literals, the two tabs behind start+1 and end, ".dddd" of three figures and the line feed
#define GFF_FIXED (sizeof(GFF_SOURCE) + sizeof(GFF_ID) + sizeof(GFF_NAME) + sizeof(GFF_LABEL) + sizeof(GFF_SCORE) + sizeof(GFF_MIN) + \
                   sizeof(GFF_AGREE) - 7 + 2 + 15 + 1)

template <int N> __device__ __forceinline__ char *put_lit(char *o, const char (&s)[N])
{
#pragma unroll
    for (int k = 0; k < N - 1; ++k) o[k] = s[k];
    return o + (N - 1);
}

__device__ __forceinline__ char *put_bytes(char *o, const char *s, int64_t n)
{
    for (int64_t k = 0; k < n; ++k) o[k] = s[k];
    return o + n;
}

// start + 1 of a 1-based closed interval, without overflow at the top of int64
__device__ __forceinline__ int start1_chars(long long start)
{
    return start < 0 ? int_chars(start + 1) : dec_chars((unsigned long long)start + 1);
}

__device__ __forceinline__ char *put_start1(char *o, long long start)
{
    return start < 0 ? put_int(o, start + 1) : put_dec(o, (unsigned long long)start + 1);
}

// One thread per row: 1 where the row gets a line (a row the check refuses gets none: nothing it names is read).
__global__ void __launch_bounds__(256) gff_emit_kernel(bed_in A, uint64_t *__restrict__ emit)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    const dgrp_row_score sc = A.scores[i];
    emit[i] = bed_name(A, A.rows[i]) >= 0 && bed_scored(sc) && bed_figures(sc).score >= A.min_score;
}

// One thread per row: the line's length from its ordinal, 0 for a row without a line.
__global__ void __launch_bounds__(256) gff_rows_kernel(bed_in A, gff_in G, const uint64_t *__restrict__ emit, const uint64_t *__restrict__ eidx,
                                                       uint64_t *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    uint64_t n = 0;
    if (emit[i]) {
        const dgrp_segment row = A.rows[i];
        const bed_figs f = bed_figures(A.scores[i]);
        const int64_t c = bed_name(A, row);
        const bool named = G.ncnames > 0 && row.label >= 1 && row.label <= G.ncnames;      // (else the check has refused the call)
        const uint64_t cname = named ? (uint64_t)(G.cname_off[row.label] - G.cname_off[row.label - 1]) : (uint64_t)(5 + int_chars(row.label));
        n = (uint64_t)(A.name_off[c + 1] - A.name_off[c]) + start1_chars(row.start) + int_chars(row.end) + dec_chars(G.id0 + eidx[i] + 1) +
            cname + int_chars(row.label) + dec_chars(f.score) + dec_chars(f.mean / 10000) + dec_chars(f.qmin / 10000) +
            dec_chars(f.agree / 10000) + GFF_FIXED;
    }
    len[i] = n;
}

// One thread per emitted row: its line at its offset.
__global__ void __launch_bounds__(256) gff_write_kernel(bed_in A, gff_in G, const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                        const uint64_t *__restrict__ eidx, char *__restrict__ text)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const bed_figs f = bed_figures(A.scores[i]);
    const int64_t c = bed_name(A, row);
    char *o = text + off[i];
    o = put_bytes(o, A.names + A.name_off[c], A.name_off[c + 1] - A.name_off[c]);
    o = put_lit(o, GFF_SOURCE);
    o = put_start1(o, row.start); *o++ = '\t';
    o = put_int(o, row.end); *o++ = '\t';
    o = put_fixed4(o, f.mean);
    o = put_lit(o, GFF_ID);
    o = put_dec(o, G.id0 + eidx[i] + 1);
    o = put_lit(o, GFF_NAME);
    if (G.ncnames > 0 && row.label >= 1 && row.label <= G.ncnames) {
        o = put_bytes(o, G.cnames + G.cname_off[row.label - 1], G.cname_off[row.label] - G.cname_off[row.label - 1]);
    } else {
        o = put_lit(o, "class");
        o = put_int(o, row.label);
    }
    o = put_lit(o, GFF_LABEL);
    o = put_int(o, row.label);
    o = put_lit(o, GFF_SCORE);
    o = put_dec(o, f.score);
    o = put_lit(o, GFF_MIN);
    o = put_fixed4(o, f.qmin);
    o = put_lit(o, GFF_AGREE);
    o = put_fixed4(o, f.agree); *o++ = '\n';
}

// ---- the index -----------------------------------------------------------------------------------------------------------------
struct bed_lines {                 // the emitted lines, compacted: m = *count of them
    const uint64_t *count;
    int64_t *beg, *end;            // text offsets: the line's first byte, the byte behind it
    uint64_t *key;                 // record << 32 | the row's end - 1 (the end itself reaches 2^32 under a CSI index of depth 6)
    uint32_t *bin;
};

// One thread per row: an emitted row becomes line eidx[i].
__global__ void __launch_bounds__(256) bed_compact_kernel(bed_in A, const uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                          const uint64_t *__restrict__ eidx, bed_lines Ln, int depth)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows || len[i] == 0) return;
    const dgrp_segment row = A.rows[i];
    const uint64_t j = eidx[i];
    Ln.beg[j] = (int64_t)off[i];
    Ln.end[j] = (int64_t)(off[i] + len[i]);
    Ln.key[j] = (uint64_t)(uint32_t)(A.by_contig ? row.contig : 0) << 32 | (uint64_t)((row.end - 1) & 0xffffffffll);
    Ln.bin[j] = tabix_reg2bin_depth(row.start, row.end, depth);
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

// One thread per window of the linear index: the record by a search over the window prefix, the line by a search over the running
// maximum.  The thread of a record's window 0 also states the end of the record's last line (0: the record has none).
__global__ void __launch_bounds__(256) bed_linear_kernel(bed_lines Ln, const uint64_t *__restrict__ runmax, const int64_t *__restrict__ wpref,
                                                         int64_t nrec, int64_t *__restrict__ linear, int64_t *__restrict__ rec_last)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= wpref[nrec]) return;
    const int64_t lo = dgrp_record_of(wpref, nrec, g);
    const uint64_t r = (uint64_t)lo, w = (uint64_t)(g - wpref[lo]);
    const int64_t m = (int64_t)*Ln.count;
    const int64_t j = lower_bound_u64(runmax, m, r << 32 | w << 14);             // end > w << 14: end - 1 >= w << 14, w < 2^18
    linear[g] = j < m && runmax[j] >> 32 == r ? Ln.beg[j] : -1;
    if (w == 0 && rec_last) {
        const int64_t e = lower_bound_u64(runmax, m, (r + 1) << 32);
        rec_last[r] = e > 0 && Ln.key[e - 1] >> 32 == r ? (int64_t)(Ln.key[e - 1] & 0xffffffffull) + 1 : 0;
    }
}

// ---- the workspace -------------------------------------------------------------------------------------------------------------
struct bed_layout {
    int64_t name_off, rec_end, wpref, cname_off, names, cnames, tables_bytes;     // inside the uploaded tables
    int64_t tables, len, off, tiles;                           // both entries
    int64_t emit, eidx, lbeg, lend, key, lbin, runmax, opens, cidx, tilemax;      // the index
    int64_t bytes;
};

// gff: the class-name table travels with the names (ncnames entries, cnames_bytes bytes) and the text entry has the two columns of
// the ordinal scan as well.  Without it the layout is the BED's, byte for byte.
static bool bed_carve(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec, bool index, bed_layout *l, bool gff = false,
                      int64_t ncnames = 0, int64_t cnames_bytes = 0)
{
    if (nrows < 0 || nrows > BED_MAX_ROWS || nnames < 1 || nnames > (1ll << 31) - 1 || names_bytes < 0 || names_bytes > (1ll << 40)) return false;
    if (index && (nrec < 1 || nrec > (1ll << 31) - 1)) return false;
    if (gff && (ncnames < 0 || ncnames > (1ll << 31) - 1 || cnames_bytes < 0 || cnames_bytes > (1ll << 40))) return false;
    l->name_off = 0;
    l->rec_end = l->name_off + (nnames + 1) * 8;
    l->wpref = l->rec_end + (index ? nrec * 8 : 0);
    l->cname_off = l->wpref + (index ? (nrec + 1) * 8 : 0);
    l->names = l->cname_off + (gff ? (ncnames + 1) * 8 : 0);
    l->cnames = l->names + names_bytes;
    l->tables_bytes = l->cnames + (gff ? cnames_bytes : 0);
    const int64_t ntiles = (nrows + SCAN_TILE - 1) / SCAN_TILE, col = dgrp_align_up(nrows * 8, 256);
    int64_t p = 256;                                           // totals and flags
    l->tables = p; p += dgrp_align_up(l->tables_bytes, 256);
    l->len = p; p += col;
    l->off = p; p += col;
    l->tiles = p; p += dgrp_align_up(ntiles * 8, 256);
    l->emit = l->eidx = l->lbeg = l->lend = l->key = l->lbin = l->runmax = l->opens = l->cidx = l->tilemax = 0;
    if (index || gff) {
        l->emit = p; p += col;
        l->eidx = p; p += col;
    }
    if (index) {
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

static int bed_check_names(const char *who, const char *names, const int64_t *name_off, int64_t nnames)
{
    DGRP_REQUIRE(nnames >= 1 && names && name_off, "%s: bad arguments (names)", who);
    DGRP_REQUIRE(name_off[0] >= 0, "%s: name offsets must start at or above 0", who);
    for (int64_t i = 0; i < nnames; ++i) DGRP_REQUIRE(name_off[i + 1] >= name_off[i], "%s: name offsets must ascend", who);
    return DGRP_OK;
}

// What the GFF3 entries hand the front beside the BED's arguments (host tables; nullptr: BED).
struct gff_host {
    const char *cnames;
    const int64_t *cname_off;
    int64_t ncnames, id0;
};

// The shared front on checked arguments: tables up (`tab` lives until the caller's synchronisation), flags cleared, check, lengths,
// offsets.  No synchronisation.  With H (GFF3): the emitted flags and their scan (the ordinals, head->lines) come before the
// lengths, and *G is what the write kernel takes.
static int bed_front(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                     const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                     const int64_t *h_wpref, char *w, const bed_layout &l, hipStream_t stream, std::vector<char> &tab, bed_in *A,
                     const gff_host *H = nullptr, gff_in *G = nullptr)
{
    tab.assign((size_t)l.tables_bytes, 0);
    memcpy(tab.data() + l.name_off, name_off, (size_t)(nnames + 1) * 8);
    if (h_rec_end) {
        memcpy(tab.data() + l.rec_end, h_rec_end, (size_t)nrec * 8);
        memcpy(tab.data() + l.wpref, h_wpref, (size_t)(nrec + 1) * 8);
    }
    if (name_off[nnames] > 0) memcpy(tab.data() + l.names, names, (size_t)name_off[nnames]);
    if (H && H->ncnames > 0) {
        memcpy(tab.data() + l.cname_off, H->cname_off, (size_t)(H->ncnames + 1) * 8);
        if (H->cname_off[H->ncnames] > 0) memcpy(tab.data() + l.cnames, H->cnames, (size_t)H->cname_off[H->ncnames]);
    }
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
                       H ? H->ncnames : (int64_t)0, head->flags);
    DGRP_LAUNCH_CHECK();
    uint64_t *len = (uint64_t *)(w + l.len);
    if (H) {
        G->cname_off = (const int64_t *)(w + l.tables + l.cname_off);
        G->cnames = w + l.tables + l.cnames;
        G->ncnames = H->ncnames; G->id0 = (uint64_t)H->id0;
        uint64_t *emit = (uint64_t *)(w + l.emit), *eidx = (uint64_t *)(w + l.eidx);
        hipLaunchKernelGGL(gff_emit_kernel, grid, block, 0, stream, *A, emit);
        DGRP_LAUNCH_CHECK();
        const int rc = device_exclusive_scan(emit, eidx, nrows, (uint64_t *)(w + l.tiles), &head->lines, stream);
        if (rc != DGRP_OK) return rc;
        hipLaunchKernelGGL(gff_rows_kernel, grid, block, 0, stream, *A, *G, (const uint64_t *)emit, (const uint64_t *)eidx, len);
        DGRP_LAUNCH_CHECK();
        return device_exclusive_scan(len, (uint64_t *)(w + l.off), nrows, (uint64_t *)(w + l.tiles), &head->bytes, stream);
    }
    hipLaunchKernelGGL(bed_rows_kernel, grid, block, 0, stream, *A, len, h_rec_end ? (uint64_t *)(w + l.emit) : nullptr);
    DGRP_LAUNCH_CHECK();
    return device_exclusive_scan(len, (uint64_t *)(w + l.off), nrows, (uint64_t *)(w + l.tiles), &head->bytes, stream);
}

// The host checks of the GFF3 arguments (class-name table, id0).
static int gff_check_host(const char *who, const gff_host &H)
{
    DGRP_REQUIRE(H.id0 >= 0 && H.id0 <= (1ll << 62), "%s: id0 %lld outside 0..2^62 (the lines in front of this text)", who, (long long)H.id0);
    DGRP_REQUIRE(H.ncnames >= 0 && H.ncnames <= (1ll << 31) - 1, "%s: bad class-name count %lld", who, (long long)H.ncnames);
    if (H.ncnames == 0) return DGRP_OK;
    DGRP_REQUIRE(H.cnames && H.cname_off, "%s: bad arguments (class names)", who);
    DGRP_REQUIRE(H.cname_off[0] >= 0, "%s: class-name offsets must start at or above 0", who);
    for (int64_t i = 0; i < H.ncnames; ++i) DGRP_REQUIRE(H.cname_off[i + 1] >= H.cname_off[i], "%s: class-name offsets must ascend", who);
    return DGRP_OK;
}

// The text entry of both formats (H == nullptr: BED; h_lines: GFF3 only).
static int text_entry(const char *who, const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                      const dgrp_row_score *d_scores, int64_t nrows, int min_score, char *d_text, int64_t cap, int64_t *h_bytes,
                      void *d_work, int64_t work_bytes, hipStream_t stream, const gff_host *H, int64_t *h_lines)
{
    DGRP_REQUIRE(h_bytes && (h_lines || !H) && nrows >= 0 && cap >= 0, "%s: bad arguments", who);
    const int rc = bed_check_names(who, names, name_off, nnames);
    if (rc != DGRP_OK) return rc;
    if (H) {
        const int rcg = gff_check_host(who, *H);
        if (rcg != DGRP_OK) return rcg;
        *h_lines = 0;
    }
    *h_bytes = 0;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && (d_text || cap == 0), "%s: bad arguments (NULL rows, scores or text)", who);
    bed_layout l;
    DGRP_REQUIRE(bed_carve(nrows, nnames, name_off[nnames], 0, false, &l, H != nullptr, H ? H->ncnames : 0,
                           H && H->ncnames ? H->cname_off[H->ncnames] : 0),
                 "%s: too many rows or names (%lld, %lld)", who, (long long)nrows, (long long)nnames);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<char> tab;                                      // (alive until the synchronisation below)
    bed_in A;
    gff_in G;
    int rc2 = bed_front(names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, 0, nullptr, nullptr, w, l, stream, tab, &A,
                        H, &G);
    if (rc2 != DGRP_OK) return rc2;
    bed_head head;
    DGRP_HIP(hipMemcpyAsync(&head, w, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    rc2 = bed_refusal(who, head);
    if (rc2 != DGRP_OK) return rc2;
    *h_bytes = (int64_t)head.bytes;
    if (H) *h_lines = (int64_t)head.lines;
    if (head.bytes == 0 || (int64_t)head.bytes > cap) return DGRP_OK;          // (too small: the caller retries with room for all of it)
    const dim3 grid((unsigned)((nrows + 255) / 256)), block(256);
    if (H) {
        hipLaunchKernelGGL(gff_write_kernel, grid, block, 0, stream, A, G, (const uint64_t *)(w + l.len), (const uint64_t *)(w + l.off),
                           (const uint64_t *)(w + l.eidx), d_text);
    } else {
        hipLaunchKernelGGL(bed_write_kernel, grid, block, 0, stream, A, (const uint64_t *)(w + l.len), (const uint64_t *)(w + l.off), d_text);
    }
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

// The index entry of both formats (H == nullptr: BED): behind the front everything works from the lengths and offsets of the lines.
// depth: the levels below the root of the binning scheme (5: a .tbi; csi: the entry takes 5 or 6 and names the limit of a CSI index).
static int index_entry(const char *who, int depth, bool csi, const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                       const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                       dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear, int64_t linear_cap,
                       int64_t *d_rec_last, void *d_work, int64_t work_bytes, hipStream_t stream, const gff_host *H)
{
    DGRP_REQUIRE(depth == TABIX_DEPTH || depth == CSI_DEPTH, "%s: depth must be 5 or 6, got %d", who, depth);
    DGRP_REQUIRE(h_nchunks && nrows >= 0 && chunk_cap >= 0 && linear_cap >= 0, "%s: bad arguments", who);
    const int rc = bed_check_names(who, names, name_off, nnames);
    if (rc != DGRP_OK) return rc;
    if (H) {
        const int rcg = gff_check_host(who, *H);
        if (rcg != DGRP_OK) return rcg;
    }
    DGRP_REQUIRE(nrec >= 1 && nrec <= (1ll << 31) - 1 && h_rec_end, "%s: bad nrec %lld or no record ends", who, (long long)nrec);
    DGRP_REQUIRE(by_contig || nrec == 1, "%s: without by_contig every row belongs to record 0, so nrec must be 1, not %lld", who, (long long)nrec);
    std::vector<int64_t> wpref((size_t)nrec + 1, 0);
    for (int64_t r = 0; r < nrec; ++r) {
        if (csi) {
            DGRP_REQUIRE(h_rec_end[r] >= 1 && h_rec_end[r] <= tabix_max_end(depth),
                         "%s: record %lld ends at %lld, outside 1..2^%d = %lld (the largest coordinate of a CSI index of depth %d)", who,
                         (long long)r, (long long)h_rec_end[r], TABIX_MIN_SHIFT + 3 * depth, (long long)tabix_max_end(depth), depth);
        } else {
            DGRP_REQUIRE(h_rec_end[r] >= 1 && h_rec_end[r] <= TABIX_MAX_END,
                         "%s: record %lld ends at %lld, outside 1..2^29 (the largest coordinate of a tabix index)", who, (long long)r,
                         (long long)h_rec_end[r]);
        }
        wpref[(size_t)r + 1] = wpref[(size_t)r] + ((h_rec_end[r] - 1) >> 14) + 1;
    }
    const int64_t W = wpref[(size_t)nrec];
    DGRP_REQUIRE(W <= (1ll << 38), "%s: %lld windows in one call", who, (long long)W);
    *h_nchunks = 0;
    if (nrows == 0) return DGRP_OK;
    DGRP_REQUIRE(d_rows && d_scores && d_linear && (d_chunks || chunk_cap == 0), "%s: bad arguments (NULL rows, scores, chunks or linear index)", who);
    DGRP_REQUIRE(linear_cap >= W, "%s: linear_cap %lld below the %lld windows of the records", who, (long long)linear_cap, (long long)W);
    bed_layout l;
    DGRP_REQUIRE(bed_carve(nrows, nnames, name_off[nnames], nrec, true, &l, H != nullptr, H ? H->ncnames : 0,
                           H && H->ncnames ? H->cname_off[H->ncnames] : 0),
                 "%s: too many rows, names or records", who);
    if (!d_work || work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace too small (%lld < %lld bytes)", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    char *w = (char *)d_work;
    std::vector<char> tab;                                      // (alive until the synchronisation below)
    bed_in A;
    gff_in G;
    int rc2 = bed_front(names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end, wpref.data(), w, l, stream,
                        tab, &A, H, &G);
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
    if (!H) {                                                   // (GFF3: the front has scanned the emitted flags for the ordinals)
        rc2 = device_exclusive_scan((const uint64_t *)(w + l.emit), eidx, nrows, tiles, &d_head->lines, stream);
        if (rc2 != DGRP_OK) return rc2;
    }
    hipLaunchKernelGGL(bed_compact_kernel, grid, block, 0, stream, A, len, off, (const uint64_t *)eidx, Ln, depth);
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
    return text_entry("dgrp_bed_text_batch", names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, d_text, cap, h_bytes,
                      d_work, work_bytes, (hipStream_t)stream_, nullptr, nullptr);
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
    return index_entry("dgrp_bed_index_batch", TABIX_DEPTH, false, names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end,
                       d_chunks, chunk_cap, h_nchunks, d_linear, linear_cap, d_rec_last, d_work, work_bytes, (hipStream_t)stream_, nullptr);
}

DGRP_EXPORT int64_t dgrp_gff_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes)
{
    bed_layout l;
    return bed_carve(nrows, nnames, names_bytes, 0, false, &l, true, ncnames, cnames_bytes) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_gff_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                                    const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                                    int64_t nrows, int min_score, int64_t id0, char *d_text, int64_t cap, int64_t *h_bytes,
                                    int64_t *h_lines, void *d_work, int64_t work_bytes, void *stream_)
{
    const gff_host H = {cnames, cname_off, ncnames, id0};
    return text_entry("dgrp_gff_text_batch", names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, d_text, cap, h_bytes,
                      d_work, work_bytes, (hipStream_t)stream_, &H, h_lines);
}

DGRP_EXPORT int64_t dgrp_gff_index_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames,
                                                   int64_t cnames_bytes, int64_t nrec)
{
    bed_layout l;
    return bed_carve(nrows, nnames, names_bytes, nrec, true, &l, true, ncnames, cnames_bytes) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_gff_index_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                                     const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                                     int64_t nrows, int min_score, int64_t id0, int64_t nrec, const int64_t *h_rec_end,
                                     dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear,
                                     int64_t linear_cap, int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream_)
{
    const gff_host H = {cnames, cname_off, ncnames, id0};
    return index_entry("dgrp_gff_index_batch", TABIX_DEPTH, false, names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec, h_rec_end,
                       d_chunks, chunk_cap, h_nchunks, d_linear, linear_cap, d_rec_last, d_work, work_bytes, (hipStream_t)stream_, &H);
}

// ---- CSI (predict --index_format csi): the index entries with the depth of the binning scheme as an argument; the workspace is the
// .tbi entries' (the depth changes bin numbers and the record-end limit, no layout)
DGRP_EXPORT int64_t dgrp_bed_csi_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec, int depth)
{
    return depth == TABIX_DEPTH || depth == CSI_DEPTH ? dgrp_bed_index_workspace_bytes(nrows, nnames, names_bytes, nrec) : 0;
}

DGRP_EXPORT int dgrp_bed_csi_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                                   const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                                   int depth, dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear,
                                   int64_t linear_cap, int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream_)
{
    return index_entry("dgrp_bed_csi_batch", depth, true, names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec,
                       h_rec_end, d_chunks, chunk_cap, h_nchunks, d_linear, linear_cap, d_rec_last, d_work, work_bytes, (hipStream_t)stream_,
                       nullptr);
}

DGRP_EXPORT int64_t dgrp_gff_csi_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes,
                                                 int64_t nrec, int depth)
{
    return depth == TABIX_DEPTH || depth == CSI_DEPTH ? dgrp_gff_index_workspace_bytes(nrows, nnames, names_bytes, ncnames, cnames_bytes, nrec)
                                                      : 0;
}

DGRP_EXPORT int dgrp_gff_csi_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                                   const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                                   int64_t nrows, int min_score, int64_t id0, int64_t nrec, const int64_t *h_rec_end, int depth,
                                   dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear,
                                   int64_t linear_cap, int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream_)
{
    const gff_host H = {cnames, cname_off, ncnames, id0};
    return index_entry("dgrp_gff_csi_batch", depth, true, names, name_off, nnames, by_contig, d_rows, d_scores, nrows, min_score, nrec,
                       h_rec_end, d_chunks, chunk_cap, h_nchunks, d_linear, linear_cap, d_rec_last, d_work, work_bytes, (hipStream_t)stream_,
                       &H);
}
