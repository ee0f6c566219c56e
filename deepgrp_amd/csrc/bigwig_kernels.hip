// bigWig tracks (predict --track_bigwig): the items of the probability tracks as binary bedGraph sections, their zoom summaries, and
// zlib streams of both, built in HBM.  Three entries, each a chain on the caller's stream:
//   * dgrp_track_sections_batch: the shared bin pass (track_chain.h: q of every class, record and bin), then
//       count   -- the items ending in every tile of 2048 bins, and by integer atomics the items of every (class, record);
//       scans   -- of the tile counts (scan.h) and, per class, of the records' items and sections (ceil(items / 1024));
//       write   -- an item exists as the bin where its run starts, which stores `start`, and the bin where it ends, which stores
//                  `end` and the value: both know the item's ordinal (the exclusive count of run ends in front of them), hence its
//                  section and slot by arithmetic.  The first item of a section also writes the header and the table row, the last
//                  one chromEnd.  No lane walks a run.
//   * dgrp_track_zoom_batch: the bin pass, then level 0 (one lane per window of 16 bins, integer summaries), nine reductions four to
//     one, a count of the windows with a covered base, one scan, and the 32-byte records with their block table.  Every (class,
//     level) segment of the window space starts at a multiple of 256 windows, so the scanned tile counts at the segment starts are
//     the segment boundaries.  Everything behind level 0 but the totals is the ladder of bbi_zoom.h, which bigbed_kernels.hip shares.
//   * dgrp_zlib_compress_batch: the member kernels of deflate_kernels.hip on a table of blocks, then one workgroup per block frames
//     the DEFLATE block as a zlib stream: the Adler-32 of the block from per-lane sums (a = sum of bytes, b = sum of (len - i) *
//     byte, 64-bit, reduced modulo 65521 per lane and again after the tree), no serial walk.
// All sums are integers; a floating-point value is one double division of an integer, rounded once to float.
// See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "deflate.h"
#include "deflate_blocks.h"
#include "scan.h"
#include "track_chain.h"
#include "bbi_zoom.h"
#include <string.h>
#include <vector>

namespace {

#define BW_SECTION_ITEMS 1024
#define BW_MAX_END 0xffffffffll          // the largest coordinate of a bigWig

// (float)((double)v / (double)scale): the float32 a reader gets from the decimal text
__device__ __forceinline__ float bw_value(uint64_t v, double scale) { return (float)((double)v / scale); }

// ------------------------------------------------------------------------------------------------------------------- sections
struct bw_run { uint32_t v; bool first, last; int64_t r, lo, hi; };

// flat bin f of one class (qk: its NBpad values; bins in [NB, NBpad) read as 0): does a run start or end here, and where
__device__ __forceinline__ bw_run bw_run_of(const uint32_t *__restrict__ qk, const tb_rec *__restrict__ recs,
                                            const int64_t *__restrict__ pref, const tb_geom &G, int64_t r0, int64_t f0, int64_t f)
{
    bw_run t;
    t.v = f < G.NB ? qk[f] : 0u;
    t.first = t.last = false;
    t.r = t.lo = t.hi = 0;
    if (t.v == 0) return t;
    t.r = tb_record_from(pref, G.nrec, r0, f0, f);
    const int64_t j = f - pref[t.r], nb = recs[t.r].nb;
    t.first = j == 0 || qk[f - 1] != t.v;
    t.last = j == nb - 1 || qk[f + 1] != t.v;
    if (t.first || t.last) track_bin_span(tb_geom_of(recs[t.r], G.bin), j, t.lo, t.hi);
    return t;
}

// items that end in every tile, and the items of every (class, record): cnt[k * nrec + r] (zeroed), integer atomics -- one per tile
// for the record the tile starts in (counted in LDS), one per item for records that start inside the tile
__global__ void __launch_bounds__(256) bw_count_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                       const int64_t *__restrict__ pref, tb_geom G, uint64_t *__restrict__ tilecount,
                                                       unsigned long long *__restrict__ cnt)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_r0;
    __shared__ unsigned int s_own;
    const int64_t tpc = G.NBpad / TRACK_TILE;
    const int64_t k = blockIdx.x / tpc, f0 = ((int64_t)blockIdx.x % tpc) * TRACK_TILE;
    if (threadIdx.x == 0) {
        s_r0 = f0 < G.NB ? dgrp_record_of(pref, G.nrec, f0) : 0;
        s_own = 0;
    }
    __syncthreads();
    const int64_t r0 = s_r0;
    const uint32_t *qk = q + k * G.NBpad;
    uint64_t s = 0;
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const bw_run t = bw_run_of(qk, recs, pref, G, r0, f0, f0 + r * 256 + threadIdx.x);
        if (!t.last) continue;
        ++s;
        if (t.r == r0) atomicAdd(&s_own, 1u);
        else atomicAdd(&cnt[k * G.nrec + t.r], 1ull);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        tilecount[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
        if (s_own) atomicAdd(&cnt[k * G.nrec + r0], (unsigned long long)s_own);
    }
}

// per class (one workgroup each): the items and the sections in front of every record, ipref and spref [ncls][nrec + 1]
__global__ void __launch_bounds__(256) bw_prefix_kernel(const unsigned long long *__restrict__ cnt, int64_t nrec, uint64_t *__restrict__ ipref,
                                                        uint64_t *__restrict__ spref)
{
    __shared__ uint64_t lds[4];
    const int64_t k = blockIdx.x;
    const unsigned long long *c = cnt + k * nrec;
    uint64_t *ip = ipref + k * (nrec + 1), *sp = spref + k * (nrec + 1);
    uint64_t ci = 0, cs = 0;
    for (int64_t base = 0; base < nrec; base += 256) {
        const int64_t r = base + threadIdx.x;
        const uint64_t v = r < nrec ? c[r] : 0, sv = (v + BW_SECTION_ITEMS - 1) / BW_SECTION_ITEMS;
        uint64_t ti, ts;
        const uint64_t ei = block_exclusive_scan(v, &ti, lds);
        const uint64_t es = block_exclusive_scan(sv, &ts, lds);
        if (r < nrec) {
            ip[r] = ci + ei;
            sp[r] = cs + es;
        }
        ci += ti;
        cs += ts;
    }
    if (threadIdx.x == 0) {
        ip[nrec] = ci;
        sp[nrec] = cs;
    }
}

// the class boundaries: items and sections in front of every class (base [2][ncls + 1]), and for the host the byte offset of every
// class's sections and the section prefix (hb [2][ncls + 1])
__global__ void __launch_bounds__(64) bw_bounds_kernel(const uint64_t *__restrict__ ipref, const uint64_t *__restrict__ spref, int64_t nrec,
                                                      int ncls, uint64_t *__restrict__ base, uint64_t *__restrict__ hb)
{
    if (threadIdx.x != 0) return;
    uint64_t it = 0, se = 0;
    for (int k = 0; k <= ncls; ++k) {
        base[k] = it;
        base[ncls + 1 + k] = se;
        hb[k] = 24 * se + 12 * it;
        hb[ncls + 1 + k] = se;
        if (k < ncls) {
            it += ipref[(int64_t)k * (nrec + 1) + nrec];
            se += spref[(int64_t)k * (nrec + 1) + nrec];
        }
    }
}

// the sections and their table (see the head of the file)
__global__ void __launch_bounds__(256) bw_write_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                       const int64_t *__restrict__ pref, tb_geom G, double scale,
                                                       const uint64_t *__restrict__ tileoff, const unsigned long long *__restrict__ cnt,
                                                       const uint64_t *__restrict__ ipref, const uint64_t *__restrict__ spref,
                                                       const uint64_t *__restrict__ base, uint32_t chrom0,
                                                       char *__restrict__ out, dgrp_track_section *__restrict__ table)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_r0;
    const int64_t tpc = G.NBpad / TRACK_TILE;
    const int64_t k = blockIdx.x / tpc, f0 = ((int64_t)blockIdx.x % tpc) * TRACK_TILE;
    if (threadIdx.x == 0) s_r0 = f0 < G.NB ? dgrp_record_of(pref, G.nrec, f0) : 0;
    __syncthreads();
    const int64_t r0 = s_r0;
    const uint32_t *qk = q + k * G.NBpad;
    const uint64_t ibase = base[k], sbase = base[G.ncls + 1 + k];
    const uint64_t cbytes = 24 * sbase + 12 * ibase;                      // where the class's sections start
    uint64_t g0 = tileoff[blockIdx.x] - ibase;                            // the class's items in front of the tile
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const bw_run t = bw_run_of(qk, recs, pref, G, r0, f0, f0 + r * 256 + threadIdx.x);
        uint64_t round;
        const uint64_t g = g0 + block_exclusive_scan(t.last ? 1 : 0, &round, lds);   // the ordinal of the item this bin starts or ends
        g0 += round;
        if (!t.first && !t.last) continue;
        const int64_t kr = k * (G.nrec + 1) + t.r;
        const uint64_t ir = g - ipref[kr], slot = ir % BW_SECTION_ITEMS, sec = spref[kr] + ir / BW_SECTION_ITEMS;
        const uint64_t total = cnt[k * G.nrec + t.r];
        const uint64_t secoff = cbytes + 24 * sec + 12 * (g - slot);
        uint32_t *head = reinterpret_cast<uint32_t *>(out + secoff), *item = head + 6 + 3 * slot;
        dgrp_track_section *row = table + sbase + sec;
        if (t.first) {
            item[0] = (uint32_t)t.lo;
            if (slot == 0) {
                const uint64_t left = total - ir, count = left < BW_SECTION_ITEMS ? left : BW_SECTION_ITEMS;
                head[0] = chrom0 + (uint32_t)t.r;
                head[1] = (uint32_t)t.lo;
                head[3] = 0;
                head[4] = 0;
                head[5] = 1u | ((uint32_t)count << 16);                   // type 1 (bedGraph), reserved, itemCount
                row->off = (int64_t)secoff;
                row->bytes = (int64_t)(24 + 12 * count);
                row->rec = (int32_t)t.r;
                row->start = (uint32_t)t.lo;
                row->pad = 0;
            }
        }
        if (t.last) {
            item[1] = (uint32_t)t.hi;
            item[2] = __float_as_uint(bw_value(t.v, scale));
            if (slot == BW_SECTION_ITEMS - 1 || ir == total - 1) {
                head[2] = (uint32_t)t.hi;
                row->end = (uint32_t)t.hi;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- zoom
struct bwz_win { uint64_t s1, s2; uint32_t start, end, valid, qmin, qmax, pad; };     // a window's integer summary; valid 0: none

// a and b, every base of b above every base of a
__device__ __forceinline__ bwz_win bbi_join(const bwz_win &a, const bwz_win &b)
{
    if (a.valid == 0) return b;
    if (b.valid == 0) return a;
    bwz_win w;
    w.s1 = a.s1 + b.s1;
    w.s2 = a.s2 + b.s2;
    w.start = a.start;
    w.end = b.end;
    w.valid = a.valid + b.valid;
    w.qmin = a.qmin < b.qmin ? a.qmin : b.qmin;
    w.qmax = a.qmax > b.qmax ? a.qmax : b.qmax;
    w.pad = 0;
    return w;
}

struct bwz_start {                       // a record's first base: its windows are numbered in the record's coordinates
    const tb_rec *recs;
    __device__ __forceinline__ int64_t operator()(int64_t r) const { return recs[r].offset; }
};

struct bwz_tail {                        // min, max, sum and sum of squares of a window's values: one double division each
    double scale;
    __device__ __forceinline__ uint4 operator()(const bwz_win &w) const
    {
        uint4 b;
        b.x = __float_as_uint(bw_value(w.qmin, scale));
        b.y = __float_as_uint(bw_value(w.qmax, scale));
        b.z = __float_as_uint(bw_value(w.s1, scale));
        b.w = __float_as_uint(bw_value(w.s2, scale * scale));
        return b;
    }
};

// level 0: one lane per window of 16 bins, from q
__global__ void __launch_bounds__(256) bwz_level0_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                         const int64_t *__restrict__ pref, const int64_t *__restrict__ wpref, tb_geom G,
                                                         bbi_levels Z, bwz_win *__restrict__ win)
{
    const int64_t Wpad = Z.seg[1] - Z.seg[0], bpc = Wpad / 256;
    const int64_t k = blockIdx.x / bpc, i = ((int64_t)blockIdx.x % bpc) * 256 + threadIdx.x;
    bwz_win w = bwz_win();
    if (i < Z.W[0]) {
        const int64_t r = dgrp_record_of(wpref, G.nrec, i);
        const tb_rec R = recs[r];
        const track_geom g = tb_geom_of(R, G.bin);
        const int64_t wi = R.offset / Z.R[0] + (i - wpref[r]);           // the window's number in the record's coordinates
        int64_t ja = wi * 16 - R.kb0, jb = ja + 16;
        if (ja < 0) ja = 0;
        if (jb > R.nb) jb = R.nb;
        const uint32_t *qr = q + k * G.NBpad + pref[r];
        for (int64_t j = ja; j < jb; ++j) {
            const uint32_t v = qr[j];
            if (v == 0) continue;
            int64_t lo, hi;
            track_bin_span(g, j, lo, hi);
            const uint64_t bases = (uint64_t)(hi - lo);
            if (w.valid == 0) {
                w.start = (uint32_t)lo;
                w.qmin = w.qmax = v;
            }
            w.end = (uint32_t)hi;
            w.valid += (uint32_t)bases;
            w.qmin = v < w.qmin ? v : w.qmin;
            w.qmax = v > w.qmax ? v : w.qmax;
            w.s1 += (uint64_t)v * bases;
            w.s2 += (uint64_t)v * v * bases;
        }
    }
    win[k * Z.seg[BBI_LEVELS] + Z.seg[0] + i] = w;
}

// the totals of every class from its top level (one workgroup per class)
__global__ void __launch_bounds__(256) bwz_totals_kernel(const bwz_win *__restrict__ win, bbi_levels Z, dgrp_track_totals *__restrict__ totals)
{
    __shared__ dgrp_track_totals part[4];
    const bwz_win *top = win + (int64_t)blockIdx.x * Z.seg[BBI_LEVELS] + Z.seg[BBI_LEVELS - 1];
    uint64_t covered = 0, qmin = ~0ull, qmax = 0, s1 = 0, s2 = 0;
    for (int64_t i = threadIdx.x; i < Z.W[BBI_LEVELS - 1]; i += 256) {
        const bwz_win w = top[i];
        if (w.valid == 0) continue;
        covered += w.valid;
        qmin = w.qmin < qmin ? w.qmin : qmin;
        qmax = w.qmax > qmax ? w.qmax : qmax;
        s1 += w.s1;
        s2 += w.s2;
    }
    for (int o = 32; o > 0; o >>= 1) {
        covered += __shfl_xor(covered, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        const uint64_t a = __shfl_xor(qmin, o), b = __shfl_xor(qmax, o);
        qmin = a < qmin ? a : qmin;
        qmax = b > qmax ? b : qmax;
    }
    if ((threadIdx.x & 63) == 0) {
        dgrp_track_totals &p = part[threadIdx.x >> 6];
        p.covered = covered; p.qmin = qmin; p.qmax = qmax; p.sum = s1; p.sumsq = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dgrp_track_totals t = part[0];
        for (int w = 1; w < 4; ++w) {
            t.covered += part[w].covered;
            t.sum += part[w].sum;
            t.sumsq += part[w].sumsq;
            t.qmin = part[w].qmin < t.qmin ? part[w].qmin : t.qmin;
            t.qmax = part[w].qmax > t.qmax ? part[w].qmax : t.qmax;
        }
        if (t.covered == 0) t.qmin = 0;
        totals[blockIdx.x] = t;
    }
}

// ---- the arguments both track entries check, and their workspaces (the shared front's, then their own parts)
static int bw_check(const char *who, const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                    const int64_t *h_startpos, const int *h_cls, int ncls, int digits, int64_t bin, int64_t chrom0)
{
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "%s: bad C %d", who, C);
    DGRP_REQUIRE(ncls >= 1 && ncls <= C, "%s: ncls must lie in 1..C (%d, C = %d)", who, ncls, C);
    DGRP_REQUIRE(h_cls, "%s: NULL h_cls", who);
    DGRP_REQUIRE(nrec >= 0 && nrec < (1ll << 31), "%s: bad nrec %lld", who, (long long)nrec);
    for (int k = 0; k < ncls; ++k) DGRP_REQUIRE(h_cls[k] >= 0 && h_cls[k] < C, "%s: class %d is not in 0..%d", who, h_cls[k], C - 1);
    DGRP_REQUIRE(digits >= 1 && digits <= 4, "%s: digits must lie in 1..4, got %d", who, digits);
    DGRP_REQUIRE(bin >= 1 && bin <= TRACK_MAX_EXTENT, "%s: bad bin %lld", who, (long long)bin);
    DGRP_REQUIRE(chrom0 >= 0 && chrom0 + nrec <= BW_MAX_END, "%s: bad first chromId %lld", who, (long long)chrom0);
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_row0 && h_n && h_startpos, "%s: NULL host table", who);
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_n[r] >= 1 && h_n[r] <= TRACK_MAX_EXTENT, "%s: record %lld: bad n %lld", who, (long long)r, (long long)h_n[r]);
        DGRP_REQUIRE(h_startpos[r] >= 0 && h_startpos[r] <= TRACK_MAX_EXTENT, "%s: record %lld: bad offset %lld", who, (long long)r,
                     (long long)h_startpos[r]);
        DGRP_REQUIRE(h_startpos[r] + h_n[r] <= BW_MAX_END,
                     "%s: record %lld ends at %lld, above 2^32 - 1 = 4294967295, the largest coordinate of a bigWig", who, (long long)r,
                     (long long)(h_startpos[r] + h_n[r]));
        DGRP_REQUIRE(h_row0[r] >= 0, "%s: record %lld: bad first row %lld", who, (long long)r, (long long)h_row0[r]);
    }
    DGRP_REQUIRE(d_probs, "%s: NULL d_probs", who);
    return DGRP_OK;
}

static bool bw_in_range(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos)
{
    if (nrec < 0 || nrec >= (1ll << 31) || (nrec > 0 && (!h_n || !h_startpos))) return false;
    for (int64_t r = 0; r < nrec; ++r)
        if (h_n[r] < 1 || h_startpos[r] < 0 || h_startpos[r] > BW_MAX_END || h_n[r] > BW_MAX_END || h_startpos[r] + h_n[r] > BW_MAX_END)
            return false;
    return true;
}

struct bws_layout { tb_layout t; int64_t cnt, ipref, spref, base, hb, bytes; };

static bool bws_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, bws_layout *l)
{
    if (!bw_in_range(nrec, h_n, h_startpos) || !dgrp_tb_carve(nrec, h_n, h_startpos, bin, ncls, 0, &l->t)) return false;
    int64_t p = l->t.bytes;
    l->cnt = p;
    p += dgrp_align_up(nrec * ncls * 8, 256);
    l->ipref = p;
    p += dgrp_align_up((nrec + 1) * ncls * 8, 256);
    l->spref = p;
    p += dgrp_align_up((nrec + 1) * ncls * 8, 256);
    l->base = p;
    p += dgrp_align_up(2 * (int64_t)(ncls + 1) * 8, 256);
    l->hb = p;
    p += dgrp_align_up(2 * (int64_t)(ncls + 1) * 8, 256);
    l->bytes = p;
    return true;
}

struct bwz_layout { tb_layout t; bbi_levels Z; int64_t wpref, win, tiles, grand, segb, totals, bytes; };

static bool bwz_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, bwz_layout *l)
{
    if (!bw_in_range(nrec, h_n, h_startpos) || bin > (1ll << 32) || !dgrp_tb_carve(nrec, h_n, h_startpos, bin, ncls, 0, &l->t)) return false;
    const bbi_levels &Z = l->Z;
    if (!bbi_levels_of(16 * bin, ncls, nrec, h_startpos, h_n, &l->Z)) return false;
    int64_t p = l->t.bytes;
    l->wpref = p;
    p += dgrp_align_up((nrec + 1) * BBI_LEVELS * 8, 256);
    l->win = p;
    p += dgrp_align_up(Z.seg[BBI_LEVELS] * ncls * (int64_t)sizeof(bwz_win), 256);
    l->tiles = p;
    p += dgrp_align_up(Z.seg[BBI_LEVELS] / 256 * ncls * 8, 256);
    l->grand = p;
    p += 256;
    l->segb = p;
    p += dgrp_align_up(2 * ((int64_t)ncls * BBI_LEVELS + 1) * 8, 256);
    l->totals = p;
    p += dgrp_align_up((int64_t)ncls * (int64_t)sizeof(dgrp_track_totals), 256);
    l->bytes = p;
    return true;
}

// --------------------------------------------------------------------------------------------------------------------- zlib
#define ZLIB_MOD 65521u
#define ZLIB_EMPTY 11                    // 78 01 | 01 00 00 ff ff | 00 00 00 01: the stream of an empty block

// member sizes (0: an empty block, or a row the deflate kernel refused) to stream sizes: a stream is its member without the 18 + 8
// bytes of gzip framing, with 2 + 4 of zlib's; *bad (zeroed) counts the rows that do not lie in the input
__global__ void __launch_bounds__(256) zlib_sizes_kernel(const char *__restrict__ rows, int64_t stride, int64_t nblk, int64_t in_bytes,
                                                         uint64_t *__restrict__ sizes, unsigned long long *__restrict__ bad)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= nblk) return;
    const int64_t *row = reinterpret_cast<const int64_t *>(rows + m * stride);
    const bool ok = row[0] >= 0 && row[1] >= 0 && row[1] <= DGRP_BGZF_BLOCK && row[0] <= in_bytes - row[1];
    if (!ok) atomicAdd(bad, 1ull);
    sizes[m] = sizes[m] == 0 ? ZLIB_EMPTY : sizes[m] - 20;
}

// offs = exclusive scan of the stream sizes with the total at offs[nblk]; workgroup m frames block m.  Nothing is written when the
// whole does not fit out_cap or a row was refused.
__global__ void __launch_bounds__(256) zlib_place_kernel(const uint8_t *__restrict__ in, const char *__restrict__ rows, int64_t stride,
                                                        const uint8_t *__restrict__ slots, const uint64_t *__restrict__ offs, int64_t nblk,
                                                        const unsigned long long *__restrict__ bad, uint8_t *__restrict__ out, int64_t out_cap,
                                                        int64_t *__restrict__ out_sizes)
{
    __shared__ uint32_t sa[4], sb[4];
    if ((int64_t)offs[nblk] > out_cap || *bad != 0) return;
    const int64_t m = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const int64_t *row = reinterpret_cast<const int64_t *>(rows + m * stride);
    const uint8_t *src = in + row[0];
    const uint32_t len = (uint32_t)row[1], size = (uint32_t)(offs[m + 1] - offs[m]);
    uint64_t a = 0, b = 0;
    for (uint32_t i = tid; i < len; i += 256) {
        const uint32_t x = src[i];
        a += x;
        b += (uint64_t)(len - i) * x;
    }
    uint32_t ra = (uint32_t)(a % ZLIB_MOD), rb = (uint32_t)(b % ZLIB_MOD);
    for (int o = 32; o > 0; o >>= 1) {
        ra += __shfl_xor(ra, o);
        rb += __shfl_xor(rb, o);
    }
    if ((tid & 63) == 0) {
        sa[tid >> 6] = ra;
        sb[tid >> 6] = rb;
    }
    __syncthreads();
    uint8_t *dst = out + offs[m];
    if (tid == 0) {
        const uint32_t A = (1u + sa[0] + sa[1] + sa[2] + sa[3]) % ZLIB_MOD;
        const uint32_t B = (len % ZLIB_MOD + sb[0] + sb[1] + sb[2] + sb[3]) % ZLIB_MOD;
        dst[0] = 0x78;
        dst[1] = 0x01;
        dst[size - 4] = (uint8_t)(B >> 8);
        dst[size - 3] = (uint8_t)B;
        dst[size - 2] = (uint8_t)(A >> 8);
        dst[size - 1] = (uint8_t)A;
        if (len == 0) {
            dst[2] = 0x01; dst[3] = 0x00; dst[4] = 0x00; dst[5] = 0xff; dst[6] = 0xff;
        }
        out_sizes[m] = size;
    }
    if (len == 0) return;
    const uint8_t *body = slots + m * DGRP_BGZF_SLOT + 18;
    for (uint32_t i = tid; i < size - 6; i += 256) dst[2 + i] = body[i];
}

static int64_t zlib_workspace(int64_t nblk, int level)
{
    const int64_t base = dgrp_align_up(nblk * DGRP_BGZF_SLOT, 256) + dgrp_align_up((nblk + 2) * 8, 256);
    return level == 0 ? base : base + nblk * DGRP_BGZF_BLOCK * (int64_t)sizeof(uint32_t);
}

}   // namespace

DGRP_EXPORT int64_t dgrp_track_sections_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls)
{
    bws_layout l;
    if (bin < 1 || ncls < 1) return 0;
    return bws_carve(nrec, h_n, h_startpos, bin, ncls, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_sections_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                          const int64_t *h_startpos, const int *h_cls, int ncls, int digits, int64_t bin, int64_t chrom0,
                                          char *d_out, int64_t cap, int64_t *h_class_off, dgrp_track_section *d_table, int64_t table_cap,
                                          int64_t *h_section_off, void *d_work, int64_t work_bytes, void *stream_)
{
    const char *who = "dgrp_track_sections_batch";
    DGRP_REQUIRE(h_class_off && h_section_off, "%s: NULL h_class_off or h_section_off", who);
    if (ncls >= 1 && ncls <= DGRP_MAXC)
        for (int k = 0; k <= ncls; ++k) h_class_off[k] = h_section_off[k] = 0;
    const int rc0 = bw_check(who, d_probs, C, nrec, h_row0, h_n, h_startpos, h_cls, ncls, digits, bin, chrom0);
    if (rc0 != DGRP_OK) return rc0;
    DGRP_REQUIRE(cap >= 0 && table_cap >= 0, "%s: bad cap/table_cap (%lld, %lld)", who, (long long)cap, (long long)table_cap);
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE((d_out || cap == 0) && (d_table || table_cap == 0) && d_work, "%s: NULL pointer", who);
    DGRP_REQUIRE(((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_table & 7) == 0, "%s: d_out must be 4-byte and d_table 8-byte aligned", who);
    bws_layout l;
    DGRP_REQUIRE(bws_carve(nrec, h_n, h_startpos, bin, ncls, &l), "%s: too many bins in one call", who);
    if (work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace %lld < %lld bytes", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *w = (char *)d_work;
    unsigned long long *cnt = (unsigned long long *)(w + l.cnt);
    uint64_t *ipref = (uint64_t *)(w + l.ipref), *spref = (uint64_t *)(w + l.spref), *base = (uint64_t *)(w + l.base);
    uint64_t *hb = (uint64_t *)(w + l.hb);
    std::vector<int64_t> name_off((size_t)nrec + 1, 0);
    std::vector<char> tab;                                                 // (alive until the first synchronisation)
    tb_dev D;
    const int rc = dgrp_tb_bins(d_probs, C, nrec, h_row0, h_n, h_startpos, nullptr, name_off.data(), h_cls, ncls, digits, bin, d_work, l.t,
                                stream, tab, &D);
    if (rc != DGRP_OK) return rc;
    DGRP_HIP(hipMemsetAsync(cnt, 0, (size_t)(nrec * ncls) * 8, stream));
    const dim3 grid((unsigned)D.ntiles), block(256);
    hipLaunchKernelGGL(bw_count_kernel, grid, block, 0, stream, D.q, D.recs, D.pref, D.G, D.tiles, cnt);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), block, 0, stream, D.tiles, D.ntiles, D.grand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bw_prefix_kernel, dim3((unsigned)ncls), block, 0, stream, cnt, nrec, ipref, spref);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bw_bounds_kernel, dim3(1), dim3(64), 0, stream, ipref, spref, nrec, ncls, base, hb);
    DGRP_LAUNCH_CHECK();
    std::vector<uint64_t> off(2 * ((size_t)ncls + 1), 0);
    DGRP_HIP(hipMemcpyAsync(off.data(), hb, off.size() * 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k <= ncls; ++k) {
        h_class_off[k] = (int64_t)off[(size_t)k];
        h_section_off[k] = (int64_t)off[(size_t)(ncls + 1 + k)];
    }
    if (h_class_off[ncls] == 0 || h_class_off[ncls] > cap || h_section_off[ncls] > table_cap) return DGRP_OK;   // (too small: the caller retries)
    double scale = 1.0;
    for (int k = 0; k < digits; ++k) scale *= 10.0;
    hipLaunchKernelGGL(bw_write_kernel, grid, block, 0, stream, D.q, D.recs, D.pref, D.G, scale, D.tiles, cnt, ipref, spref, base, (uint32_t)chrom0,
                       d_out, d_table);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_track_zoom_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls)
{
    bwz_layout l;
    if (bin < 1 || ncls < 1) return 0;
    return bwz_carve(nrec, h_n, h_startpos, bin, ncls, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_zoom_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                      const int64_t *h_startpos, const int *h_cls, int ncls, int digits, int64_t bin, int64_t chrom0,
                                      char *d_out, int64_t cap, int64_t *h_record_off, dgrp_track_zoom_block *d_table, int64_t table_cap,
                                      int64_t *h_block_off, dgrp_track_totals *h_totals, void *d_work, int64_t work_bytes, void *stream_)
{
    const char *who = "dgrp_track_zoom_batch";
    DGRP_REQUIRE(h_record_off && h_block_off && h_totals, "%s: NULL h_record_off, h_block_off or h_totals", who);
    if (ncls >= 1 && ncls <= DGRP_MAXC) {
        for (int s = 0; s <= ncls * BBI_LEVELS; ++s) h_record_off[s] = h_block_off[s] = 0;
        memset(h_totals, 0, (size_t)ncls * sizeof(dgrp_track_totals));
    }
    const int rc0 = bw_check(who, d_probs, C, nrec, h_row0, h_n, h_startpos, h_cls, ncls, digits, bin, chrom0);
    if (rc0 != DGRP_OK) return rc0;
    DGRP_REQUIRE(bin <= (1ll << 32), "%s: bad bin %lld (zoom windows of 16 * bin * 4^9 bases)", who, (long long)bin);
    DGRP_REQUIRE(cap >= 0 && table_cap >= 0, "%s: bad cap/table_cap (%lld, %lld)", who, (long long)cap, (long long)table_cap);
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE((d_out || cap == 0) && (d_table || table_cap == 0) && d_work, "%s: NULL pointer", who);
    DGRP_REQUIRE(((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_table & 7) == 0, "%s: d_out must be 16-byte and d_table 8-byte aligned", who);
    bwz_layout l;
    DGRP_REQUIRE(bwz_carve(nrec, h_n, h_startpos, bin, ncls, &l), "%s: too many bins in one call", who);
    if (work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace %lld < %lld bytes", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *w = (char *)d_work;
    const bbi_levels &Z = l.Z;
    int64_t *d_wpref = (int64_t *)(w + l.wpref);
    bwz_win *win = (bwz_win *)(w + l.win);
    uint64_t *tiles = (uint64_t *)(w + l.tiles), *grand = (uint64_t *)(w + l.grand), *segb = (uint64_t *)(w + l.segb);
    dgrp_track_totals *d_totals = (dgrp_track_totals *)(w + l.totals);
    const int nseg = ncls * BBI_LEVELS;
    const std::vector<int64_t> wpref = bbi_wpref(Z, nrec, h_startpos, h_n);
    DGRP_HIP(hipMemcpyAsync(d_wpref, wpref.data(), wpref.size() * 8, hipMemcpyHostToDevice, stream));
    std::vector<int64_t> name_off((size_t)nrec + 1, 0);
    std::vector<char> tab;                                                 // (alive until the first synchronisation)
    tb_dev D;
    const int rc = dgrp_tb_bins(d_probs, C, nrec, h_row0, h_n, h_startpos, nullptr, name_off.data(), h_cls, ncls, digits, bin, d_work, l.t,
                                stream, tab, &D);
    if (rc != DGRP_OK) return rc;
    const dim3 block(256);
    hipLaunchKernelGGL(bwz_level0_kernel, dim3((unsigned)((Z.seg[1] - Z.seg[0]) / 256 * ncls)), block, 0, stream, D.q, D.recs, D.pref, d_wpref,
                       D.G, Z, win);
    DGRP_LAUNCH_CHECK();
    for (int k = 1; k < BBI_LEVELS; ++k) {
        hipLaunchKernelGGL((bbi_reduce_kernel<bwz_win, bwz_start>), dim3((unsigned)((Z.seg[k + 1] - Z.seg[k]) / 256 * ncls)), block, 0, stream,
                           bwz_start{D.recs}, d_wpref, nrec, Z, k, win);
        DGRP_LAUNCH_CHECK();
    }
    const int64_t ntiles = Z.seg[BBI_LEVELS] / 256 * ncls;
    hipLaunchKernelGGL(bbi_count_kernel<bwz_win>, dim3((unsigned)ntiles), block, 0, stream, win, tiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), block, 0, stream, tiles, ntiles, grand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL((bbi_bounds_kernel<bwz_win, false>), dim3(1), dim3(64), 0, stream, win, tiles, grand, Z, ncls, segb, nullptr);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bwz_totals_kernel, dim3((unsigned)ncls), block, 0, stream, win, Z, d_totals);
    DGRP_LAUNCH_CHECK();
    std::vector<uint64_t> off(2 * ((size_t)nseg + 1), 0);
    DGRP_HIP(hipMemcpyAsync(off.data(), segb, off.size() * 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipMemcpyAsync(h_totals, d_totals, (size_t)ncls * sizeof(dgrp_track_totals), hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int s = 0; s <= nseg; ++s) {
        h_record_off[s] = (int64_t)off[(size_t)s];
        h_block_off[s] = (int64_t)off[(size_t)(nseg + 1 + s)];
    }
    if (h_record_off[nseg] == 0 || 32 * h_record_off[nseg] > cap || h_block_off[nseg] > table_cap) return DGRP_OK;   // (the caller retries)
    double scale = 1.0;
    for (int k = 0; k < digits; ++k) scale *= 10.0;
    hipLaunchKernelGGL((bbi_write_kernel<bwz_win, bwz_tail>), dim3((unsigned)ntiles), block, 0, stream, win, d_wpref, nrec, Z, bwz_tail{scale}, tiles,
                       segb, ncls, (uint32_t)chrom0, (uint4 *)d_out, d_table);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_zlib_bound(int64_t nblk, int64_t in_bytes) { return nblk < 0 || in_bytes < 0 ? 0 : in_bytes + ZLIB_EMPTY * nblk; }

DGRP_EXPORT int64_t dgrp_zlib_workspace_bytes(int64_t nblk, int level)
{
    return nblk < 0 || nblk > INT32_MAX - 1 || level < 0 || level > 1 ? 0 : zlib_workspace(nblk, level);
}

DGRP_EXPORT int dgrp_zlib_compress_batch(const uint8_t *d_in, int64_t in_bytes, const void *d_rows, int64_t stride, int64_t nblk, int level,
                                         uint8_t *d_out, int64_t out_cap, int64_t *d_sizes, int64_t *h_out_bytes, void *d_work,
                                         int64_t work_bytes, void *stream_)
{
    const char *who = "dgrp_zlib_compress_batch";
    DGRP_REQUIRE(h_out_bytes, "%s: NULL h_out_bytes", who);
    *h_out_bytes = 0;
    DGRP_REQUIRE(in_bytes >= 0 && nblk >= 0 && nblk <= INT32_MAX - 1 && out_cap >= 0 && work_bytes >= 0, "%s: bad arguments", who);
    DGRP_REQUIRE(stride >= 16 && stride % 8 == 0, "%s: a row is at least an int64 offset and an int64 length (stride %lld)", who,
                 (long long)stride);
    DGRP_REQUIRE(level == 0 || level == 1, "%s: level %d (0: literals, 1: matches)", who, level);
    if (nblk == 0) return DGRP_OK;
    DGRP_REQUIRE((d_in || in_bytes == 0) && d_rows && (d_out || out_cap == 0) && d_sizes && d_work, "%s: NULL pointer", who);
    DGRP_REQUIRE(((uintptr_t)d_work & 15) == 0 && ((uintptr_t)d_rows & 7) == 0, "%s: d_work must be 16-byte, d_rows 8-byte aligned", who);
    if (work_bytes < zlib_workspace(nblk, level)) {
        dgrp_set_error("%s: workspace too small", who);
        return DGRP_ENOMEM;
    }
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t *slots = (uint8_t *)d_work;
    uint64_t *sizes = (uint64_t *)(slots + dgrp_align_up(nblk * DGRP_BGZF_SLOT, 256));
    uint32_t *lz = level == 0 ? nullptr : (uint32_t *)((uint8_t *)sizes + dgrp_align_up((nblk + 2) * 8, 256));
    unsigned long long *bad = (unsigned long long *)(sizes + nblk + 1);
    const char *rows = (const char *)d_rows;
    DGRP_HIP(hipMemsetAsync(bad, 0, 8, stream));
    const int rc = dgrp_deflate_members(d_in, in_bytes, rows, stride, nblk, level, slots, sizes, lz, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(zlib_sizes_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, stream, rows, stride, nblk, in_bytes, sizes, bad);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, sizes, nblk, sizes + nblk);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(zlib_place_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, d_in, rows, stride, slots, sizes, nblk, bad, d_out, out_cap,
                       d_sizes);
    DGRP_LAUNCH_CHECK();
    uint64_t tail[2] = {0, 0};                                             // the total, the refused rows
    DGRP_HIP(hipMemcpyAsync(tail, sizes + nblk, 16, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    DGRP_REQUIRE(tail[1] == 0, "%s: %llu rows do not lie in the input or are longer than 65280 bytes (nothing written)", who,
                 (unsigned long long)tail[1]);
    *h_out_bytes = (int64_t)tail[0];
    if (*h_out_bytes > out_cap) {
        dgrp_set_error("%s: output of %lld bytes, %lld needed (nothing written)", who, (long long)out_cap, (long long)*h_out_bytes);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_zlib_compress_host(const uint8_t *h_in, int64_t in_bytes, const void *h_rows, int64_t stride, int64_t nblk, int level,
                                        uint8_t *h_out, int64_t out_cap, int64_t *h_sizes, int64_t *h_out_bytes)
{
    const char *who = "dgrp_zlib_compress_host";
    DGRP_REQUIRE(h_out_bytes, "%s: NULL h_out_bytes", who);
    *h_out_bytes = 0;
    DGRP_REQUIRE(in_bytes >= 0 && nblk >= 0 && out_cap >= 0, "%s: bad arguments", who);
    DGRP_REQUIRE(stride >= 16 && stride % 8 == 0, "%s: a row is at least an int64 offset and an int64 length (stride %lld)", who,
                 (long long)stride);
    DGRP_REQUIRE(level == 0 || level == 1, "%s: level %d (0: literals, 1: matches)", who, level);
    if (nblk == 0) return DGRP_OK;
    DGRP_REQUIRE((h_in || in_bytes == 0) && h_rows && (h_out || out_cap == 0) && h_sizes, "%s: NULL pointer", who);
    for (int64_t m = 0; m < nblk; ++m) {
        const int64_t *row = (const int64_t *)((const char *)h_rows + m * stride);
        DGRP_REQUIRE(row[0] >= 0 && row[1] >= 0 && row[1] <= DGRP_BGZF_BLOCK && row[0] <= in_bytes - row[1],
                     "%s: row %lld (offset %lld, %lld bytes) does not lie in the input or is longer than 65280 bytes", who, (long long)m,
                     (long long)row[0], (long long)row[1]);
    }
    std::vector<uint32_t> slot(DGRP_BGZF_SLOT / 4), lz(level ? DGRP_BGZF_BLOCK : 0);
    std::vector<uint16_t> head(level ? 1 << DGRP_LZ_HASH_BITS : 0);
    dgrp_deflate_plan plan;
    dgrp_lz_plan lzplan;
    int64_t pos = 0;
    bool fits = true;                                                      // once a stream does not fit nothing more is written, only counted
    for (int64_t m = 0; m < nblk; ++m) {
        const int64_t *row = (const int64_t *)((const char *)h_rows + m * stride);
        const uint8_t *src = h_in + row[0];
        const uint32_t len = (uint32_t)row[1];
        uint32_t size = ZLIB_EMPTY;
        if (len > 0)
            size = (level ? dgrp_bgzf_member_serial_lz(src, len, slot.data(), &plan, &lzplan, lz.data(), head.data())
                          : dgrp_bgzf_member_serial(src, len, slot.data(), &plan)) - 20;
        uint32_t a = 1, b = 0;
        for (uint32_t i = 0; i < len; ++i) {
            a = (a + src[i]) % ZLIB_MOD;
            b = (b + a) % ZLIB_MOD;
        }
        fits = fits && pos + size <= out_cap;
        if (fits) {
            uint8_t *dst = h_out + pos;
            dst[0] = 0x78;
            dst[1] = 0x01;
            if (len == 0) {
                dst[2] = 0x01; dst[3] = 0x00; dst[4] = 0x00; dst[5] = 0xff; dst[6] = 0xff;
            } else {
                memcpy(dst + 2, (const uint8_t *)slot.data() + 18, size - 6);
            }
            dst[size - 4] = (uint8_t)(b >> 8); dst[size - 3] = (uint8_t)b; dst[size - 2] = (uint8_t)(a >> 8); dst[size - 1] = (uint8_t)a;
        }
        h_sizes[m] = size;
        pos += size;
    }
    *h_out_bytes = pos;
    if (!fits) {
        dgrp_set_error("%s: output of %lld bytes, %lld needed", who, (long long)out_cap, (long long)pos);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}
