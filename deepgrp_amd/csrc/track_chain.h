// What the chains over the probability tracks share (track_kernels.hip: text and tabix index; bigwig_kernels.hip: bigWig sections and
// zoom summaries): the record table, the flat bin space [class k][record r][bin j] with every class at a tile boundary, the
// workspace layout of its front, and the bin pass that fills q -- defined in track_kernels.hip, one copy in the library.
// Not here: the record of a flat bin (dgrp_record_of, dgrp_common.h: the search every prefix table of the library uses) and the
// zoom ladder above bigWig's level 0 (bbi_zoom.h, shared with bigBed).
#pragma once
#include "dgrp_common.h"
#include <vector>

struct track_geom {
    int64_t offset, n, bin;       // span [offset, offset + n) in record coordinates, bin width
    int64_t kb0, nb;              // first bin (offset / bin), bins touching the span
};

// the coordinates [lo, hi) of bin j, clipped to the span
static __device__ __forceinline__ void track_bin_span(const track_geom &g, int64_t j, int64_t &lo, int64_t &hi)
{
    const int64_t a = (g.kb0 + j) * g.bin, b = a + g.bin;
    lo = a > g.offset ? a : g.offset;
    hi = b < g.offset + g.n ? b : g.offset + g.n;
}

#define TRACK_TILE 2048                  // bins per workgroup: 8 rounds of 256 consecutive bins

struct tb_rec { int64_t row0, n, offset, kb0, nb, name_off, name_len, pad; };     // one record: 64 bytes of the uploaded table
struct tb_geom {
    int64_t nrec, NB, NBpad, bin;        // records, bins of all records, the same rounded up to TRACK_TILE, bin width
    int C, ncls, digits;
};

// The record of flat bin f < pref[nrec] is dgrp_record_of(pref, nrec, f) (every record has at least one bin).  The same for
// f >= f0 when r0 is the record of f0 (found once per tile): mostly r0 itself, else one of the next f - f0 records
static __device__ __forceinline__ int64_t tb_record_from(const int64_t *__restrict__ pref, int64_t nrec, int64_t r0, int64_t f0, int64_t f)
{
    if (pref[r0 + 1] > f) return r0;
    int64_t lo = r0 + 1, hi = r0 + (f - f0) + 1;
    if (hi > nrec) hi = nrec;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pref[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

static __device__ __forceinline__ track_geom tb_geom_of(const tb_rec &R, int64_t bin)
{
    track_geom g;
    g.offset = R.offset; g.n = R.n; g.bin = bin; g.kb0 = R.kb0; g.nb = R.nb;
    return g;
}

// byte offsets of the workspace's parts (recs .. names within the uploaded tables); NB = the bins per class it has room for
struct tb_layout { int64_t NB, NBpad, tables, tables_bytes, recs, pref, cls, names, q, tiles, bytes; };

#define TRACK_MAX_EXTENT (1ll << 40)     // n, offset and bin: far beyond any genome; no product overflows

// what the front half of the chain leaves on the device for the pass that follows it
struct tb_dev {
    uint64_t *grand, *bounds;            // the text's total, its class boundaries [ncls + 1]
    const tb_rec *recs;
    const int64_t *pref;
    const int *cls;
    const char *names;
    uint32_t *q;
    uint64_t *tiles;                     // scanned: the text offset of every tile
    tb_geom G;
    uint32_t qmax;
    int64_t tpc, ntiles;                 // tiles per class, tiles
};

// the workspace for the bins of the given records; false: arguments the entries refuse
bool dgrp_tb_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, int64_t names_bytes, tb_layout *l);

// On checked arguments and a workspace carved as `l`: one upload of the tables (from `tab`, which the caller keeps until its next
// synchronisation) and the bin pass (q of every class), on the stream, without a synchronisation.  D->tiles is room for one uint64
// per tile, left unset.
int dgrp_tb_bins(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n, const int64_t *h_startpos,
                 const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits, int64_t bin, void *d_work,
                 const tb_layout &l, hipStream_t stream, std::vector<char> &tab, tb_dev *D);
