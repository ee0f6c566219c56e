// Probability tracks (predict --track_dir): class columns of merged probabilities [rows, C] as 4-column bedGraph text, built in HBM.
// Three passes: bin max + quantisation (reads the strided columns), bytes of text per tile of bins, and the text itself; between
// them one scan of the tile sums.  Every index and byte offset is 64-bit.
// One chain writes any number of records and classes (dgrp_track_text_batch): a file of thousands of short records costs a handful
// of launches and two synchronisations instead of that per record and class.  One class of one record (dgrp_track_text) is the same
// chain with one record and one class.  The flat bin space is [class k][record r][bin j]; every class starts at a tile boundary
// (NBpad = bins of all records rounded up to TRACK_TILE), so no tile straddles a class and the scanned tile offsets at each
// class's first tile are the class boundaries of the text.
// See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "scan.h"
#include "tabix_bins.h"
#include "track_chain.h"
#include <string.h>
#include <vector>

namespace {

#define TRACK_WAVE_BIN 64         // bins wider than this are reduced by a whole wave, narrower ones by one lane

// floor(v * 10^D + 0.5) as two float32 roundings (this file is compiled with -ffp-contract=off), clamped to [0, 10^D]
__device__ __forceinline__ uint32_t track_quantise(float v, float scale, uint32_t qmax)
{
    const float t = v * scale;
    const float q = floorf(t + 0.5f);
    return q <= 0.0f ? 0u : q >= (float)qmax ? qmax : (uint32_t)q;
}

__device__ __forceinline__ int track_decimal_width(uint64_t v)
{
    int w = 1;
    for (uint64_t p = 10; w < 19 && v >= p; p *= 10) ++w;
    return w;
}

__device__ __forceinline__ void track_put_decimal(char *o, uint64_t v, int w)
{
    if (v <= 0xffffffffu) {                      // (32-bit division where it suffices: every coordinate below 4.29 Gbp)
        uint32_t u = (uint32_t)v;
        for (int k = w - 1; k >= 0; --k) { o[k] = (char)('0' + u % 10); u /= 10; }
        return;
    }
    for (int k = w - 1; k >= 0; --k) {
        o[k] = (char)('0' + v % 10);
        v /= 10;
    }
}

#define TRACK_STAGE 32768                // bytes of one round's text that are assembled in LDS (longer rounds write directly)

#define TB_CLS 8                         // classes reduced side by side from one read of a row (more classes: one more pass per 8)

// one lane per (record, bin), bins up to TRACK_WAVE_BIN wide: every row is read once for up to TB_CLS selected classes
__global__ void __launch_bounds__(256) tb_bin_lane_kernel(const float *__restrict__ probs, const tb_rec *__restrict__ recs,
                                                          const int64_t *__restrict__ pref, const int *__restrict__ cls, tb_geom G,
                                                          float scale, uint32_t qmax, uint32_t *__restrict__ q)
{
    __shared__ int64_t s_r0;
    const int64_t f0 = (int64_t)blockIdx.x * 256, f = f0 + threadIdx.x;
    if (threadIdx.x == 0) s_r0 = dgrp_record_of(pref, G.nrec, f0);
    __syncthreads();
    if (f >= G.NB) return;
    const int64_t r = tb_record_from(pref, G.nrec, s_r0, f0, f);
    const tb_rec R = recs[r];
    int64_t lo, hi;
    track_bin_span(tb_geom_of(R, G.bin), f - pref[r], lo, hi);
    const float *p = probs + (R.row0 + (lo - R.offset)) * G.C;
    const int rows = (int)(hi - lo);
    for (int k0 = 0; k0 < G.ncls; k0 += TB_CLS) {
        float m[TB_CLS];
        int c[TB_CLS];
#pragma unroll
        for (int k = 0; k < TB_CLS; ++k) {
            m[k] = 0.0f;
            c[k] = k0 + k < G.ncls ? cls[k0 + k] : 0;
        }
        for (int i = 0; i < rows; ++i) {
            const float *row = p + (int64_t)i * G.C;
#pragma unroll
            for (int k = 0; k < TB_CLS; ++k)
                if (k0 + k < G.ncls) m[k] = fmaxf(m[k], row[c[k]]);
        }
#pragma unroll
        for (int k = 0; k < TB_CLS; ++k)
            if (k0 + k < G.ncls) q[(int64_t)(k0 + k) * G.NBpad + f] = track_quantise(m[k], scale, qmax);
    }
}

// one wave per (record, bin): wider bins
__global__ void __launch_bounds__(256) tb_bin_wave_kernel(const float *__restrict__ probs, const tb_rec *__restrict__ recs,
                                                          const int64_t *__restrict__ pref, const int *__restrict__ cls, tb_geom G,
                                                          float scale, uint32_t qmax, uint32_t *__restrict__ q)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t f = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); f < G.NB; f += waves) {
        const int64_t r = dgrp_record_of(pref, G.nrec, f);
        const tb_rec R = recs[r];
        int64_t lo, hi;
        track_bin_span(tb_geom_of(R, G.bin), f - pref[r], lo, hi);
        const float *p = probs + (R.row0 + (lo - R.offset)) * G.C;
        const int64_t rows = hi - lo;
        for (int k0 = 0; k0 < G.ncls; k0 += TB_CLS) {
            float m[TB_CLS];
            int c[TB_CLS];
#pragma unroll
            for (int k = 0; k < TB_CLS; ++k) {
                m[k] = 0.0f;
                c[k] = k0 + k < G.ncls ? cls[k0 + k] : 0;
            }
            for (int64_t i = lane; i < rows; i += 64) {
                const float *row = p + i * G.C;
#pragma unroll
                for (int k = 0; k < TB_CLS; ++k)
                    if (k0 + k < G.ncls) m[k] = fmaxf(m[k], row[c[k]]);
            }
#pragma unroll
            for (int k = 0; k < TB_CLS; ++k) {
                if (k0 + k >= G.ncls) continue;                      // (uniform)
                float v = m[k];
                for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
                if (lane == 0) q[(int64_t)(k0 + k) * G.NBpad + f] = track_quantise(v, scale, qmax);
            }
        }
    }
}

// A line "name\tstart\tend\tv.vv\n" is written in two parts: the bin where its run starts writes "name\tstart\t", the bin where it
// ends writes "end\tv.vv\n" (one bin may do both).  The exclusive prefix sum of the parts' bytes over the bins is then where each
// part goes: no per-run arrays.
struct track_part { uint32_t v; bool first, last; int64_t lo, hi; int64_t head, tail; };

// the parts of flat bin f of one class (qk = that class's NBpad values): a run never leaves its record, bin 0 of a record is
// always `first` and its last bin always `last`.  Bins in [NB, NBpad) read as q = 0.
struct tb_part { track_part p; int64_t name_off, name_len; };

__device__ __forceinline__ tb_part tb_part_of(const uint32_t *__restrict__ qk, const tb_rec *__restrict__ recs,
                                              const int64_t *__restrict__ pref, const tb_geom &G, int64_t r0, int64_t f0, int64_t f)
{
    tb_part t;
    t.p.v = f < G.NB ? qk[f] : 0u;
    t.p.first = t.p.last = false;
    t.p.head = t.p.tail = 0;
    t.p.lo = t.p.hi = 0;
    t.name_off = t.name_len = 0;
    if (t.p.v == 0) return t;
    const int64_t r = tb_record_from(pref, G.nrec, r0, f0, f);
    const int64_t j = f - pref[r], nb = recs[r].nb;
    t.p.first = j == 0 || qk[f - 1] != t.p.v;
    t.p.last = j == nb - 1 || qk[f + 1] != t.p.v;
    if (!t.p.first && !t.p.last) return t;
    const tb_rec R = recs[r];
    track_bin_span(tb_geom_of(R, G.bin), j, t.p.lo, t.p.hi);
    t.name_off = R.name_off;
    t.name_len = R.name_len;
    if (t.p.first) t.p.head = R.name_len + track_decimal_width((uint64_t)t.p.lo) + 2;
    if (t.p.last) t.p.tail = track_decimal_width((uint64_t)t.p.hi) + G.digits + 4;
    return t;
}

// bytes of text per tile; tile t belongs to class t / (NBpad / TRACK_TILE)
__global__ void __launch_bounds__(256) tb_count_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                       const int64_t *__restrict__ pref, tb_geom G, uint64_t *__restrict__ tilebytes)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_r0;
    const int64_t tpc = G.NBpad / TRACK_TILE;
    const int64_t k = blockIdx.x / tpc, f0 = ((int64_t)blockIdx.x % tpc) * TRACK_TILE;
    if (threadIdx.x == 0) s_r0 = dgrp_record_of(pref, G.nrec, f0);
    __syncthreads();
    const int64_t r0 = s_r0;
    const uint32_t *qk = q + k * G.NBpad;
    uint64_t s = 0;
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const tb_part t = tb_part_of(qk, recs, pref, G, r0, f0, f0 + r * 256 + threadIdx.x);
        s += (uint64_t)(t.p.head + t.p.tail);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tilebytes[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// the class boundaries of the text, side by side for one copy to the host: the scanned offset of each class's first tile, the total
__global__ void __launch_bounds__(128) tb_bounds_kernel(const uint64_t *__restrict__ tileoff, int64_t tpc, int ncls,
                                                       const uint64_t *__restrict__ grand, uint64_t *__restrict__ bounds)
{
    const int k = threadIdx.x;
    if (k < ncls) bounds[k] = tileoff[(int64_t)k * tpc];
    if (k == ncls) bounds[k] = *grand;
}

// the parts of one bin at o (LDS image or d_text); the name comes from the uploaded blob
__device__ __forceinline__ void tb_emit(char *o, const tb_part &t, const char *__restrict__ names, int digits, uint32_t qmax)
{
    if (t.p.first) {
        const char *nm = names + t.name_off;
        for (int64_t c = 0; c < t.name_len; ++c) o[c] = nm[c];
        o += t.name_len;
        *o++ = '\t';
        const int w = track_decimal_width((uint64_t)t.p.lo);
        track_put_decimal(o, (uint64_t)t.p.lo, w);
        o += w;
        *o++ = '\t';
    }
    if (t.p.last) {
        const int w = track_decimal_width((uint64_t)t.p.hi);
        track_put_decimal(o, (uint64_t)t.p.hi, w);
        o += w;
        *o++ = '\t';
        *o++ = (char)('0' + t.p.v / qmax);
        *o++ = '.';
        track_put_decimal(o, t.p.v % qmax, digits);
        o += digits;
        *o = '\n';
    }
}

// The text, in 8 rounds of 256 consecutive bins per tile.  A round of up to TRACK_STAGE bytes is assembled in LDS, laid out congruent
// to its global address modulo 16, and flushed with aligned 16-byte stores: only words that lie wholly inside the round's byte range
// go out wide, the bytes at its two edges as byte stores, so no word is shared between rounds or tiles and no byte is written
// twice.  A longer round (long names) writes directly; the choice is uniform, the round's total comes from the block scan.
__global__ void __launch_bounds__(256) tb_write_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                       const int64_t *__restrict__ pref, const char *__restrict__ names, tb_geom G,
                                                       uint32_t qmax, const uint64_t *__restrict__ tileoff, char *text)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_r0;
    __shared__ __attribute__((aligned(16))) char stage[TRACK_STAGE + 16];
    const int64_t tpc = G.NBpad / TRACK_TILE;
    const int64_t k = blockIdx.x / tpc, f0 = ((int64_t)blockIdx.x % tpc) * TRACK_TILE;
    if (threadIdx.x == 0) s_r0 = dgrp_record_of(pref, G.nrec, f0);
    __syncthreads();
    const int64_t r0 = s_r0;
    const uint32_t *qk = q + k * G.NBpad;
    int64_t at = (int64_t)tileoff[blockIdx.x];
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const tb_part t = tb_part_of(qk, recs, pref, G, r0, f0, f0 + r * 256 + threadIdx.x);
        uint64_t round_bytes;
        const int64_t ex = (int64_t)block_exclusive_scan((uint64_t)(t.p.head + t.p.tail), &round_bytes, lds);
        if (round_bytes == 0) continue;                                    // (uniform)
        if (round_bytes > TRACK_STAGE) {
            tb_emit(text + at + ex, t, names, G.digits, qmax);
        } else {
            const int64_t mis = (int64_t)((uintptr_t)(text + at) & 15);
            tb_emit(stage + mis + ex, t, names, G.digits, qmax);
            __syncthreads();
            char *dst = text + at - mis;                                   // the 16-byte aligned address of stage[0]
            const int64_t b0 = mis, b1 = mis + (int64_t)round_bytes;       // the round's bytes in the image
            const int64_t w0 = (b0 + 15) & ~(int64_t)15, w1 = b1 & ~(int64_t)15;
            const int64_t h1 = w0 < b1 ? w0 : b1;
            for (int64_t i = b0 + threadIdx.x; i < h1; i += 256) dst[i] = stage[i];
            for (int64_t i = w0 + 16 * (int64_t)threadIdx.x; i < w1; i += 16 * 256)
                *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(stage + i);
            for (int64_t i = (w1 > h1 ? w1 : h1) + threadIdx.x; i < b1; i += 256) dst[i] = stage[i];
            __syncthreads();
        }
        at += (int64_t)round_bytes;
    }
}

// the workspace with room for NB bins per class; false: more bins than the grids take (2^39)
static bool tb_carve_bins(int64_t nrec, int64_t NB, int ncls, int64_t names_bytes, tb_layout *l)
{
    l->NB = NB;
    l->NBpad = dgrp_align_up(NB, TRACK_TILE);
    if (l->NBpad / TRACK_TILE * ncls >= (1ll << 31) || (NB + 255) / 256 >= (1ll << 31)) return false;
    // the uploaded tables: records | bin prefix | classes | names
    l->recs = 0;
    l->pref = l->recs + nrec * (int64_t)sizeof(tb_rec);
    l->cls = l->pref + (nrec + 1) * 8;
    l->names = l->cls + dgrp_align_up((int64_t)ncls * 4, 8);
    l->tables_bytes = l->names + names_bytes;
    int64_t p = 256 + dgrp_align_up((int64_t)(ncls + 1) * 8, 256);        // total, class boundaries
    l->tables = p;
    p += dgrp_align_up(l->tables_bytes, 256);
    l->q = p;
    p += dgrp_align_up(l->NBpad * ncls * 4, 256);
    l->tiles = p;
    p += dgrp_align_up(l->NBpad / TRACK_TILE * ncls * 8, 256);
    l->bytes = p;
    return true;
}

// the same for the bins of the given records; false: arguments the entry refuses
static bool tb_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, int64_t names_bytes,
                     tb_layout *l)
{
    if (nrec < 0 || bin < 1 || bin > TRACK_MAX_EXTENT || ncls < 1 || ncls > DGRP_MAXC || names_bytes < 0) return false;
    if (nrec > 0 && (!h_n || !h_startpos)) return false;
    int64_t NB = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        if (h_n[r] < 1 || h_n[r] > TRACK_MAX_EXTENT || h_startpos[r] < 0 || h_startpos[r] > TRACK_MAX_EXTENT) return false;
        NB += (h_startpos[r] + h_n[r] - 1) / bin - h_startpos[r] / bin + 1;
        if (NB > 4 * TRACK_MAX_EXTENT) return false;
    }
    return tb_carve_bins(nrec, NB, ncls, names_bytes, l);
}

// The shared start of every chain on checked arguments and a workspace carved as `l`: one upload of the tables (`tab`, which the
// caller keeps until its next synchronisation) and the bin pass.  No synchronisation.
static int tb_bins(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n, const int64_t *h_startpos,
                   const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits, int64_t bin, void *d_work,
                   const tb_layout &l, hipStream_t stream, std::vector<char> &tab, tb_dev *D)
{
    const int64_t names_bytes = h_name_off[nrec];
    tab.assign((size_t)(l.names + names_bytes), 0);
    tb_rec *recs = (tb_rec *)(tab.data() + l.recs);
    int64_t *pref = (int64_t *)(tab.data() + l.pref);
    pref[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        tb_rec &R = recs[r];
        R.row0 = h_row0[r]; R.n = h_n[r]; R.offset = h_startpos[r];
        R.kb0 = R.offset / bin;
        R.nb = (R.offset + R.n - 1) / bin - R.kb0 + 1;
        R.name_off = h_name_off[r]; R.name_len = h_name_off[r + 1] - h_name_off[r]; R.pad = 0;
        pref[r + 1] = pref[r] + R.nb;
    }
    memcpy(tab.data() + l.cls, h_cls, (size_t)ncls * 4);
    if (names_bytes > 0) memcpy(tab.data() + l.names, names, (size_t)names_bytes);
    char *w = (char *)d_work;
    DGRP_HIP(hipMemcpyAsync(w + l.tables, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
    uint64_t *grand = (uint64_t *)w, *bounds = (uint64_t *)(w + 256);
    const tb_rec *d_recs = (const tb_rec *)(w + l.tables + l.recs);
    const int64_t *d_pref = (const int64_t *)(w + l.tables + l.pref);
    const int *d_cls = (const int *)(w + l.tables + l.cls);
    uint32_t *q = (uint32_t *)(w + l.q);
    uint64_t *tiles = (uint64_t *)(w + l.tiles);
    tb_geom G;
    G.nrec = nrec; G.NB = pref[nrec]; G.NBpad = l.NBpad; G.bin = bin; G.C = C; G.ncls = ncls; G.digits = digits;
    uint32_t qmax = 1;
    for (int k = 0; k < digits; ++k) qmax *= 10;
    const float scale = (float)qmax;
    const int64_t tpc = l.NBpad / TRACK_TILE, ntiles = tpc * ncls;

    if (bin <= TRACK_WAVE_BIN) {
        hipLaunchKernelGGL(tb_bin_lane_kernel, dim3((unsigned)((G.NB + 255) / 256)), dim3(256), 0, stream, d_probs, d_recs, d_pref, d_cls, G,
                           scale, qmax, q);
    } else {
        hipLaunchKernelGGL(tb_bin_wave_kernel, dim3(grid_for(G.NB * 64, 256)), dim3(256), 0, stream, d_probs, d_recs, d_pref, d_cls, G,
                           scale, qmax, q);
    }
    DGRP_LAUNCH_CHECK();
    D->grand = grand; D->bounds = bounds; D->recs = d_recs; D->pref = d_pref; D->cls = d_cls; D->names = w + l.tables + l.names;
    D->q = q; D->tiles = tiles; D->G = G; D->qmax = qmax; D->tpc = tpc; D->ntiles = ntiles;
    return DGRP_OK;
}

// The front half of every text chain on checked arguments and a workspace carved as `l` (room for at least the records' bins and
// names): one upload of the tables, bin pass, count, scan, the class boundaries to h_class_off (one synchronisation).
static int tb_front(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n, const int64_t *h_startpos,
                    const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits, int64_t bin,
                    int64_t *h_class_off, void *d_work, const tb_layout &l, hipStream_t stream, tb_dev *D)
{
    std::vector<char> tab;                                                 // (alive until the synchronisation below)
    const int rc = tb_bins(d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin, d_work, l, stream, tab, D);
    if (rc != DGRP_OK) return rc;
    const tb_rec *d_recs = D->recs;
    const int64_t *d_pref = D->pref;
    uint32_t *q = D->q;
    uint64_t *tiles = D->tiles, *grand = D->grand, *bounds = D->bounds;
    const tb_geom G = D->G;
    const int64_t tpc = D->tpc, ntiles = D->ntiles;
    hipLaunchKernelGGL(tb_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, q, d_recs, d_pref, G, tiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, tiles, ntiles, grand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(tb_bounds_kernel, dim3(1), dim3(128), 0, stream, tiles, tpc, ncls, grand, bounds);
    DGRP_LAUNCH_CHECK();
    std::vector<uint64_t> off((size_t)ncls + 1, 0);
    DGRP_HIP(hipMemcpyAsync(off.data(), bounds, off.size() * 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k <= ncls; ++k) h_class_off[k] = (int64_t)off[(size_t)k];
    return DGRP_OK;
}

// The text chain of both text entries: the front half (first synchronisation) and, if the text fits cap, the write pass (second
// synchronisation).
static int tb_run(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n, const int64_t *h_startpos,
                  const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits, int64_t bin, char *d_text,
                  int64_t cap, int64_t *h_class_off, void *d_work, const tb_layout &l, hipStream_t stream)
{
    tb_dev D;
    const int rc = tb_front(d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin, h_class_off, d_work, l,
                            stream, &D);
    if (rc != DGRP_OK) return rc;
    const int64_t total = h_class_off[ncls];
    if (total == 0 || total > cap) return DGRP_OK;                          // (too small: the caller retries with room for all of it)
    hipLaunchKernelGGL(tb_write_kernel, dim3((unsigned)D.ntiles), dim3(256), 0, stream, D.q, D.recs, D.pref, D.names, D.G, D.qmax, D.tiles,
                       d_text);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}

// one record, whatever its offset, has at most n / bin + 2 bins
static bool track_carve_one(int64_t n, int64_t bin, tb_layout *l)
{
    if (n < 0 || n > TRACK_MAX_EXTENT || bin < 1 || bin > TRACK_MAX_EXTENT) return false;
    return tb_carve_bins(1, n / bin + 2, 1, DGRP_TRACK_NAME_ROOM, l);
}

// ---- tabix index of the text (dgrp_track_index_batch): the chunks of hts_idx_push and the 16 kb linear index, in offsets of the text
// the text entry would write.  A line exists only as its `first` and its `last` bin, possibly tiles apart, so what a line needs of
// itself and of the line in front of it comes from one forward scan: the two latest `first` positions and the two latest `last`
// positions at or in front of every bin (firsts and lasts alternate, so at a `last` bin these are the line's own first bin, the
// previous line's first bin, the bin itself and the previous line's last bin).  Coordinates follow from bin positions by
// arithmetic, and a line's first byte is its end minus its length, which its coordinates give.  No lane walks a run or a gap.
struct ix_top2 { int64_t a, b; };        // the largest and the second largest position of a set (-1: none)
struct ix_state { ix_top2 F, L; };       // of the `first` bins and of the `last` bins

// the two largest of l and r, every position of r being above every position of l
__device__ __forceinline__ ix_top2 ix_join(ix_top2 l, ix_top2 r)
{
    if (r.a < 0) return l;
    ix_top2 o;
    o.a = r.a;
    o.b = r.b >= 0 ? r.b : l.a;
    return o;
}

__device__ __forceinline__ ix_state ix_join(const ix_state &l, const ix_state &r)
{
    ix_state o;
    o.F = ix_join(l.F, r.F);
    o.L = ix_join(l.L, r.L);
    return o;
}

__device__ __forceinline__ ix_state ix_none()
{
    ix_state o;
    o.F.a = o.F.b = o.L.a = o.L.b = -1;
    return o;
}

// 256 threads: the inclusive scan of v under ix_join, on top of `carry` (what lies in front of the workgroup's elements), which
// becomes the state behind them (uniform)
__device__ __forceinline__ ix_state ix_block_scan(ix_state v, ix_state &carry, ix_state *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ix_state x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ix_state y;
        y.F.a = (int64_t)__shfl_up((long long)x.F.a, o);
        y.F.b = (int64_t)__shfl_up((long long)x.F.b, o);
        y.L.a = (int64_t)__shfl_up((long long)x.L.a, o);
        y.L.b = (int64_t)__shfl_up((long long)x.L.b, o);
        if (lane >= o) x = ix_join(y, x);
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    ix_state base = carry, tot = carry;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base = ix_join(base, lds[w]);
        tot = ix_join(tot, lds[w]);
    }
    __syncthreads();
    carry = tot;
    return ix_join(base, x);
}

// One pass over the tiles of the text chain, in three modes.  0: the state of every tile on its own (tilestate).  Between 0 and the
// others ix_carry_kernel turns these into the state at every tile's end.  1: the chunks that start in every tile (tilechunks).
// 2, with tilechunks scanned: the chunks and the windows.  A chunk starts at a line whose bin differs from the previous line's, or
// that has no previous line in its record; it ends where the next chunk of its class begins (the text holds nothing but lines), the
// last one of a class at the class's end (ix_ends_kernel).  Line i owns the windows w with previous line's end <= w << 14 < its
// own end; the windows of a round's lines are numbered by a scan and dealt out to the lanes one by one, so a line that owns
// thousands costs its lane what any other does.
template <int MODE>
__global__ void __launch_bounds__(256) ix_tile_kernel(const uint32_t *__restrict__ q, const tb_rec *__restrict__ recs,
                                                      const int64_t *__restrict__ pref, const int64_t *__restrict__ wpref, tb_geom G,
                                                      int64_t W, const uint64_t *__restrict__ tileoff, const uint64_t *__restrict__ bounds,
                                                      ix_state *__restrict__ tilestate, uint64_t *__restrict__ tilechunks,
                                                      const uint64_t *__restrict__ cbounds, dgrp_track_chunk *__restrict__ chunks,
                                                      int64_t *__restrict__ linear, int depth)
{
    __shared__ uint64_t lds[4];
    __shared__ ix_state slds[4];
    __shared__ int64_t s_r0;
    __shared__ int64_t w_off[MODE == 2 ? 256 : 1], w_base[MODE == 2 ? 256 : 1], w_val[MODE == 2 ? 256 : 1];
    const int64_t tpc = G.NBpad / TRACK_TILE;
    const int64_t k = blockIdx.x / tpc, ti = (int64_t)blockIdx.x % tpc, f0 = ti * TRACK_TILE;
    if (threadIdx.x == 0) s_r0 = dgrp_record_of(pref, G.nrec, f0);
    __syncthreads();
    const int64_t r0 = s_r0;
    const uint32_t *qk = q + k * G.NBpad;
    ix_state carry = ix_none();
    if (MODE != 0 && ti > 0) carry = tilestate[blockIdx.x - 1];
    int64_t at = 0;                                                        // offset in the class's slice of the text
    uint64_t nchunk = 0, cfirst = 0, count = 0;
    if (MODE == 2) {
        at = (int64_t)(tileoff[blockIdx.x] - bounds[k]);
        nchunk = tilechunks[blockIdx.x];
        cfirst = cbounds[k];
    }
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const int64_t f = f0 + r * 256 + threadIdx.x;
        const tb_part t = tb_part_of(qk, recs, pref, G, r0, f0, f);
        ix_state v = ix_none();
        if (t.p.first) v.F.a = f;
        if (t.p.last) v.L.a = f;
        const ix_state s = ix_block_scan(v, carry, slds);
        if (MODE == 0) continue;
        uint64_t round_bytes = 0;
        int64_t ex = 0;
        if (MODE == 2) ex = (int64_t)block_exclusive_scan((uint64_t)(t.p.head + t.p.tail), &round_bytes, lds);
        bool cs = false;
        uint32_t bn = 0;
        int64_t rr = 0, beg = 0, wbase = 0, wc = 0;
        if (t.p.last) {
            rr = tb_record_from(pref, G.nrec, r0, f0, f);
            const tb_rec R = recs[rr];
            const track_geom g = tb_geom_of(R, G.bin);
            const int64_t p0 = pref[rr], end = t.p.hi;
            int64_t start, pstart, pend = 0, x;
            track_bin_span(g, s.F.a - p0, start, x);                       // the line's first bin
            bn = tabix_reg2bin_depth(start, end, depth);
            const bool prev = s.L.b >= p0;                                 // the previous `last` bin lies in this record
            cs = true;
            if (prev) {
                track_bin_span(g, s.F.b - p0, pstart, x);
                track_bin_span(g, s.L.b - p0, x, pend);
                cs = tabix_reg2bin_depth(pstart, pend, depth) != bn;
            }
            if (MODE == 2) {
                const int64_t len = R.name_len + track_decimal_width((uint64_t)start) + track_decimal_width((uint64_t)end) + G.digits + 6;
                beg = at + ex + t.p.head + t.p.tail - len;
                const int64_t wl = prev ? (pend + (1 << TABIX_MIN_SHIFT) - 1) >> TABIX_MIN_SHIFT : 0;
                wc = ((end - 1) >> TABIX_MIN_SHIFT) - wl + 1;
                wbase = k * W + wpref[rr] + wl;
            }
        }
        if (MODE == 1) {
            count += cs ? 1 : 0;
            continue;
        }
        uint64_t ctot, wtot;
        const uint64_t cex = block_exclusive_scan(cs ? 1 : 0, &ctot, lds);
        if (cs) {
            const uint64_t c = nchunk + cex;
            chunks[c].beg = beg;
            chunks[c].rec = (int32_t)rr;
            chunks[c].bin = bn;
            if (c > cfirst) chunks[c - 1].end = beg;
        }
        nchunk += ctot;
        const uint64_t wex = block_exclusive_scan((uint64_t)wc, &wtot, lds);
        if (wtot > 0) {                                                    // (uniform)
            w_off[threadIdx.x] = (int64_t)wex;
            w_base[threadIdx.x] = wbase;
            w_val[threadIdx.x] = beg;
            __syncthreads();
            for (int64_t i = threadIdx.x; i < (int64_t)wtot; i += 256) {
                int lo = 0, hi = 256;                                      // w_off[lo] <= i < w_off[hi]: the last line at or below i owns it
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (w_off[mid] <= i) lo = mid; else hi = mid;
                }
                linear[w_base[lo] + (i - w_off[lo])] = w_val[lo];
            }
            __syncthreads();
        }
        at += (int64_t)round_bytes;
    }
    if (MODE == 0 && threadIdx.x == 0) tilestate[blockIdx.x] = carry;
    if (MODE == 1) {
        for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = count;
        __syncthreads();
        if (threadIdx.x == 0) tilechunks[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
    }
}

// the tiles' own states to the states at their ends, class by class: one workgroup per class
__global__ void __launch_bounds__(256) ix_carry_kernel(ix_state *__restrict__ tilestate, int64_t tpc)
{
    __shared__ ix_state slds[4];
    ix_state *ts = tilestate + (int64_t)blockIdx.x * tpc;
    ix_state carry = ix_none();
    for (int64_t base = 0; base < tpc; base += 256) {
        const int64_t i = base + threadIdx.x;
        const ix_state s = ix_block_scan(i < tpc ? ts[i] : ix_none(), carry, slds);
        if (i < tpc) ts[i] = s;
    }
}

// the last chunk of every class ends where the class's text ends
__global__ void __launch_bounds__(128) ix_ends_kernel(const uint64_t *__restrict__ cbounds, const uint64_t *__restrict__ bounds, int ncls,
                                                     dgrp_track_chunk *__restrict__ chunks)
{
    const int k = threadIdx.x;
    if (k < ncls && cbounds[k + 1] > cbounds[k]) chunks[cbounds[k + 1] - 1].end = (int64_t)(bounds[k + 1] - bounds[k]);
}

// the index entry's workspace: the text chain's, then its own parts
struct ix_layout { tb_layout t; int64_t wpref, state, tilechunks, cgrand, cbounds, bytes; };

static bool ix_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, int64_t names_bytes,
                     int depth, ix_layout *l)
{
    if (depth != TABIX_DEPTH && depth != CSI_DEPTH) return false;
    if (!tb_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, &l->t) || nrec >= (1ll << 31)) return false;
    for (int64_t r = 0; r < nrec; ++r)
        if (h_startpos[r] + h_n[r] > tabix_max_end(depth)) return false;
    const int64_t ntiles = l->t.NBpad / TRACK_TILE * ncls;
    int64_t p = l->t.bytes;
    l->wpref = p;
    p += dgrp_align_up((nrec + 1) * 8, 256);
    l->state = p;
    p += dgrp_align_up(ntiles * (int64_t)sizeof(ix_state), 256);
    l->tilechunks = p;
    p += dgrp_align_up(ntiles * 8, 256);
    l->cgrand = p;
    p += 256;
    l->cbounds = p;
    p += dgrp_align_up((int64_t)(ncls + 1) * 8, 256);
    l->bytes = p;
    return true;
}

}   // namespace

bool dgrp_tb_carve(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls, int64_t names_bytes, tb_layout *l)
{
    return tb_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, l);
}

int dgrp_tb_bins(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n, const int64_t *h_startpos,
                 const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits, int64_t bin, void *d_work,
                 const tb_layout &l, hipStream_t stream, std::vector<char> &tab, tb_dev *D)
{
    return tb_bins(d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin, d_work, l, stream, tab, D);
}

DGRP_EXPORT int64_t dgrp_track_workspace_bytes(int64_t n, int64_t bin)
{
    tb_layout l;
    return track_carve_one(n, bin, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_text(const float *d_probs, int64_t n, int C, int cls, int digits, int64_t bin, int64_t offset,
                                const char *name, int64_t name_len, char *d_text, int64_t cap, int64_t *h_bytes,
                                void *d_work, int64_t work_bytes, void *stream_)
{
    DGRP_REQUIRE(h_bytes, "dgrp_track_text: NULL h_bytes");
    DGRP_REQUIRE(n >= 0 && n <= TRACK_MAX_EXTENT, "dgrp_track_text: bad n %lld", (long long)n);
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC && cls >= 0 && cls < C, "dgrp_track_text: bad C/cls (%d, %d)", C, cls);
    DGRP_REQUIRE(digits >= 1 && digits <= 4, "dgrp_track_text: digits must lie in 1..4, got %d", digits);
    DGRP_REQUIRE(bin >= 1 && bin <= TRACK_MAX_EXTENT, "dgrp_track_text: bad bin %lld", (long long)bin);
    DGRP_REQUIRE(offset >= 0 && offset <= TRACK_MAX_EXTENT, "dgrp_track_text: bad offset %lld", (long long)offset);
    DGRP_REQUIRE(name_len >= 0 && cap >= 0, "dgrp_track_text: bad name_len/cap");
    DGRP_REQUIRE(name_len <= DGRP_TRACK_NAME_ROOM, "dgrp_track_text: a name of %lld bytes is longer than the limit of %d",
                 (long long)name_len, DGRP_TRACK_NAME_ROOM);
    DGRP_REQUIRE((name || name_len == 0) && (d_text || cap == 0) && (n == 0 || (d_probs && d_work)),
                 "dgrp_track_text: NULL pointer");
    *h_bytes = 0;
    if (n == 0) return DGRP_OK;
    tb_layout l;
    DGRP_REQUIRE(track_carve_one(n, bin, &l), "dgrp_track_text: too many bins in one call");
    if (work_bytes < l.bytes) {
        dgrp_set_error("dgrp_track_text: workspace %lld < %lld bytes", (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    const int64_t row0 = 0, name_off[2] = {0, name_len};
    int64_t class_off[2] = {0, 0};
    const int rc = tb_run(d_probs, C, 1, &row0, &n, &offset, name, name_off, &cls, 1, digits, bin, d_text, cap, class_off, d_work, l,
                          (hipStream_t)stream_);
    *h_bytes = class_off[1];
    return rc;
}

DGRP_EXPORT int64_t dgrp_track_batch_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                                     int64_t names_bytes)
{
    tb_layout l;
    return tb_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_text_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                      const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls,
                                      int ncls, int digits, int64_t bin, char *d_text, int64_t cap, int64_t *h_class_off,
                                      void *d_work, int64_t work_bytes, void *stream_)
{
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "dgrp_track_text_batch: bad C %d", C);
    DGRP_REQUIRE(ncls >= 1 && ncls <= C, "dgrp_track_text_batch: ncls must lie in 1..C (%d, C = %d)", ncls, C);
    DGRP_REQUIRE(h_class_off && h_cls, "dgrp_track_text_batch: NULL h_class_off or h_cls");
    for (int k = 0; k <= ncls; ++k) h_class_off[k] = 0;
    DGRP_REQUIRE(nrec >= 0, "dgrp_track_text_batch: bad nrec %lld", (long long)nrec);
    for (int k = 0; k < ncls; ++k)
        DGRP_REQUIRE(h_cls[k] >= 0 && h_cls[k] < C, "dgrp_track_text_batch: class %d is not in 0..%d", h_cls[k], C - 1);
    DGRP_REQUIRE(digits >= 1 && digits <= 4, "dgrp_track_text_batch: digits must lie in 1..4, got %d", digits);
    DGRP_REQUIRE(bin >= 1 && bin <= TRACK_MAX_EXTENT, "dgrp_track_text_batch: bad bin %lld", (long long)bin);
    DGRP_REQUIRE(cap >= 0, "dgrp_track_text_batch: bad cap %lld", (long long)cap);
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_row0 && h_n && h_startpos && h_name_off, "dgrp_track_text_batch: NULL host table");
    DGRP_REQUIRE(h_name_off[0] >= 0, "dgrp_track_text_batch: record 0: bad name offset %lld", (long long)h_name_off[0]);
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_n[r] >= 1 && h_n[r] <= TRACK_MAX_EXTENT, "dgrp_track_text_batch: record %lld: bad n %lld", (long long)r,
                     (long long)h_n[r]);
        DGRP_REQUIRE(h_startpos[r] >= 0 && h_startpos[r] <= TRACK_MAX_EXTENT, "dgrp_track_text_batch: record %lld: bad offset %lld",
                     (long long)r, (long long)h_startpos[r]);
        DGRP_REQUIRE(h_row0[r] >= 0, "dgrp_track_text_batch: record %lld: bad first row %lld", (long long)r, (long long)h_row0[r]);
        DGRP_REQUIRE(h_name_off[r + 1] >= h_name_off[r], "dgrp_track_text_batch: record %lld: descending name offsets (%lld, %lld)",
                     (long long)r, (long long)h_name_off[r], (long long)h_name_off[r + 1]);
    }
    const int64_t names_bytes = h_name_off[nrec];
    DGRP_REQUIRE((names || names_bytes == 0) && (d_text || cap == 0) && d_probs && d_work, "dgrp_track_text_batch: NULL pointer");
    tb_layout l;
    DGRP_REQUIRE(tb_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, &l), "dgrp_track_text_batch: too many bins in one call");
    if (work_bytes < l.bytes) {
        dgrp_set_error("dgrp_track_text_batch: workspace %lld < %lld bytes", (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    return tb_run(d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin, d_text, cap, h_class_off, d_work,
                  l, (hipStream_t)stream_);
}

// The index entry at `depth` levels below the root (5: the .tbi entry `who` = dgrp_track_index_batch, whose texts these are; 5 or 6:
// dgrp_track_csi_batch).  Only the bin numbers and the record-end limit depend on the depth.
static int ix_entry(const char *who, int depth, const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                    const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls, int ncls, int digits,
                    int64_t bin, dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_chunk_off, int64_t *d_linear,
                    int64_t linear_cap, void *d_work, int64_t work_bytes, void *stream_, bool csi)
{
    DGRP_REQUIRE(depth == TABIX_DEPTH || depth == CSI_DEPTH, "%s: depth must be 5 or 6, got %d", who, depth);
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC, "%s: bad C %d", who, C);
    DGRP_REQUIRE(ncls >= 1 && ncls <= C, "%s: ncls must lie in 1..C (%d, C = %d)", who, ncls, C);
    DGRP_REQUIRE(h_chunk_off && h_cls, "%s: NULL h_chunk_off or h_cls", who);
    for (int k = 0; k <= ncls; ++k) h_chunk_off[k] = 0;
    DGRP_REQUIRE(nrec >= 0 && nrec < (1ll << 31), "%s: bad nrec %lld", who, (long long)nrec);
    for (int k = 0; k < ncls; ++k)
        DGRP_REQUIRE(h_cls[k] >= 0 && h_cls[k] < C, "%s: class %d is not in 0..%d", who, h_cls[k], C - 1);
    DGRP_REQUIRE(digits >= 1 && digits <= 4, "%s: digits must lie in 1..4, got %d", who, digits);
    DGRP_REQUIRE(bin >= 1 && bin <= TRACK_MAX_EXTENT, "%s: bad bin %lld", who, (long long)bin);
    DGRP_REQUIRE(chunk_cap >= 0 && linear_cap >= 0, "%s: bad chunk_cap/linear_cap (%lld, %lld)", who, (long long)chunk_cap,
                 (long long)linear_cap);
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_row0 && h_n && h_startpos && h_name_off, "%s: NULL host table", who);
    DGRP_REQUIRE(h_name_off[0] >= 0, "%s: record 0: bad name offset %lld", who, (long long)h_name_off[0]);
    std::vector<int64_t> wpref((size_t)nrec + 1, 0);                       // windows in front of every record
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_n[r] >= 1 && h_n[r] <= TRACK_MAX_EXTENT, "%s: record %lld: bad n %lld", who, (long long)r,
                     (long long)h_n[r]);
        DGRP_REQUIRE(h_startpos[r] >= 0 && h_startpos[r] <= TRACK_MAX_EXTENT, "%s: record %lld: bad offset %lld", who,
                     (long long)r, (long long)h_startpos[r]);
        if (csi) {
            DGRP_REQUIRE(h_startpos[r] + h_n[r] <= tabix_max_end(depth),
                         "%s: record %lld ends at %lld, above 2^%d = %lld, the largest coordinate of a CSI index of depth %d", who,
                         (long long)r, (long long)(h_startpos[r] + h_n[r]), TABIX_MIN_SHIFT + 3 * depth, (long long)tabix_max_end(depth),
                         depth);
        } else {
            DGRP_REQUIRE(h_startpos[r] + h_n[r] <= TABIX_MAX_END,
                         "%s: record %lld ends at %lld, above 2^29 = 536870912, the largest coordinate of a tabix index", who,
                         (long long)r, (long long)(h_startpos[r] + h_n[r]));
        }
        DGRP_REQUIRE(h_row0[r] >= 0, "%s: record %lld: bad first row %lld", who, (long long)r, (long long)h_row0[r]);
        DGRP_REQUIRE(h_name_off[r + 1] >= h_name_off[r], "%s: record %lld: descending name offsets (%lld, %lld)", who,
                     (long long)r, (long long)h_name_off[r], (long long)h_name_off[r + 1]);
        wpref[(size_t)r + 1] = wpref[(size_t)r] + ((h_startpos[r] + h_n[r] - 1) >> TABIX_MIN_SHIFT) + 1;
    }
    const int64_t names_bytes = h_name_off[nrec], W = wpref[(size_t)nrec];
    DGRP_REQUIRE(linear_cap >= W * ncls, "%s: linear_cap %lld < %lld windows of %d classes", who, (long long)linear_cap,
                 (long long)(W * ncls), ncls);
    DGRP_REQUIRE((names || names_bytes == 0) && (d_chunks || chunk_cap == 0) && d_linear && d_probs && d_work,
                 "%s: NULL pointer", who);
    ix_layout l;
    DGRP_REQUIRE(ix_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, depth, &l), "%s: too many bins in one call", who);
    if (work_bytes < l.bytes) {
        dgrp_set_error("%s: workspace %lld < %lld bytes", who, (long long)work_bytes, (long long)l.bytes);
        return DGRP_ENOMEM;
    }
    hipStream_t stream = (hipStream_t)stream_;
    char *w = (char *)d_work;
    int64_t *d_wpref = (int64_t *)(w + l.wpref);
    ix_state *state = (ix_state *)(w + l.state);
    uint64_t *tilechunks = (uint64_t *)(w + l.tilechunks), *cgrand = (uint64_t *)(w + l.cgrand), *cbounds = (uint64_t *)(w + l.cbounds);
    DGRP_HIP(hipMemcpyAsync(d_wpref, wpref.data(), wpref.size() * 8, hipMemcpyHostToDevice, stream));
    tb_dev D;
    std::vector<int64_t> text_off((size_t)ncls + 1, 0);
    const int rc = tb_front(d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin, text_off.data(), d_work,
                            l.t, stream, &D);
    if (rc != DGRP_OK) return rc;
    const dim3 grid((unsigned)D.ntiles), block(256);
    hipLaunchKernelGGL(ix_tile_kernel<0>, grid, block, 0, stream, D.q, D.recs, D.pref, d_wpref, D.G, W, D.tiles, D.bounds, state, tilechunks,
                       cbounds, d_chunks, d_linear, depth);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ix_carry_kernel, dim3((unsigned)ncls), block, 0, stream, state, D.tpc);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ix_tile_kernel<1>, grid, block, 0, stream, D.q, D.recs, D.pref, d_wpref, D.G, W, D.tiles, D.bounds, state, tilechunks,
                       cbounds, d_chunks, d_linear, depth);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), block, 0, stream, tilechunks, D.ntiles, cgrand);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(tb_bounds_kernel, dim3(1), dim3(128), 0, stream, tilechunks, D.tpc, ncls, cgrand, cbounds);
    DGRP_LAUNCH_CHECK();
    std::vector<uint64_t> off((size_t)ncls + 1, 0);
    DGRP_HIP(hipMemcpyAsync(off.data(), cbounds, off.size() * 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k <= ncls; ++k) h_chunk_off[k] = (int64_t)off[(size_t)k];
    if (h_chunk_off[ncls] > chunk_cap) return DGRP_OK;                      // (too small: the caller retries with room for all of them)
    DGRP_HIP(hipMemsetAsync(d_linear, 0xff, (size_t)(W * ncls) * 8, stream));          // -1: no line ends behind this window
    hipLaunchKernelGGL(ix_tile_kernel<2>, grid, block, 0, stream, D.q, D.recs, D.pref, d_wpref, D.G, W, D.tiles, D.bounds, state, tilechunks,
                       cbounds, d_chunks, d_linear, depth);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ix_ends_kernel, dim3(1), dim3(128), 0, stream, cbounds, D.bounds, ncls, d_chunks);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_track_index_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                                     int64_t names_bytes)
{
    ix_layout l;
    return ix_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, TABIX_DEPTH, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_index_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                       const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls,
                                       int ncls, int digits, int64_t bin, dgrp_track_chunk *d_chunks, int64_t chunk_cap,
                                       int64_t *h_chunk_off, int64_t *d_linear, int64_t linear_cap, void *d_work, int64_t work_bytes,
                                       void *stream_)
{
    return ix_entry("dgrp_track_index_batch", TABIX_DEPTH, d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits,
                    bin, d_chunks, chunk_cap, h_chunk_off, d_linear, linear_cap, d_work, work_bytes, stream_, false);
}

DGRP_EXPORT int64_t dgrp_track_csi_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                                   int64_t names_bytes, int depth)
{
    ix_layout l;
    return ix_carve(nrec, h_n, h_startpos, bin, ncls, names_bytes, depth, &l) ? l.bytes : 0;
}

DGRP_EXPORT int dgrp_track_csi_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                     const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls,
                                     int ncls, int digits, int64_t bin, int depth, dgrp_track_chunk *d_chunks, int64_t chunk_cap,
                                     int64_t *h_chunk_off, int64_t *d_linear, int64_t linear_cap, void *d_work, int64_t work_bytes,
                                     void *stream_)
{
    return ix_entry("dgrp_track_csi_batch", depth, d_probs, C, nrec, h_row0, h_n, h_startpos, names, h_name_off, h_cls, ncls, digits, bin,
                    d_chunks, chunk_cap, h_chunk_off, d_linear, linear_cap, d_work, work_bytes, stream_, true);
}
