// UCSC .2bit output (predict --mask_twobit): the masked text of plain record bodies, as dgrp_fasta_mask_batch leaves it on the
// device, turned into the records of a 2bit file -- dnaSize, the N and mask block tables (the maximal runs of non-ACGT and of
// lower-case characters) and the packed bases.  A byte stream read twice, 16 bytes per lane: once for the per-tile counts, once for
// the write.  The only order between workgroups is the launch boundary; no atomics.  See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "body_tiles.h"
#include "scan.h"
#include <vector>

namespace {

#define TBP_CODES (BODY_TILE + 16) // two-bit codes of one tile in LDS: up to 3 in front (the byte the previous tile owns), 3 behind

// T=0 C=1 A=2 G=3 in either case; 4: anything else, which is N
__device__ __forceinline__ uint32_t tbp_code(uint32_t x)
{
    const uint32_t l = x | 0x20u;
    return l == 't' ? 0u : l == 'c' ? 1u : l == 'a' ? 2u : l == 'g' ? 3u : 4u;
}

__device__ __forceinline__ bool tbp_lower(uint32_t x) { return x >= 'a' && x <= 'z'; }

// The sequence byte in front of buffer position q of the record whose body starts at `lo`: the nearest byte below q that is neither
// CR nor LF -- it may lie beyond a line end or in the previous tile.  At sequence position 0 there is none: 'A', after which no run
// is open.  Run starts and run ends are decided against this byte alone.
__device__ __forceinline__ uint32_t tbp_prev_seq_byte(const uint8_t *__restrict__ raw, int64_t lo, int64_t q)
{
    while (q > lo) {
        const uint32_t x = raw[--q];
        if (!body_lineend(x)) return x;
    }
    return 'A';
}

// blobs start at any byte: a 32-bit word goes out whole where it is aligned, else byte by byte (little-endian)
__device__ __forceinline__ void tbp_store_u32(uint8_t *p, uint32_t v)
{
    if (((uintptr_t)p & 3) == 0) {
        *(uint32_t *)p = v;
    } else {
        p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
    }
}

__device__ __forceinline__ uint32_t tbp_load_u32(const uint8_t *p)
{
    if (((uintptr_t)p & 3) == 0) return *(const uint32_t *)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- stage 1.  Per tile: cnt[t] = sequence bytes, cnt[ntiles + t] = N-run starts | mask-run starts << 32.
__global__ void __launch_bounds__(256) tbp_count_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ tile0,
                                                        const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                        int64_t nrec, int64_t ntiles, uint64_t *__restrict__ cnt)
{
    __shared__ uint64_t lds[2][4];
    __shared__ int64_t s_rec;
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) s_rec = dgrp_record_of(tile0, nrec, t);
    __syncthreads();
    const int64_t r = s_rec;
    const body_span s = body_lane_span(off[r], len[r], t - tile0[r]);
    alignas(16) uint8_t b[16];
    body_load(raw, s, b);
    uint64_t c = 0, runs = 0;
    if (s.hi > s.lo) {
        const uint32_t prev = tbp_prev_seq_byte(raw, off[r], s.word + s.lo);
        bool pn = tbp_code(prev) == 4u, pl = tbp_lower(prev);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t x = b[j];
            if (body_lineend(x)) continue;
            const bool n = tbp_code(x) == 4u, l = tbp_lower(x);
            c += 1;
            runs += (n && !pn ? 1ull : 0ull) + (l && !pl ? 1ull << 32 : 0ull);
            pn = n; pl = l;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o); runs += __shfl_xor(runs, o); }
    if ((threadIdx.x & 63) == 0) { lds[0][threadIdx.x >> 6] = c; lds[1][threadIdx.x >> 6] = runs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[t] = lds[0][0] + lds[0][1] + lds[0][2] + lds[0][3];
        cnt[ntiles + t] = lds[1][0] + lds[1][1] + lds[1][2] + lds[1][3];
    }
}

// ex = the exclusive scan of cnt over 2 ntiles elements, ex[2 ntiles] its total.  Sequence bytes in front of tile t: ex[t]; runs in
// front of it: ex[ntiles + t] - ex[ntiles] (the scan ran on through the first half; the difference is exact modulo 2^64).
__device__ __forceinline__ uint64_t tbp_runs_before(const uint64_t *__restrict__ ex, int64_t ntiles, int64_t t)
{
    return ex[ntiles + t] - ex[ntiles];
}

// rc[2 r] = sequence bytes, rc[2 r + 1] = runs (N | mask << 32) in front of record r, r = 0 .. nrec
__global__ void __launch_bounds__(256) tbp_record_kernel(const uint64_t *__restrict__ ex, const int64_t *__restrict__ tile0,
                                                         int64_t nrec, int64_t ntiles, uint64_t *__restrict__ rc)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrec) return;
    rc[2 * r] = ex[tile0[r]];
    rc[2 * r + 1] = tbp_runs_before(ex, ntiles, tile0[r]);
}

struct tbp_blob {                 // where the parts of one record's blob lie
    uint8_t *base, *nstart, *nsize, *mstart, *msize, *packed;
    uint32_t dna, nb, mb;
};

__device__ __forceinline__ tbp_blob tbp_blob_of(uint8_t *out, const int64_t *__restrict__ blob, const uint64_t *__restrict__ rc, int64_t r)
{
    tbp_blob B;
    const uint64_t runs = rc[2 * r + 3] - rc[2 * r + 1];
    B.dna = (uint32_t)(rc[2 * r + 2] - rc[2 * r]);
    B.nb = (uint32_t)runs;
    B.mb = (uint32_t)(runs >> 32);
    B.base = out + blob[r];
    B.nstart = B.base + 8;
    B.nsize = B.nstart + 4 * (int64_t)B.nb;
    B.mstart = B.nsize + 4 * (int64_t)B.nb + 4;
    B.msize = B.mstart + 4 * (int64_t)B.mb;
    B.packed = B.msize + 4 * (int64_t)B.mb + 4;
    return B;
}

// ---- stage 2.  Per tile: the run starts into the start tables, the run ENDS into the size tables (tbp_finish_kernel subtracts),
// and the packed bytes whose first base lies in this tile -- their last bases may lie in the following tiles.
__global__ void __launch_bounds__(256) tbp_write_kernel(const uint8_t *__restrict__ raw, const int64_t *__restrict__ tile0,
                                                        const int64_t *__restrict__ off, const int64_t *__restrict__ len,
                                                        const int64_t *__restrict__ blob, int64_t nrec, int64_t ntiles,
                                                        const uint64_t *__restrict__ ex, const uint64_t *__restrict__ rc,
                                                        uint8_t *__restrict__ out)
{
    __shared__ uint64_t lds[4];
    __shared__ int64_t s_rec;
    __shared__ alignas(16) uint8_t cd[TBP_CODES];
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) s_rec = dgrp_record_of(tile0, nrec, t);
    __syncthreads();
    const int64_t r = s_rec;
    const int64_t p0 = (int64_t)(ex[t] - rc[2 * r]), p1 = p0 + (int64_t)(ex[t + 1] - ex[t]);      // sequence positions of this tile
    if (p1 == p0) return;                                           // line ends only: nothing starts, ends or is packed here
    const tbp_blob B = tbp_blob_of(out, blob, rc, r);
    const uint64_t runs0 = tbp_runs_before(ex, ntiles, t) - rc[2 * r + 1];
    const int64_t o = p0 & ~(int64_t)3;                              // cd[i] = code of sequence position o + i
    const int64_t roff = off[r], rlen = len[r];
    const body_span s = body_lane_span(roff, rlen, t - tile0[r]);
    alignas(16) uint8_t b[16];
    body_load(raw, s, b);
    uint64_t v = 0;
    bool pn = false, pl = false;
    if (s.hi > s.lo) {
        const uint32_t prev = tbp_prev_seq_byte(raw, roff, s.word + s.lo);
        pn = tbp_code(prev) == 4u; pl = tbp_lower(prev);
        bool qn = pn, ql = pl;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t x = b[j];
            if (body_lineend(x)) continue;
            const bool n = tbp_code(x) == 4u, l = tbp_lower(x);
            v += 1ull + (n && !qn ? 1ull << 16 : 0ull) + (l && !ql ? 1ull << 32 : 0ull);
            qn = n; ql = l;
        }
    }
    const uint64_t e = block_exclusive_scan(v, nullptr, lds);        // per lane: sequence bytes | N starts << 16 | mask starts << 32
    int64_t p = p0 + (int64_t)(e & 0xffffu);
    int64_t kn = (int64_t)(uint32_t)runs0 + (int64_t)((e >> 16) & 0xffffu), km = (int64_t)(runs0 >> 32) + (int64_t)(e >> 32);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t x = b[j];
        if (body_lineend(x)) continue;
        const uint32_t code = tbp_code(x);
        const bool n = code == 4u, l = tbp_lower(x);
        if (n && !pn) { tbp_store_u32(B.nstart + 4 * kn, (uint32_t)p); ++kn; }
        if (!n && pn) tbp_store_u32(B.nsize + 4 * (kn - 1), (uint32_t)p);
        if (l && !pl) { tbp_store_u32(B.mstart + 4 * km, (uint32_t)p); ++km; }
        if (!l && pl) tbp_store_u32(B.msize + 4 * (km - 1), (uint32_t)p);
        if (p + 1 == (int64_t)B.dna) {                                // a run that is open at the last base ends behind it
            if (n) tbp_store_u32(B.nsize + 4 * (kn - 1), B.dna);
            if (l) tbp_store_u32(B.msize + 4 * (km - 1), B.dna);
        }
        cd[p - o] = (uint8_t)(n ? 0u : code);
        pn = n; pl = l;
        ++p;
    }
    if (threadIdx.x == 0 && (p1 & 3)) {
        // the last owned byte ends in the following tiles: up to three more sequence bytes of the record, 0 where it ends first
        int64_t q = (roff & ~(int64_t)15) + (t - tile0[r] + 1) * BODY_TILE;
        const int64_t end = roff + rlen;
        int got = 0;
        for (; q < end && got < 3; ++q) {
            const uint32_t x = raw[q];
            if (body_lineend(x)) continue;
            const uint32_t code = tbp_code(x);
            cd[p1 - o + got++] = (uint8_t)(code == 4u ? 0u : code);
        }
        for (; got < 3; ++got) cd[p1 - o + got] = 0;
    }
    __syncthreads();
    // packed bytes [q0, q1) are this tile's: those whose first base is one of its sequence positions.  A lane takes one 16-byte
    // aligned word of the output.
    const int64_t q0 = (p0 + 3) >> 2, q1 = (p1 + 3) >> 2;
    const int64_t a0 = (int64_t)(((uintptr_t)B.packed + (uintptr_t)q0) & ~(uintptr_t)15) - (int64_t)(uintptr_t)B.packed;   // (as a byte index)
    const int64_t w = a0 + (int64_t)threadIdx.x * 16;
    const int64_t qa = w > q0 ? w : q0, qe = w + 16 < q1 ? w + 16 : q1;
    if (qa >= qe) return;
    uint32_t c[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t q = w + j;
        if (q < qa || q >= qe) continue;
        const uint32_t k = *(const uint32_t *)(cd + (4 * q - o));      // four codes, the first base in the low byte
        const uint32_t byte = ((k & 3u) << 6) | (((k >> 8) & 3u) << 4) | (((k >> 16) & 3u) << 2) | ((k >> 24) & 3u);
        c[j >> 2] |= byte << (8 * (j & 3));
    }
    if (qa == w && qe == w + 16) {
        *(uint4 *)(B.packed + w) = make_uint4(c[0], c[1], c[2], c[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t q = w + j;
            if (q >= qa && q < qe) B.packed[q] = (uint8_t)(c[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// largest r < nrec whose runs in front (N: the low half of rc[2 r + 1], mask: the high half) are <= g
__device__ __forceinline__ int64_t tbp_record_of_run(const uint64_t *__restrict__ rc, int64_t nrec, int64_t g, int shift)
{
    int64_t lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(uint32_t)(rc[2 * mid + 1] >> shift) <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- stage 2, after the write: one lane per record for the four words around the tables, one per run for end -> size.
__global__ void __launch_bounds__(256) tbp_finish_kernel(const int64_t *__restrict__ blob, int64_t nrec, const uint64_t *__restrict__ rc,
                                                         int64_t nruns, int64_t mruns, uint8_t *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nrec) {
        const tbp_blob B = tbp_blob_of(out, blob, rc, i);
        tbp_store_u32(B.base, B.dna);
        tbp_store_u32(B.base + 4, B.nb);
        tbp_store_u32(B.mstart - 4, B.mb);
        tbp_store_u32(B.packed - 4, 0u);
        return;
    }
    i -= nrec;
    if (i >= nruns + mruns) return;
    const bool mask = i >= nruns;
    const int64_t g = mask ? i - nruns : i;
    const int64_t r = tbp_record_of_run(rc, nrec, g, mask ? 32 : 0);
    const tbp_blob B = tbp_blob_of(out, blob, rc, r);
    const int64_t k = g - (int64_t)(uint32_t)(rc[2 * r + 1] >> (mask ? 32 : 0));
    uint8_t *st = (mask ? B.mstart : B.nstart) + 4 * k, *sz = (mask ? B.msize : B.nsize) + 4 * k;
    tbp_store_u32(sz, tbp_load_u32(sz) - tbp_load_u32(st));
}

}   // namespace

DGRP_EXPORT int64_t dgrp_twobit_pack_workspace_bytes(int64_t nrec, int64_t total_bytes)
{
    if (nrec < 0 || total_bytes < 0) return 0;
    const int64_t tiles = body_tile_bound(nrec, total_bytes);
    return dgrp_align_up((2 * tiles + 1) * 8, 256) + dgrp_align_up(((2 * tiles + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256) +
           dgrp_align_up((4 * nrec + 1) * 8, 256) + dgrp_align_up(2 * (nrec + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_twobit_pack_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len, uint8_t *d_out,
                                       int64_t out_off, int64_t out_cap, int64_t *h_counts, int64_t *h_blob_off, void *d_work,
                                       int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(nrec >= 0 && out_off >= 0 && out_cap >= 0, "dgrp_twobit_pack_batch: negative size");
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_off && h_len && h_counts && h_blob_off, "dgrp_twobit_pack_batch: NULL host table");
    int64_t total = 0;
    std::vector<int64_t> tab((size_t)(4 * nrec + 1));                  // tile0[nrec + 1], off[nrec], len[nrec], blob[nrec]
    int64_t *tile0 = tab.data(), *off = tile0 + nrec + 1, *len = off + nrec, *blob = len + nrec;
    tile0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        DGRP_REQUIRE(h_off[r] >= 0 && h_len[r] >= 0, "dgrp_twobit_pack_batch: negative range (record %lld)", (long long)r);
        DGRP_REQUIRE(h_len[r] <= 0xffffffffll - total, "dgrp_twobit_pack_batch: more than 2^32 - 1 bytes in one call (record %lld)",
                     (long long)r);
        total += h_len[r];
        off[r] = h_off[r];
        len[r] = h_len[r];
        tile0[r + 1] = tile0[r] + body_tiles_of(h_off[r], h_len[r]);
    }
    const int64_t ntiles = tile0[nrec];
    const int64_t need = dgrp_twobit_pack_workspace_bytes(nrec, total);
    if (work_bytes < need) {
        dgrp_set_error("dgrp_twobit_pack_batch: workspace %lld < %lld bytes", (long long)work_bytes, (long long)need);
        return DGRP_ENOMEM;
    }
    if (out_off > out_cap || 16 * nrec > out_cap - out_off) {           // (every blob has its four words)
        dgrp_set_error("dgrp_twobit_pack_batch: %lld records do not fit the output buffer of %lld bytes from offset %lld",
                       (long long)nrec, (long long)out_cap, (long long)out_off);
        return DGRP_ENOMEM;
    }
    DGRP_REQUIRE(d_out && d_work && (ntiles == 0 || d_raw), "dgrp_twobit_pack_batch: NULL device pointer");
    DGRP_REQUIRE(((uintptr_t)d_raw & 15) == 0, "dgrp_twobit_pack_batch: d_raw must be 16-byte aligned");
    const int64_t bound = body_tile_bound(nrec, total);
    uint64_t *ex = (uint64_t *)d_work;                                  // counts [2 ntiles], then their exclusive scan and the total
    uint64_t *scan_tiles = (uint64_t *)((char *)ex + dgrp_align_up((2 * bound + 1) * 8, 256));
    int64_t *d_tab = (int64_t *)((char *)scan_tiles + dgrp_align_up(((2 * bound + SCAN_TILE - 1) / SCAN_TILE + 1) * 8, 256));
    uint64_t *d_rc = (uint64_t *)((char *)d_tab + dgrp_align_up((4 * nrec + 1) * 8, 256));
    int64_t *d_tile0 = d_tab, *d_off = d_tile0 + nrec + 1, *d_len = d_off + nrec, *d_blob = d_len + nrec;
    std::vector<uint64_t> rc((size_t)(2 * (nrec + 1)), 0);
    if (ntiles > 0) {
        DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), (size_t)(3 * nrec + 1) * 8, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(tbp_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, d_tile0, d_off, d_len, nrec, ntiles, ex);
        DGRP_LAUNCH_CHECK();
        const int rcs = device_exclusive_scan(ex, ex, 2 * ntiles, scan_tiles, ex + 2 * ntiles, stream);
        if (rcs != DGRP_OK) return rcs;
        hipLaunchKernelGGL(tbp_record_kernel, dim3((unsigned)((nrec + 256) / 256)), dim3(256), 0, stream, ex, d_tile0, nrec, ntiles, d_rc);
        DGRP_LAUNCH_CHECK();
        DGRP_HIP(hipMemcpyAsync(rc.data(), d_rc, rc.size() * 8, hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipStreamSynchronize(stream));                        // the entry's only synchronisation: the blobs are laid out by the counts
    } else {
        DGRP_HIP(hipMemcpyAsync(d_rc, rc.data(), rc.size() * 8, hipMemcpyHostToDevice, stream));
    }
    int64_t pos = out_off;
    for (int64_t r = 0; r < nrec; ++r) {
        const uint64_t runs = rc[2 * r + 3] - rc[2 * r + 1];
        const int64_t dna = (int64_t)(rc[2 * r + 2] - rc[2 * r]), nb = (int64_t)(uint32_t)runs, mb = (int64_t)(runs >> 32);
        h_counts[3 * r] = dna; h_counts[3 * r + 1] = nb; h_counts[3 * r + 2] = mb;
        h_blob_off[r] = blob[r] = pos;
        pos += 16 + 8 * (nb + mb) + (dna + 3) / 4;
    }
    h_blob_off[nrec] = pos;
    if (pos > out_cap) {
        dgrp_set_error("dgrp_twobit_pack_batch: the records take %lld bytes from offset %lld, the output buffer has %lld",
                       (long long)(pos - out_off), (long long)out_off, (long long)out_cap);
        return DGRP_ENOMEM;
    }
    const int64_t nruns = (int64_t)(uint32_t)rc[2 * nrec + 1], mruns = (int64_t)(rc[2 * nrec + 1] >> 32);
    // (pageable sources: the copies have left the vectors when the call returns)
    DGRP_HIP(hipMemcpyAsync(d_blob, blob, (size_t)nrec * 8, hipMemcpyHostToDevice, stream));
    if (ntiles > 0) {
        hipLaunchKernelGGL(tbp_write_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, d_raw, d_tile0, d_off, d_len, d_blob, nrec, ntiles,
                           ex, d_rc, d_out);
        DGRP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tbp_finish_kernel, dim3((unsigned)((nrec + nruns + mruns + 255) / 256)), dim3(256), 0, stream, d_blob, nrec, d_rc,
                       nruns, mruns, d_out);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
