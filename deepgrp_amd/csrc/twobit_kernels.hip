// UCSC .2bit input (an addition; the reference reads FASTA text only): the packed bases of the records of ONE uploaded file turned
// into class indices (dgrp_twobit_encode_batch) or into the FASTA text of the file (dgrp_twobit_text_batch).  Both are one pass,
// n/4 bytes read and n written per base, 16 bytes per lane and store; N and soft-mask blocks arrive as merged, ascending, disjoint
// [start, end) intervals.  Nothing here synchronises or reads back.  See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include <vector>

namespace {

#define TB_LANE 16                              // output bytes per lane and store
#define TB_ITER 4                               // stores per lane
#define TB_WORDS (256 * TB_ITER)                // 16-byte words per workgroup
#define TB_SPAN (TB_WORDS * TB_LANE)            // output bytes per workgroup: 16 384
#define TB_LINE 50                              // bases per line of the text
#define TB_NONE 0x7fffffffffffffffll

// (the record of workgroup w is dgrp_record_of(wg0, nrec, w): records without workgroups share wg0 with the next record)

// first interval k in [lo, hi) whose end lies above `pos` (hi if none): the first that can cover a base >= pos
__device__ __forceinline__ int64_t tb_first_ending_after(const int64_t *__restrict__ iv, int64_t lo, int64_t hi, int64_t pos)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (iv[2 * mid + 1] > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// first interval k in [lo, hi) whose start is at or above `pos` (hi if none): the first that cannot cover a base < pos
__device__ __forceinline__ int64_t tb_first_starting_from(const int64_t *__restrict__ iv, int64_t lo, int64_t hi, int64_t pos)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (iv[2 * mid] >= pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// A lane's walk over the intervals of its workgroup: seek once, then ask for ascending bases.
struct tb_cursor {
    const int64_t *iv;
    int64_t k, hi, s, e;
    __device__ __forceinline__ void load()
    {
        if (k < hi) { s = iv[2 * k]; e = iv[2 * k + 1]; } else { s = e = TB_NONE; }
    }
    __device__ __forceinline__ void seek(const int64_t *iv_, int64_t lo_, int64_t hi_, int64_t pos)
    {
        iv = iv_; hi = hi_;
        k = tb_first_ending_after(iv, lo_, hi_, pos);
        load();
    }
    __device__ __forceinline__ bool covers(int64_t i)
    {
        while (e <= i) { ++k; load(); }
        return s <= i;
    }
};

// one packed byte (T=0 C=1 A=2 G=3, first base in the two most significant bits) -> four class indices (A=0 C=1 G=2 T=3), the
// first base in the low byte.  Per two-bit value (h, l): index = (h xnor l, not h).
__device__ __forceinline__ uint32_t tb_codes4(uint32_t b)
{
    const uint32_t x = (b >> 6) | (((b >> 4) & 3u) << 8) | (((b >> 2) & 3u) << 16) | ((b & 3u) << 24);
    const uint32_t h = (x >> 1) & 0x01010101u, l = x & 0x01010101u;
    return (h ^ 0x01010101u) | (((h ^ l) ^ 0x01010101u) << 1);
}

__device__ __forceinline__ uint32_t tb_code1(const uint8_t *__restrict__ packed, int64_t i)
{
    return (tb_codes4(packed[i >> 2]) >> (8 * (int)(i & 3))) & 0xffu;
}

// The packed bytes of bases [i0, i0 + 16) as 32 bits, first base on top.  i0 >= 0; bytes at or past `pbytes` read as 0 (their
// bases lie past the record and are not stored).
__device__ __forceinline__ uint32_t tb_bits16(const uint8_t *__restrict__ packed, int64_t pbytes, int64_t i0)
{
    const int64_t b0 = i0 >> 2;
    const int sh = (int)(i0 & 3);
    if (sh == 0 && b0 + 4 <= pbytes && (((uintptr_t)(packed + b0)) & 3) == 0)
        return __builtin_bswap32(*(const uint32_t *)(packed + b0));
    uint64_t w = 0;
    for (int k = 0; k < 5; ++k) w = (w << 8) | (uint64_t)(b0 + k < pbytes ? packed[b0 + k] : 0);
    return (uint32_t)(w >> (8 - 2 * sh));
}

// ---- packed bases -> class indices.  Lane: one 16-byte aligned word of the index buffer, clipped to the record.
__global__ void __launch_bounds__(256) twobit_encode_kernel(const uint8_t *__restrict__ file, const int64_t *__restrict__ tab, int64_t nrec,
                                                            const int64_t *__restrict__ niv, uint8_t *__restrict__ idx)
{
    __shared__ int64_t s_rec, s_lo, s_hi;
    const int64_t *poff = tab, *dna = tab + nrec, *ooff = tab + 2 * nrec, *ivoff = tab + 3 * nrec, *wg0 = tab + 4 * nrec + 1;
    const int64_t w = blockIdx.x;
    if (threadIdx.x == 0) {
        const int64_t r = dgrp_record_of(wg0, nrec, w);
        const int64_t n = dna[r];
        const int64_t o = (int64_t)((uintptr_t)(idx + ooff[r]) & 15);          // the record starts `o` bytes into its first word
        int64_t b0 = (w - wg0[r]) * TB_SPAN - o, b1 = b0 + TB_SPAN;               // bases of this workgroup
        b0 = b0 < 0 ? 0 : b0;
        b1 = b1 > n ? n : b1;
        s_rec = r;
        s_lo = tb_first_ending_after(niv, ivoff[r], ivoff[r + 1], b0);
        s_hi = tb_first_starting_from(niv, s_lo, ivoff[r + 1], b1);
    }
    __syncthreads();
    const int64_t r = s_rec, lo_iv = s_lo, hi_iv = s_hi;
    const int64_t n = dna[r];
    const uint8_t *packed = file + poff[r];
    const int64_t pbytes = (n + 3) >> 2;
    uint8_t *out = idx + ooff[r];
    const int64_t o = (int64_t)((uintptr_t)out & 15);
    for (int it = 0; it < TB_ITER; ++it) {
        // word `g` of the record covers bases [ib, ib + 16), of which [a, e) exist
        const int64_t g = (w - wg0[r]) * TB_WORDS + it * 256 + threadIdx.x;
        const int64_t ib = g * TB_LANE - o;
        const int64_t a = ib < 0 ? 0 : ib, e = ib + TB_LANE < n ? ib + TB_LANE : n;
        if (a >= e) continue;
        const bool full = a == ib && e == ib + TB_LANE;
        uint32_t c[4];
        if (full) {
            const uint32_t bits = tb_bits16(packed, pbytes, ib);
            c[0] = tb_codes4(bits >> 24);
            c[1] = tb_codes4((bits >> 16) & 0xffu);
            c[2] = tb_codes4((bits >> 8) & 0xffu);
            c[3] = tb_codes4(bits & 0xffu);
        } else {
            c[0] = c[1] = c[2] = c[3] = 0;
#pragma unroll
            for (int j = 0; j < TB_LANE; ++j) {
                const int64_t i = ib + j;
                if (i >= a && i < e) c[j >> 2] |= tb_code1(packed, i) << (8 * (j & 3));
            }
        }
        if (lo_iv < hi_iv) {
            // bases inside an N block are N whatever their two bits say
            for (int64_t k = tb_first_ending_after(niv, lo_iv, hi_iv, a); k < hi_iv; ++k) {
                const int64_t s = niv[2 * k], t = niv[2 * k + 1];
                if (s >= e) break;
                const int js = (int)((s > a ? s : a) - ib), je = (int)((t < e ? t : e) - ib);
#pragma unroll
                for (int j = 0; j < TB_LANE; ++j)
                    if (j >= js && j < je) c[j >> 2] = (c[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (4u << (8 * (j & 3)));
            }
        }
        if (full) {
            *(uint4 *)(out + ib) = make_uint4(c[0], c[1], c[2], c[3]);
        } else {
#pragma unroll
            for (int j = 0; j < TB_LANE; ++j) {
                const int64_t i = ib + j;
                if (i >= a && i < e) out[i] = (uint8_t)(c[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
}

struct tb_text_rec {                            // one record of dgrp_twobit_text_batch, as the kernel reads it
    int64_t name_off, name_len, poff, dna, toff, nlo, nhi, mlo, mhi, wg0;
};

// text bytes of a record: '>' name LF, then TB_LINE bases and LF per line
__host__ __device__ static inline int64_t tb_text_bytes(int64_t name_len, int64_t dna)
{
    return 2 + name_len + dna + (dna + TB_LINE - 1) / TB_LINE;
}

// bases in front of position `qb` of a record's body text (a line feed counts as the end of its line)
__device__ __forceinline__ int64_t tb_bases_before(int64_t qb)
{
    return qb <= 0 ? 0 : qb - qb / (TB_LINE + 1);
}

// ---- packed bases -> FASTA text.  Lane: one 16-byte aligned word of the text buffer, clipped to the record's text.
__global__ void __launch_bounds__(256) twobit_text_kernel(const uint8_t *__restrict__ file, const tb_text_rec *__restrict__ recs,
                                                          const int64_t *__restrict__ wg0, int64_t nrec, const int64_t *__restrict__ niv,
                                                          const int64_t *__restrict__ miv, uint8_t *__restrict__ text)
{
    __shared__ int64_t s_rec, s_nlo, s_nhi, s_mlo, s_mhi;
    const int64_t w = blockIdx.x;
    if (threadIdx.x == 0) {
        const int64_t r = dgrp_record_of(wg0, nrec, w);
        const tb_text_rec R = recs[r];
        const int64_t o = (int64_t)((uintptr_t)(text + R.toff) & 15);
        const int64_t hdr = R.name_len + 2;
        const int64_t q0 = (w - R.wg0) * TB_SPAN - o;
        int64_t b0 = tb_bases_before(q0 - hdr), b1 = tb_bases_before(q0 + TB_SPAN - hdr);
        b1 = b1 > R.dna ? R.dna : b1;
        s_rec = r;
        s_nlo = tb_first_ending_after(niv, R.nlo, R.nhi, b0);
        s_nhi = tb_first_starting_from(niv, s_nlo, R.nhi, b1);
        s_mlo = tb_first_ending_after(miv, R.mlo, R.mhi, b0);
        s_mhi = tb_first_starting_from(miv, s_mlo, R.mhi, b1);
    }
    __syncthreads();
    const tb_text_rec R = recs[s_rec];
    const uint8_t *packed = file + R.poff, *name = file + R.name_off;
    const int64_t pbytes = (R.dna + 3) >> 2;
    const int64_t hdr = R.name_len + 2, total = tb_text_bytes(R.name_len, R.dna);
    uint8_t *out = text + R.toff;
    const int64_t o = (int64_t)((uintptr_t)out & 15);
    for (int it = 0; it < TB_ITER; ++it) {
        const int64_t g = (w - R.wg0) * TB_WORDS + it * 256 + threadIdx.x;
        const int64_t qw = g * TB_LANE - o;                              // text position of the word's first byte
        const int64_t a = qw < 0 ? 0 : qw, e = qw + TB_LANE < total ? qw + TB_LANE : total;
        if (a >= e) continue;
        // the bases of this word: [i0, i0 + 16) at most, their packed bits first base on top
        const int64_t i0 = tb_bases_before(a - hdr);
        const uint32_t bits = i0 < R.dna ? tb_bits16(packed, pbytes, i0) : 0u;
        tb_cursor nc, mc;
        nc.seek(niv, s_nlo, s_nhi, i0);
        mc.seek(miv, s_mlo, s_mhi, i0);
        int64_t qb = a - hdr;                                            // position in the body text (negative: header line)
        int col = qb > 0 ? (int)(qb % (TB_LINE + 1)) : 0;
        int64_t i = i0;
        uint32_t c[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int j = 0; j < TB_LANE; ++j) {
            const int64_t q = qw + j;
            if (q < a || q >= e) continue;
            uint32_t ch;
            if (qb < 0) {
                ch = q == 0 ? (uint32_t)'>' : q == hdr - 1 ? (uint32_t)'\n' : (uint32_t)name[q - 1];
            } else if (col == TB_LINE || q == total - 1) {
                ch = '\n';
                col = -1;
            } else {
                const uint32_t v = (bits >> (30 - 2 * (int)(i - i0))) & 3u;
                ch = nc.covers(i) ? (uint32_t)'N' : (0x47414354u >> (8 * v)) & 0xffu;      // "TCAG"
                if (mc.covers(i)) ch |= 0x20u;
                ++i;
            }
            if (qb >= 0) ++col;
            ++qb;
            c[j >> 2] |= ch << (8 * (j & 3));
        }
        if (a == qw && e == qw + TB_LANE) {
            *(uint4 *)(out + qw) = make_uint4(c[0], c[1], c[2], c[3]);
        } else {
#pragma unroll
            for (int j = 0; j < TB_LANE; ++j) {
                const int64_t q = qw + j;
                if (q >= a && q < e) out[q] = (uint8_t)(c[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
}

// 16-byte words a range of `len` bytes at address `addr` touches, in workgroups
static inline int64_t tb_workgroups(uintptr_t addr, int64_t len)
{
    if (len <= 0) return 0;
    const int64_t words = (int64_t)(((addr & 15) + (uint64_t)len + 15) >> 4);
    return (words + TB_WORDS - 1) / TB_WORDS;
}

static bool tb_offsets_ok(const int64_t *off, int64_t nrec, int64_t count)
{
    if (off[0] < 0 || off[nrec] > count) return false;
    for (int64_t r = 0; r < nrec; ++r)
        if (off[r] > off[r + 1]) return false;
    return true;
}

}  // namespace

DGRP_EXPORT int64_t dgrp_twobit_workspace_bytes(int64_t nrec)
{
    if (nrec < 0) return 0;
    return dgrp_align_up((int64_t)sizeof(tb_text_rec) * nrec + 8 * (nrec + 1), 256);
}

DGRP_EXPORT int dgrp_twobit_encode_batch(const uint8_t *d_file, int64_t file_bytes, int64_t nrec, const int64_t *h_packed_off,
                                         const int64_t *h_dna_size, const int64_t *d_n_iv, const int64_t *h_n_iv_off, int64_t n_iv,
                                         const int64_t *h_out_off, uint8_t *d_idx, int64_t idx_cap, void *d_work, int64_t work_bytes,
                                         void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(nrec >= 0 && file_bytes >= 0 && n_iv >= 0 && idx_cap >= 0, "dgrp_twobit_encode_batch: negative size");
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_packed_off && h_dna_size && h_n_iv_off && h_out_off, "dgrp_twobit_encode_batch: NULL host table");
    DGRP_REQUIRE(tb_offsets_ok(h_n_iv_off, nrec, n_iv), "dgrp_twobit_encode_batch: h_n_iv_off is not ascending inside [0, %lld]", (long long)n_iv);
    DGRP_REQUIRE(h_n_iv_off[nrec] == h_n_iv_off[0] || d_n_iv, "dgrp_twobit_encode_batch: intervals without d_n_iv");
    std::vector<int64_t> tab((size_t)(5 * nrec + 2));
    int64_t *poff = tab.data(), *dna = poff + nrec, *ooff = dna + nrec, *ivoff = ooff + nrec, *wg0 = ivoff + nrec + 1;
    wg0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        const int64_t n = h_dna_size[r], p = h_packed_off[r], o = h_out_off[r];
        DGRP_REQUIRE(n >= 0 && n <= 0xffffffffll, "dgrp_twobit_encode_batch: record %lld: dnaSize %lld", (long long)r, (long long)n);
        DGRP_REQUIRE(p >= 0 && p <= file_bytes && (n + 3) / 4 <= file_bytes - p,
                     "dgrp_twobit_encode_batch: record %lld: packed bytes [%lld, +%lld) leave the file of %lld bytes", (long long)r,
                     (long long)p, (long long)((n + 3) / 4), (long long)file_bytes);
        DGRP_REQUIRE(o >= 0 && o <= idx_cap && n <= idx_cap - o,
                     "dgrp_twobit_encode_batch: record %lld: indices [%lld, +%lld) leave the buffer of %lld bytes", (long long)r,
                     (long long)o, (long long)n, (long long)idx_cap);
        poff[r] = p; dna[r] = n; ooff[r] = o; ivoff[r] = h_n_iv_off[r];
        wg0[r + 1] = wg0[r] + tb_workgroups((uintptr_t)d_idx + (uintptr_t)o, n);
    }
    ivoff[nrec] = h_n_iv_off[nrec];
    const int64_t nwg = wg0[nrec];
    if (nwg == 0) return DGRP_OK;
    DGRP_REQUIRE(d_file && d_idx && d_work, "dgrp_twobit_encode_batch: NULL device pointer");
    DGRP_REQUIRE(nwg <= 0x7fffffffll, "dgrp_twobit_encode_batch: %lld workgroups in one call", (long long)nwg);
    if (work_bytes < dgrp_twobit_workspace_bytes(nrec)) {
        dgrp_set_error("dgrp_twobit_encode_batch: workspace %lld < %lld bytes", (long long)work_bytes, (long long)dgrp_twobit_workspace_bytes(nrec));
        return DGRP_ENOMEM;
    }
    // (a pageable source: the copy has left `tab` when the call returns)
    DGRP_HIP(hipMemcpyAsync(d_work, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(twobit_encode_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, d_file, (const int64_t *)d_work, nrec, d_n_iv, d_idx);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_twobit_text_batch(const uint8_t *d_file, int64_t file_bytes, int64_t nrec, const int64_t *h_name_off,
                                       const int64_t *h_name_len, const int64_t *h_packed_off, const int64_t *h_dna_size,
                                       const int64_t *d_n_iv, const int64_t *h_n_iv_off, int64_t n_iv, const int64_t *d_m_iv,
                                       const int64_t *h_m_iv_off, int64_t m_iv, const int64_t *h_text_off, uint8_t *d_text,
                                       int64_t text_cap, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(nrec >= 0 && file_bytes >= 0 && n_iv >= 0 && m_iv >= 0 && text_cap >= 0, "dgrp_twobit_text_batch: negative size");
    if (nrec == 0) return DGRP_OK;
    DGRP_REQUIRE(h_name_off && h_name_len && h_packed_off && h_dna_size && h_n_iv_off && h_m_iv_off && h_text_off,
                 "dgrp_twobit_text_batch: NULL host table");
    DGRP_REQUIRE(tb_offsets_ok(h_n_iv_off, nrec, n_iv), "dgrp_twobit_text_batch: h_n_iv_off is not ascending inside [0, %lld]", (long long)n_iv);
    DGRP_REQUIRE(tb_offsets_ok(h_m_iv_off, nrec, m_iv), "dgrp_twobit_text_batch: h_m_iv_off is not ascending inside [0, %lld]", (long long)m_iv);
    DGRP_REQUIRE(h_n_iv_off[nrec] == h_n_iv_off[0] || d_n_iv, "dgrp_twobit_text_batch: intervals without d_n_iv");
    DGRP_REQUIRE(h_m_iv_off[nrec] == h_m_iv_off[0] || d_m_iv, "dgrp_twobit_text_batch: intervals without d_m_iv");
    const size_t rec_bytes = sizeof(tb_text_rec) * (size_t)nrec;
    std::vector<char> tab(rec_bytes + 8 * (size_t)(nrec + 1));
    tb_text_rec *recs = (tb_text_rec *)tab.data();
    int64_t *wg0 = (int64_t *)(tab.data() + rec_bytes);
    wg0[0] = 0;
    for (int64_t r = 0; r < nrec; ++r) {
        const int64_t n = h_dna_size[r], p = h_packed_off[r], o = h_text_off[r], no = h_name_off[r], nl = h_name_len[r];
        DGRP_REQUIRE(n >= 0 && n <= 0xffffffffll, "dgrp_twobit_text_batch: record %lld: dnaSize %lld", (long long)r, (long long)n);
        DGRP_REQUIRE(nl >= 0 && nl <= 255 && no >= 0 && no <= file_bytes && nl <= file_bytes - no,
                     "dgrp_twobit_text_batch: record %lld: name [%lld, +%lld) leaves the file of %lld bytes", (long long)r, (long long)no,
                     (long long)nl, (long long)file_bytes);
        DGRP_REQUIRE(p >= 0 && p <= file_bytes && (n + 3) / 4 <= file_bytes - p,
                     "dgrp_twobit_text_batch: record %lld: packed bytes [%lld, +%lld) leave the file of %lld bytes", (long long)r,
                     (long long)p, (long long)((n + 3) / 4), (long long)file_bytes);
        const int64_t len = tb_text_bytes(nl, n);
        DGRP_REQUIRE(o >= 0 && o <= text_cap && len <= text_cap - o,
                     "dgrp_twobit_text_batch: record %lld: text [%lld, +%lld) leaves the buffer of %lld bytes", (long long)r, (long long)o,
                     (long long)len, (long long)text_cap);
        tb_text_rec &R = recs[r];
        R.name_off = no; R.name_len = nl; R.poff = p; R.dna = n; R.toff = o;
        R.nlo = h_n_iv_off[r]; R.nhi = h_n_iv_off[r + 1]; R.mlo = h_m_iv_off[r]; R.mhi = h_m_iv_off[r + 1];
        R.wg0 = wg0[r];
        wg0[r + 1] = wg0[r] + tb_workgroups((uintptr_t)d_text + (uintptr_t)o, len);
    }
    const int64_t nwg = wg0[nrec];
    DGRP_REQUIRE(d_file && d_text && d_work, "dgrp_twobit_text_batch: NULL device pointer");
    DGRP_REQUIRE(nwg <= 0x7fffffffll, "dgrp_twobit_text_batch: %lld workgroups in one call", (long long)nwg);
    if (work_bytes < dgrp_twobit_workspace_bytes(nrec)) {
        dgrp_set_error("dgrp_twobit_text_batch: workspace %lld < %lld bytes", (long long)work_bytes, (long long)dgrp_twobit_workspace_bytes(nrec));
        return DGRP_ENOMEM;
    }
    // (a pageable source: the copy has left `tab` when the call returns)
    DGRP_HIP(hipMemcpyAsync(d_work, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(twobit_text_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, d_file, (const tb_text_rec *)d_work,
                       (const int64_t *)((const char *)d_work + rec_bytes), nrec, d_n_iv, d_m_iv, d_text);
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
