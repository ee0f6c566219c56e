// DEFLATE (RFC 1951) encode core for BGZF output, written once for the host and the device: integer arithmetic only, so that
// deflate_kernels.hip and dgrp_bgzf_compress_host produce the same bytes.
//
// A member (at most DGRP_BGZF_BLOCK input bytes) becomes ONE block of literals and the end-of-block symbol, no matches:
//   * byte histogram, end-of-block counted once (so a member has at least two used symbols and its code is complete);
//   * optimal code lengths from the symbols sorted by (count, value), in place (Moffat & Katajainen, "In-place calculation of
//     minimum-redundancy codes", 1995), then limited to 15 bits on the per-length counts: lengths above the limit are folded onto
//     it, and while the Kraft sum exceeds one a code of the limit is dropped and the longest shorter code is split in two
//     (zlib's overflow repair stated on counts); the lengths are then handed out again by frequency, so the code stays complete
//     and the most frequent symbols keep the shortest codes;
//   * the dynamic header: HLIT = 257 codes, HDIST = one distance code of length 0, the lengths run-length coded with 16/17/18
//     (greedy: zero runs as 18 then 17, other runs as the value then 16s), their code limited to 7 bits the same way;
//   * a stored block instead when its 5 + n bytes are not more than the dynamic block, hence a member never exceeds n + 31 bytes;
//   * the BGZF frame as bgzip writes it: 18-byte header with BC / BSIZE, the block, CRC-32, ISIZE.
//
// The plan (everything but the body's bits) is serial and small; the body is a table lookup per byte at a bit offset that is a
// prefix sum of code lengths -- the host walks it, the device scans it (deflate_kernels.hip).  Bits from word 4 of the member on
// are kept in 32-bit little-endian words: bits 0..15 of that word are BSIZE, the block starts at bit 16.
#pragma once
#include <stdint.h>

#include "crc32.h"

#define DGRP_BGZF_BLOCK 0xff00                    // input bytes per member, as bgzip takes them
#define DGRP_BGZF_SLOT (DGRP_BGZF_BLOCK + 32)     // a member never exceeds n + 31 bytes; rounded to 16
#define DGRP_BGZF_EOF_BYTES 28
#define DGRP_DEFLATE_NSYM 257                     // literals and end-of-block
#define DGRP_DEFLATE_HDR_WORDS 64                 // 16 + 3 + 14 + 19 * 3 + 258 * 7 + 12 bits at most
#define DGRP_DEFLATE_MAXBITS 15
#define DGRP_DEFLATE_CL_MAXBITS 7

struct dgrp_deflate_plan {
    uint32_t freq[DGRP_DEFLATE_NSYM];             // in: byte counts, freq[256] = 1
    uint16_t order[DGRP_DEFLATE_NSYM];            // in: the used symbols ascending by (count, value)  (dgrp_deflate_place)
    uint32_t table[DGRP_DEFLATE_NSYM];            // out: bit-reversed code | length << 16 per symbol
    uint32_t hdr[DGRP_DEFLATE_HDR_WORDS];         // out: BSIZE and the block header (stored: 01, LEN, NLEN), from word 4 of the member
    uint32_t hdr_end;                             // out: bits of hdr in use = where the body starts
    uint32_t stored;                              // out: 1 = stored block
    uint32_t deflate_bytes;                       // out: bytes of the block
    // scratch
    uint32_t work[DGRP_DEFLATE_NSYM];
    uint16_t count[DGRP_DEFLATE_MAXBITS + 2], next[DGRP_DEFLATE_MAXBITS + 2];
    uint8_t len[DGRP_DEFLATE_NSYM + 1];           // code length per symbol, then the one distance length (0)
    uint8_t tok_sym[DGRP_DEFLATE_NSYM + 1], tok_extra[DGRP_DEFLATE_NSYM + 1];
    uint32_t cl_freq[19];
    uint16_t cl_order[19];
    uint8_t cl_len[19];
    uint16_t cl_code[19];
};

// the member's first 16 bytes as little-endian words: 1f 8b 08 04 | MTIME 0 | XFL 0, OS ff, XLEN 6 | 'B' 'C' SLEN 2
DGRP_HD static inline uint32_t dgrp_bgzf_head_word(int k)
{
    return k == 0 ? 0x04088b1fu : k == 1 ? 0u : k == 2 ? 0x0006ff00u : 0x00024342u;
}
// order of the code length code lengths (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
DGRP_HD static inline int dgrp_deflate_clen_order(int i)
{
    if (i < 3) return 16 + i;
    if (i == 3) return 0;
    const int k = (i - 4) >> 1;
    return (i & 1) ? 7 - k : 8 + k;
}

// order[rank of sym among the used symbols by (count, value)] = sym: independent per symbol (one thread each on the device)
DGRP_HD static inline void dgrp_deflate_place(dgrp_deflate_plan *p, int sym)
{
    const uint32_t f = p->freq[sym];
    if (f == 0) return;
    int rank = 0;
    for (int s = 0; s < DGRP_DEFLATE_NSYM; ++s) {
        const uint32_t g = p->freq[s];
        rank += (g != 0) & ((g < f) | ((g == f) & (s < sym)));
    }
    p->order[rank] = (uint16_t)sym;
}

// Code lengths of the n >= 2 symbols order[0..n) (ascending by freq) limited to maxbits -> len[symbol]; count[l] = codes of length l
DGRP_HD static void dgrp_deflate_lengths(const uint32_t *freq, const uint16_t *order, int n, int maxbits, uint32_t *A, uint16_t *count,
                                         uint8_t *len)
{
    for (int i = 0; i < n; ++i) A[i] = freq[order[i]];
    // Moffat & Katajainen: parents, then internal depths, then leaf depths, all in A
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int nxt = 1; nxt < n - 1; ++nxt) {
        if (leaf >= n || A[root] < A[leaf]) { A[nxt] = A[root]; A[root++] = (uint32_t)nxt; }
        else A[nxt] = A[leaf++];
        if (leaf >= n || (root < nxt && A[root] < A[leaf])) { A[nxt] += A[root]; A[root++] = (uint32_t)nxt; }
        else A[nxt] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int nxt = n - 3; nxt >= 0; --nxt) A[nxt] = A[A[nxt]] + 1;
    int avbl = 1, used = 0, dpth = 0, nxt = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[nxt--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    // the limit, on counts
    for (int l = 0; l <= maxbits; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[(int)A[i] < maxbits ? A[i] : maxbits]++;
    uint32_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += (uint32_t)count[l] << (maxbits - l);
    while (total > (1u << maxbits)) {
        count[maxbits]--;
        for (int l = maxbits - 1; l > 0; --l)
            if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        --total;
    }
    // rarest symbols take the longest codes
    int i = 0;
    for (int l = maxbits; l >= 1; --l)
        for (int c = count[l]; c > 0; --c) len[order[i++]] = (uint8_t)l;
}

DGRP_HD static inline uint32_t dgrp_bitrev(uint32_t c, int len)
{
    c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
    c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
    c = ((c & 0x0f0fu) << 4) | ((c >> 4) & 0x0f0fu);
    c = ((c & 0x00ffu) << 8) | ((c >> 8) & 0x00ffu);
    return c >> (16 - len);
}

// first canonical code of every length (RFC 1951 3.2.2) from count[]
DGRP_HD static inline void dgrp_deflate_next(const uint16_t *count, int maxbits, uint16_t *next)
{
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l <= maxbits; ++l) {
        code = (code + (l > 1 ? count[l - 1] : 0)) << 1;
        next[l] = (uint16_t)code;
    }
}

struct dgrp_bitput {
    uint32_t *w;
    uint32_t pos;
};
DGRP_HD static inline void dgrp_put(dgrp_bitput &b, uint32_t v, int k)      // k <= 16 bits of v, LSB first; the words start zeroed
{
    const uint32_t i = b.pos >> 5, s = b.pos & 31;
    b.w[i] |= v << s;
    if (s + (uint32_t)k > 32) b.w[i + 1] |= v >> (32 - s);
    b.pos += (uint32_t)k;
}

// Everything about the member of n bytes (1 <= n <= DGRP_BGZF_BLOCK) but its body bits, from freq[] and order[].
DGRP_HD static void dgrp_deflate_plan_member(dgrp_deflate_plan *p, uint32_t n)
{
    int nused = 0;
    for (int s = 0; s < DGRP_DEFLATE_NSYM; ++s) {
        nused += p->freq[s] != 0;
        p->len[s] = 0;
        p->table[s] = 0;
    }
    p->len[DGRP_DEFLATE_NSYM] = 0;                                   // the distance code
    dgrp_deflate_lengths(p->freq, p->order, nused, DGRP_DEFLATE_MAXBITS, p->work, p->count, p->len);
    dgrp_deflate_next(p->count, DGRP_DEFLATE_MAXBITS, p->next);
    uint32_t body_bits = 0;
    for (int s = 0; s < DGRP_DEFLATE_NSYM; ++s) {
        const int l = p->len[s];
        if (l == 0) continue;
        p->table[s] = dgrp_bitrev(p->next[l]++, l) | ((uint32_t)l << 16);
        body_bits += p->freq[s] * (uint32_t)l;
    }
    // the lengths as tokens of the code length alphabet
    for (int i = 0; i < 19; ++i) p->cl_freq[i] = 0, p->cl_len[i] = 0, p->cl_code[i] = 0;
    int ntok = 0;
    for (int i = 0; i <= DGRP_DEFLATE_NSYM;) {
        const int v = p->len[i];
        int run = 1;
        while (i + run <= DGRP_DEFLATE_NSYM && p->len[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                p->tok_sym[ntok] = 18, p->tok_extra[ntok++] = (uint8_t)(r - 11), run -= r;
            }
            if (run >= 3) p->tok_sym[ntok] = 17, p->tok_extra[ntok++] = (uint8_t)(run - 3), run = 0;
        } else {
            p->tok_sym[ntok] = (uint8_t)v, p->tok_extra[ntok++] = 0, --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                p->tok_sym[ntok] = 16, p->tok_extra[ntok++] = (uint8_t)(r - 3), run -= r;
            }
        }
        for (; run > 0; --run) p->tok_sym[ntok] = (uint8_t)v, p->tok_extra[ntok++] = 0;
    }
    for (int t = 0; t < ntok; ++t) p->cl_freq[p->tok_sym[t]]++;
    // their code: at least a length and a zero or zero-run symbol are in use, so it is complete as well
    int cl_used = 0;
    for (int s = 0; s < 19; ++s) {
        if (p->cl_freq[s] == 0) continue;
        int k = cl_used++;
        for (; k > 0 && p->cl_freq[p->cl_order[k - 1]] > p->cl_freq[s]; --k) p->cl_order[k] = p->cl_order[k - 1];
        p->cl_order[k] = (uint16_t)s;
    }
    dgrp_deflate_lengths(p->cl_freq, p->cl_order, cl_used, DGRP_DEFLATE_CL_MAXBITS, p->work, p->count, p->cl_len);
    dgrp_deflate_next(p->count, DGRP_DEFLATE_CL_MAXBITS, p->next);
    for (int s = 0; s < 19; ++s)
        if (p->cl_len[s]) p->cl_code[s] = (uint16_t)dgrp_bitrev(p->next[p->cl_len[s]]++, p->cl_len[s]);
    int hclen = 19;
    while (hclen > 4 && p->cl_len[dgrp_deflate_clen_order(hclen - 1)] == 0) --hclen;
    uint32_t hdr_bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int t = 0; t < ntok; ++t) {
        const int s = p->tok_sym[t];
        hdr_bits += p->cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    const uint32_t dyn_bytes = (hdr_bits + body_bits + 7) >> 3;
    p->stored = 5 + n <= dyn_bytes;
    p->deflate_bytes = p->stored ? 5 + n : dyn_bytes;
    for (int i = 0; i < DGRP_DEFLATE_HDR_WORDS; ++i) p->hdr[i] = 0;
    dgrp_bitput b{p->hdr, 0};
    dgrp_put(b, 18 + p->deflate_bytes + 8 - 1, 16);                  // BSIZE
    if (p->stored) {
        dgrp_put(b, 1, 8);                                           // BFINAL, BTYPE = 00, padding
        dgrp_put(b, n, 16);
        dgrp_put(b, ~n & 0xffffu, 16);
    } else {
        dgrp_put(b, 1, 1);
        dgrp_put(b, 2, 2);
        dgrp_put(b, 0, 5);                                           // HLIT: 257 codes
        dgrp_put(b, 0, 5);                                           // HDIST: 1 code
        dgrp_put(b, (uint32_t)hclen - 4, 4);
        for (int i = 0; i < hclen; ++i) dgrp_put(b, p->cl_len[dgrp_deflate_clen_order(i)], 3);
        for (int t = 0; t < ntok; ++t) {
            const int s = p->tok_sym[t];
            dgrp_put(b, p->cl_code[s], p->cl_len[s]);
            if (s >= 16) dgrp_put(b, p->tok_extra[t], s == 16 ? 2 : s == 17 ? 3 : 7);
        }
    }
    p->hdr_end = b.pos;
}

// One member of in[0, n), 1 <= n <= DGRP_BGZF_BLOCK, into slot[0, DGRP_BGZF_SLOT) (4-byte aligned; zeroed here), serially.
// Returns its size.
DGRP_HD static uint32_t dgrp_bgzf_member_serial(const uint8_t *in, uint32_t n, uint32_t *slot, dgrp_deflate_plan *p)
{
    for (int s = 0; s < DGRP_DEFLATE_NSYM; ++s) p->freq[s] = 0;
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) p->freq[in[i]]++;
    p->freq[256] = 1;
    for (int s = 0; s < DGRP_DEFLATE_NSYM; ++s) dgrp_deflate_place(p, s);
    dgrp_deflate_plan_member(p, n);
    const uint32_t total = 18 + p->deflate_bytes + 8;
    for (uint32_t i = 0; i < DGRP_BGZF_SLOT / 4; ++i) slot[i] = 0;
    uint8_t *bytes = (uint8_t *)slot;
    for (int i = 0; i < 4; ++i) slot[i] = dgrp_bgzf_head_word(i);
    const uint32_t hw = (p->hdr_end + 31) >> 5;
    for (uint32_t i = 0; i < hw; ++i) slot[4 + i] = p->hdr[i];
    if (p->stored) {
        for (uint32_t i = 0; i < n; ++i) bytes[23 + i] = in[i];
    } else {
        dgrp_bitput b{slot + 4, p->hdr_end};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t e = p->table[in[i]];
            dgrp_put(b, e & 0xffffu, (int)(e >> 16));
        }
        const uint32_t e = p->table[256];
        dgrp_put(b, e & 0xffffu, (int)(e >> 16));
    }
    for (uint32_t i = 0; i < n; ++i) crc = dgrp_crc_table_entry((crc ^ in[i]) & 0xff) ^ (crc >> 8);
    crc ^= 0xffffffffu;
    uint8_t *t = bytes + 18 + p->deflate_bytes;
    for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(crc >> (8 * k)), t[4 + k] = (uint8_t)(n >> (8 * k));
    return total;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Level 1: the same member with matches.  The token sequence is a pure function of the member's bytes (no evaluation order in it):
//   * key(p)  = the 4 bytes at p hashed to DGRP_LZ_HASH_BITS bits, for p + 4 <= n;
//   * cand(p) = the largest q < p with key(q) == key(p) (the same bucket: the bytes themselves may differ);
//   * len(p)  = common prefix of the text at p and at cand(p), capped at 258 and at the member's end, and 0 when cand(p) lies more
//     than 32768 back; usable when >= 4; overlap (distance < length) is allowed;
//   * greedy parse: next(p) = p + len(p) if usable, else p + 1; the tokens are the positions reachable from 0.
// One block: a dynamic code over literals, end-of-block and length symbols and a dynamic distance code (a lone distance symbol gets
// a one-bit code), both from dgrp_deflate_lengths, the lengths of both run-length coded in one sequence.  The member is the smallest
// of level 0's block (stored or literals) and this one; on a tie level 0's.  The host walks the text, the device evaluates the same
// rule in parallel (deflate_kernels.hip): per position one word, len | (distance - 1) << 9, DGRP_LZ_TOKEN set on the parse's positions.
#define DGRP_LZ_HASH_BITS 15
#define DGRP_LZ_MIN 4
#define DGRP_LZ_MAX 258
#define DGRP_LZ_WINDOW 32768u
#define DGRP_LZ_NLIT 286
#define DGRP_LZ_NDIST 30
#define DGRP_LZ_NSYM (DGRP_LZ_NLIT + DGRP_LZ_NDIST)
#define DGRP_LZ_HDR_WORDS 96                      // 16 + 3 + 14 + 19 * 3 + 316 * 7 + 7 bits at most
#define DGRP_LZ_TOKEN 0x80000000u

DGRP_HD static inline uint32_t dgrp_lz_key(uint32_t four_bytes) { return (four_bytes * 2654435761u) >> (32 - DGRP_LZ_HASH_BITS); }
DGRP_HD static inline uint32_t dgrp_lz_len(uint32_t e) { return e & 0x1ffu; }
DGRP_HD static inline uint32_t dgrp_lz_dist(uint32_t e) { return ((e >> 9) & 0x7fffu) + 1; }
DGRP_HD static inline uint32_t dgrp_lz_step(uint32_t e) { return dgrp_lz_len(e) >= DGRP_LZ_MIN ? dgrp_lz_len(e) : 1u; }

// length 3..258 -> symbol 257..285 | extra bits << 16 | their value << 24
DGRP_HD static inline uint32_t dgrp_lz_len_sym(uint32_t len)
{
    if (len == 258) return 285;
    const uint32_t l = len - 3;
    if (l < 8) return 257 + l;
    const uint32_t eb = (uint32_t)(31 - __builtin_clz(l)) - 2;
    return (257 + 4 * (eb + 1) + ((l >> eb) & 3u)) | (eb << 16) | ((l & ((1u << eb) - 1)) << 24);
}
// distance 1..32768 -> symbol 0..29 | extra bits << 8 | their value << 16
DGRP_HD static inline uint32_t dgrp_lz_dist_sym(uint32_t dist)
{
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t hb = (uint32_t)(31 - __builtin_clz(d)), eb = hb - 1;
    return (2 * hb + ((d >> eb) & 1u)) | (eb << 8) | ((d & ((1u << eb) - 1)) << 16);
}
DGRP_HD static inline uint32_t dgrp_lz_len_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }
DGRP_HD static inline uint32_t dgrp_lz_dist_extra(uint32_t sym) { return sym < 4 ? 0u : (sym - 2) >> 1; }

struct dgrp_lz_plan {
    uint32_t freq[DGRP_LZ_NSYM];                  // in: literal/length counts (freq[256] = 1), then the distance counts
    uint16_t order[DGRP_LZ_NSYM];                 // in: the used symbols of either code ascending by (count, value)  (dgrp_lz_place)
    uint32_t table[DGRP_LZ_NSYM];                 // out: bit-reversed code | length << 16 per symbol
    uint32_t hdr[DGRP_LZ_HDR_WORDS];              // out: BSIZE and the block header
    uint32_t hdr_end;
    uint32_t usable;                              // out: 1 = there are matches (else level 0's block is the member)
    uint32_t deflate_bytes;                       // out: bytes of the block
    // scratch
    uint32_t work[DGRP_LZ_NLIT];
    uint16_t count[DGRP_DEFLATE_MAXBITS + 2], next[DGRP_DEFLATE_MAXBITS + 2];
    uint8_t len[DGRP_LZ_NSYM];
    uint8_t tok_sym[DGRP_LZ_NSYM], tok_extra[DGRP_LZ_NSYM];
    uint32_t cl_freq[19];
    uint16_t cl_order[19];
    uint8_t cl_len[19];
    uint16_t cl_code[19];
};

// order[rank of sym among the used symbols of its own code] = sym - base, for sym in [base, base + nsym): independent per symbol
DGRP_HD static inline void dgrp_lz_place(dgrp_lz_plan *p, int sym)
{
    const int base = sym < DGRP_LZ_NLIT ? 0 : DGRP_LZ_NLIT, nsym = sym < DGRP_LZ_NLIT ? DGRP_LZ_NLIT : DGRP_LZ_NDIST;
    const uint32_t f = p->freq[sym];
    if (f == 0) return;
    int rank = 0;
    for (int s = base; s < base + nsym; ++s) {
        const uint32_t g = p->freq[s];
        rank += (g != 0) & ((g < f) | ((g == f) & (s < sym)));
    }
    p->order[base + rank] = (uint16_t)(sym - base);
}

// Everything about the level-1 block but its body bits, from freq[] and order[].
DGRP_HD static void dgrp_lz_plan_member(dgrp_lz_plan *p)
{
    int nlit = 0, ndist = 0, hlit = 257, hdist = 1;
    for (int s = 0; s < DGRP_LZ_NSYM; ++s) {
        p->len[s] = 0;
        p->table[s] = 0;
        if (p->freq[s] == 0) continue;
        if (s < DGRP_LZ_NLIT) ++nlit, hlit = s + 1 > hlit ? s + 1 : hlit;
        else ++ndist, hdist = s - DGRP_LZ_NLIT + 1;
    }
    p->usable = ndist > 0;
    p->hdr_end = 0;
    p->deflate_bytes = 0;
    if (!p->usable) return;
    uint32_t body_bits = 0;
    dgrp_deflate_lengths(p->freq, p->order, nlit, DGRP_DEFLATE_MAXBITS, p->work, p->count, p->len);
    dgrp_deflate_next(p->count, DGRP_DEFLATE_MAXBITS, p->next);
    for (int s = 0; s < DGRP_LZ_NLIT; ++s) {
        const int l = p->len[s];
        if (l == 0) continue;
        p->table[s] = dgrp_bitrev(p->next[l]++, l) | ((uint32_t)l << 16);
        body_bits += p->freq[s] * ((uint32_t)l + dgrp_lz_len_extra((uint32_t)s));
    }
    uint8_t *dlen = p->len + DGRP_LZ_NLIT;
    if (ndist == 1) {
        dlen[hdist - 1] = 1;                                         // a one-bit code, the bit is 0
        for (int l = 0; l <= DGRP_DEFLATE_MAXBITS; ++l) p->count[l] = l == 1;
    } else {
        dgrp_deflate_lengths(p->freq + DGRP_LZ_NLIT, p->order + DGRP_LZ_NLIT, ndist, DGRP_DEFLATE_MAXBITS, p->work, p->count, dlen);
    }
    dgrp_deflate_next(p->count, DGRP_DEFLATE_MAXBITS, p->next);
    for (int s = 0; s < DGRP_LZ_NDIST; ++s) {
        const int l = dlen[s];
        if (l == 0) continue;
        p->table[DGRP_LZ_NLIT + s] = dgrp_bitrev(p->next[l]++, l) | ((uint32_t)l << 16);
        body_bits += p->freq[DGRP_LZ_NLIT + s] * ((uint32_t)l + dgrp_lz_dist_extra((uint32_t)s));
    }
    // the lengths of both codes, hlit then hdist of them, as tokens of the code length alphabet
    for (int i = 0; i < 19; ++i) p->cl_freq[i] = 0, p->cl_len[i] = 0, p->cl_code[i] = 0;
    const int nall = hlit + hdist;
    int ntok = 0;
    for (int i = 0; i < nall;) {
        const int v = p->len[i < hlit ? i : i - hlit + DGRP_LZ_NLIT];
        int run = 1;
        while (i + run < nall && p->len[i + run < hlit ? i + run : i + run - hlit + DGRP_LZ_NLIT] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                p->tok_sym[ntok] = 18, p->tok_extra[ntok++] = (uint8_t)(r - 11), run -= r;
            }
            if (run >= 3) p->tok_sym[ntok] = 17, p->tok_extra[ntok++] = (uint8_t)(run - 3), run = 0;
        } else {
            p->tok_sym[ntok] = (uint8_t)v, p->tok_extra[ntok++] = 0, --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                p->tok_sym[ntok] = 16, p->tok_extra[ntok++] = (uint8_t)(r - 3), run -= r;
            }
        }
        for (; run > 0; --run) p->tok_sym[ntok] = (uint8_t)v, p->tok_extra[ntok++] = 0;
    }
    for (int t = 0; t < ntok; ++t) p->cl_freq[p->tok_sym[t]]++;
    int cl_used = 0;
    for (int s = 0; s < 19; ++s) {
        if (p->cl_freq[s] == 0) continue;
        int k = cl_used++;
        for (; k > 0 && p->cl_freq[p->cl_order[k - 1]] > p->cl_freq[s]; --k) p->cl_order[k] = p->cl_order[k - 1];
        p->cl_order[k] = (uint16_t)s;
    }
    if (cl_used == 1) {
        p->cl_len[p->cl_order[0]] = 1;                               // (every length equal and no run symbol: cannot happen with
        for (int l = 0; l <= DGRP_DEFLATE_CL_MAXBITS; ++l) p->count[l] = l == 1;   //  end-of-block's code beside a byte's, kept total)
    } else {
        dgrp_deflate_lengths(p->cl_freq, p->cl_order, cl_used, DGRP_DEFLATE_CL_MAXBITS, p->work, p->count, p->cl_len);
    }
    dgrp_deflate_next(p->count, DGRP_DEFLATE_CL_MAXBITS, p->next);
    for (int s = 0; s < 19; ++s)
        if (p->cl_len[s]) p->cl_code[s] = (uint16_t)dgrp_bitrev(p->next[p->cl_len[s]]++, p->cl_len[s]);
    int hclen = 19;
    while (hclen > 4 && p->cl_len[dgrp_deflate_clen_order(hclen - 1)] == 0) --hclen;
    uint32_t hdr_bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int t = 0; t < ntok; ++t) {
        const int s = p->tok_sym[t];
        hdr_bits += p->cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    p->deflate_bytes = (hdr_bits + body_bits + 7) >> 3;
    for (int i = 0; i < DGRP_LZ_HDR_WORDS; ++i) p->hdr[i] = 0;
    dgrp_bitput b{p->hdr, 0};
    dgrp_put(b, 18 + p->deflate_bytes + 8 - 1, 16);                  // BSIZE (of a block that is only used when it is the smaller)
    dgrp_put(b, 1, 1);
    dgrp_put(b, 2, 2);
    dgrp_put(b, (uint32_t)hlit - 257, 5);
    dgrp_put(b, (uint32_t)hdist - 1, 5);
    dgrp_put(b, (uint32_t)hclen - 4, 4);
    for (int i = 0; i < hclen; ++i) dgrp_put(b, p->cl_len[dgrp_deflate_clen_order(i)], 3);
    for (int t = 0; t < ntok; ++t) {
        const int s = p->tok_sym[t];
        dgrp_put(b, p->cl_code[s], p->cl_len[s]);
        if (s >= 16) dgrp_put(b, p->tok_extra[t], s == 16 ? 2 : s == 17 ? 3 : 7);
    }
    p->hdr_end = b.pos;
}

// the member is level 1's block when it is strictly smaller than level 0's
DGRP_HD static inline bool dgrp_lz_wins(const dgrp_lz_plan *z, const dgrp_deflate_plan *p)
{
    return z->usable && z->deflate_bytes < p->deflate_bytes;
}

// The bits of the token at a parse position: lo = the literal's or the length's code and extra bits (nlo of them), hi = the
// distance's (nhi; 0 for a literal).  byte = the text's byte there.
DGRP_HD static inline void dgrp_lz_token_bits(const uint32_t *table, uint32_t e, uint32_t byte, uint32_t &lo, uint32_t &nlo, uint32_t &hi,
                                              uint32_t &nhi)
{
    if (dgrp_lz_len(e) < DGRP_LZ_MIN) {
        const uint32_t t = table[byte];
        lo = t & 0xffffu, nlo = t >> 16, hi = 0, nhi = 0;
        return;
    }
    const uint32_t ls = dgrp_lz_len_sym(dgrp_lz_len(e)), ds = dgrp_lz_dist_sym(dgrp_lz_dist(e));
    const uint32_t tl = table[ls & 0xffffu], td = table[DGRP_LZ_NLIT + (ds & 0xffu)];
    lo = (tl & 0xffffu) | ((ls >> 24) << (tl >> 16)), nlo = (tl >> 16) + ((ls >> 16) & 0xffu);
    hi = (td & 0xffffu) | ((ds >> 16) << (td >> 16)), nhi = (td >> 16) + ((ds >> 8) & 0xffu);
}

// Level 1's statement: one member of in[0, n) into slot, serially; lz[0, n) and head[0, 1 << DGRP_LZ_HASH_BITS) are scratch.
DGRP_HD static uint32_t dgrp_bgzf_member_serial_lz(const uint8_t *in, uint32_t n, uint32_t *slot, dgrp_deflate_plan *p, dgrp_lz_plan *z,
                                                   uint32_t *lz, uint16_t *head)
{
    for (uint32_t k = 0; k < (1u << DGRP_LZ_HASH_BITS); ++k) head[k] = 0xffffu;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t e = 0;
        if (i + 4 <= n) {
            const uint32_t key = dgrp_lz_key((uint32_t)in[i] | ((uint32_t)in[i + 1] << 8) | ((uint32_t)in[i + 2] << 16) | ((uint32_t)in[i + 3] << 24));
            const uint32_t q = head[key];
            head[key] = (uint16_t)i;
            if (q != 0xffffu && i - q <= DGRP_LZ_WINDOW) {
                const uint32_t cap = n - i < DGRP_LZ_MAX ? n - i : DGRP_LZ_MAX;
                uint32_t l = 0;
                while (l < cap && in[q + l] == in[i + l]) ++l;
                e = l | ((i - q - 1) << 9);
            }
        }
        lz[i] = e;
    }
    for (int s = 0; s < DGRP_LZ_NSYM; ++s) z->freq[s] = 0;
    for (uint32_t i = 0; i < n; i += dgrp_lz_step(lz[i])) {
        lz[i] |= DGRP_LZ_TOKEN;
        if (dgrp_lz_len(lz[i]) < DGRP_LZ_MIN) z->freq[in[i]]++;
        else z->freq[dgrp_lz_len_sym(dgrp_lz_len(lz[i])) & 0xffffu]++, z->freq[DGRP_LZ_NLIT + (dgrp_lz_dist_sym(dgrp_lz_dist(lz[i])) & 0xffu)]++;
    }
    z->freq[256] = 1;
    for (int s = 0; s < DGRP_LZ_NSYM; ++s) dgrp_lz_place(z, s);
    dgrp_lz_plan_member(z);
    const uint32_t size0 = dgrp_bgzf_member_serial(in, n, slot, p);
    if (!dgrp_lz_wins(z, p)) return size0;
    const uint32_t total = 18 + z->deflate_bytes + 8;
    for (uint32_t i = 4; i < DGRP_BGZF_SLOT / 4; ++i) slot[i] = 0;
    const uint32_t hw = (z->hdr_end + 31) >> 5;
    for (uint32_t i = 0; i < hw; ++i) slot[4 + i] = z->hdr[i];
    dgrp_bitput b{slot + 4, z->hdr_end};
    for (uint32_t i = 0; i < n; i += dgrp_lz_step(lz[i])) {
        uint32_t lo, nlo, hi, nhi;
        dgrp_lz_token_bits(z->table, lz[i], in[i], lo, nlo, hi, nhi);
        dgrp_put(b, lo & 0xffffu, nlo < 16 ? (int)nlo : 16);
        if (nlo > 16) dgrp_put(b, lo >> 16, (int)nlo - 16);
        if (nhi) {
            dgrp_put(b, hi & 0xffffu, nhi < 16 ? (int)nhi : 16);
            if (nhi > 16) dgrp_put(b, hi >> 16, (int)nhi - 16);
        }
    }
    const uint32_t eob = z->table[256];
    dgrp_put(b, eob & 0xffffu, (int)(eob >> 16));
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) crc = dgrp_crc_table_entry((crc ^ in[i]) & 0xff) ^ (crc >> 8);
    crc ^= 0xffffffffu;
    uint8_t *t = (uint8_t *)slot + 18 + z->deflate_bytes;
    for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(crc >> (8 * k)), t[4 + k] = (uint8_t)(n >> (8 * k));
    return total;
}
