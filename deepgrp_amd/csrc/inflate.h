// DEFLATE (RFC 1951) decode core, written once for the host and the device.
//
// The decoder is serial (one symbol after the other, canonical Huffman decode one bit at a time against the per-length code
// counts, as RFC 1951 3.2.2 constructs the codes).  Where the output goes is a template parameter: the host writes bytes one by
// one; the device runs the same code on every lane of a wave (all lanes hold the same state) and spreads match and stored-block
// copies over the lanes (inflate_kernels.hip).
//
// Every read is checked against the input slice [0, in_len) and every write and back-reference against the output slice
// [0, out_cap): a bad stream ends with a DGRP_INFLATE_E* reason (include/deepgrp_hip.h), never with an access outside either slice.
#pragma once
#include <stdint.h>

#include "../../include/deepgrp_hip.h"

#include "crc32.h"   // DGRP_HD; the CRC-32 of the member trailers

#define DGRP_HUFF_MAXBITS 15

// one canonical code: count[len] = codes of that length, symbol[] = symbols ordered by (length, value)
struct dgrp_huff {
    int16_t count[DGRP_HUFF_MAXBITS + 1];
    int16_t symbol[288];
};

// per-stream tables (LDS on the device: 2 KB)
struct dgrp_inflate_tables {
    dgrp_huff lencode, distcode;
    int16_t lengths[288 + 32];
    int16_t offs[DGRP_HUFF_MAXBITS + 1];
    int fixed;                                   // the tables hold the fixed codes (rebuilt only when a dynamic block intervened)
};

struct dgrp_bits {
    const uint8_t *in;
    uint32_t len, pos;                           // input slice and the next byte to load into buf
    uint64_t buf;                                // bits not yet consumed, LSB first
    int cnt;
};

DGRP_HD static inline uint32_t dgrp_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

DGRP_HD static inline void dgrp_bits_refill(dgrp_bits &s)
{
    if (s.cnt <= 32 && s.pos + 4 <= s.len) {
        s.buf |= (uint64_t)dgrp_le32(s.in + s.pos) << s.cnt;
        s.cnt += 32;
        s.pos += 4;
    }
    while (s.cnt <= 56 && s.pos < s.len) {
        s.buf |= (uint64_t)s.in[s.pos++] << s.cnt;
        s.cnt += 8;
    }
}

// the reader at bit `skip` (0..7) of in[0, len)
DGRP_HD static inline void dgrp_bits_open(dgrp_bits &s, const uint8_t *in, uint32_t len, uint32_t skip)
{
    s.in = in;
    s.len = len;
    s.pos = 0;
    s.buf = 0;
    s.cnt = 0;
    if (skip) {
        dgrp_bits_refill(s);
        if (s.cnt >= (int)skip) {
            s.buf >>= skip;
            s.cnt -= (int)skip;
        }
    }
}
// the next bit not consumed, relative to the slice
DGRP_HD static inline int64_t dgrp_bits_tell(const dgrp_bits &s) { return (int64_t)s.pos * 8 - s.cnt; }

// n <= 16 bits; false when the input ends first
DGRP_HD static inline bool dgrp_bits_get(dgrp_bits &s, int n, uint32_t &v)
{
    if (s.cnt < n) {
        dgrp_bits_refill(s);
        if (s.cnt < n) return false;
    }
    v = (uint32_t)(s.buf & ((1ull << n) - 1));
    s.buf >>= n;
    s.cnt -= n;
    return true;
}

// Canonical code of lengths length[0..n): 0 = complete, > 0 = incomplete (codes left over), < 0 = over-subscribed.
// (always inline: left to itself the compiler keeps it as a call in some of the decoding kernels, and a kernel with a call in it
// takes more registers -- the member kernel 127 VGPRs against 103 and 1.7 % more time, count and symbols ~117 against 80)
DGRP_HD static inline __attribute__((always_inline)) int dgrp_huff_build(dgrp_huff *h, int16_t *offs, const int16_t *length, int n)
{
    for (int len = 0; len <= DGRP_HUFF_MAXBITS; ++len) h->count[len] = 0;
    for (int sym = 0; sym < n; ++sym) h->count[length[sym]]++;
    if (h->count[0] == n) return 0;              // no codes: decoding with it fails (ESYMBOL)
    int left = 1;
    for (int len = 1; len <= DGRP_HUFF_MAXBITS; ++len) {
        left <<= 1;
        left -= h->count[len];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < DGRP_HUFF_MAXBITS; ++len) offs[len + 1] = (int16_t)(offs[len] + h->count[len]);
    for (int sym = 0; sym < n; ++sym)
        if (length[sym] != 0) h->symbol[offs[length[sym]]++] = (int16_t)sym;
    return left;
}

// next symbol, or -reason
DGRP_HD static inline int dgrp_huff_decode(dgrp_bits &s, const dgrp_huff *h)
{
    if (s.cnt < DGRP_HUFF_MAXBITS) dgrp_bits_refill(s);
    uint64_t buf = s.buf;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= DGRP_HUFF_MAXBITS; ++len) {
        if (len > s.cnt) return -DGRP_INFLATE_EINPUT;
        code |= (int)(buf & 1);
        buf >>= 1;
        const int count = h->count[len];
        if (code - count < first) {
            s.buf >>= len;
            s.cnt -= len;
            return h->symbol[index + (code - first)];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -DGRP_INFLATE_ESYMBOL;                // a bit pattern no code of an incomplete set has
}

// RFC 1951 3.2.5 in closed form: base length / extra bits of length symbol i = sym - 257 (0..28), distance symbol d (0..29)
DGRP_HD static inline void dgrp_len_code(int i, int &base, int &extra)
{
    if (i < 8) { base = 3 + i; extra = 0; }
    else if (i == 28) { base = 258; extra = 0; }
    else { extra = (i - 4) >> 2; base = ((4 + (i & 3)) << extra) + 3; }
}
DGRP_HD static inline void dgrp_dist_code(int d, int &base, int &extra)
{
    if (d < 4) { base = d + 1; extra = 0; }
    else { extra = (d - 2) >> 1; base = ((2 + (d & 1)) << extra) + 1; }
}
// order of the code length code lengths (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
DGRP_HD static inline int dgrp_clen_order(int i)
{
    if (i < 3) return 16 + i;
    if (i == 3) return 0;
    const int k = (i - 4) >> 1;
    return (i & 1) ? 7 - k : 8 + k;
}

// A code set of a dynamic block may be incomplete only when it is a single code of one bit (RFC 1951 allows one distance code;
// zlib accepts the same for literal/length).
DGRP_HD static inline bool dgrp_code_ok(int err, const dgrp_huff *h, int n)
{
    return err == 0 || (err > 0 && n - h->count[0] == 1 && h->count[1] == 1);
}

DGRP_HD static int dgrp_read_dynamic(dgrp_bits &s, dgrp_inflate_tables *t)
{
    uint32_t nlen, ndist, ncode, v;
    if (!dgrp_bits_get(s, 5, nlen) || !dgrp_bits_get(s, 5, ndist) || !dgrp_bits_get(s, 4, ncode)) return DGRP_INFLATE_EINPUT;
    nlen += 257;
    ndist += 1;
    ncode += 4;
    if (nlen > 286 || ndist > 30) return DGRP_INFLATE_ECODES;
    for (int i = 0; i < 19; ++i) {
        v = 0;
        if (i < (int)ncode && !dgrp_bits_get(s, 3, v)) return DGRP_INFLATE_EINPUT;
        t->lengths[dgrp_clen_order(i)] = (int16_t)v;
    }
    if (dgrp_huff_build(&t->lencode, t->offs, t->lengths, 19) != 0) return DGRP_INFLATE_ECODES;   // must be complete
    const int total = (int)(nlen + ndist);
    int index = 0;
    while (index < total) {
        const int sym = dgrp_huff_decode(s, &t->lencode);
        if (sym < 0) return -sym;
        if (sym < 16) { t->lengths[index++] = (int16_t)sym; continue; }
        int16_t len = 0;
        uint32_t rep;
        if (sym == 16) {
            if (index == 0) return DGRP_INFLATE_ECODES;        // repeat with no previous length
            len = t->lengths[index - 1];
            if (!dgrp_bits_get(s, 2, rep)) return DGRP_INFLATE_EINPUT;
            rep += 3;
        } else if (sym == 17) {
            if (!dgrp_bits_get(s, 3, rep)) return DGRP_INFLATE_EINPUT;
            rep += 3;
        } else {
            if (!dgrp_bits_get(s, 7, rep)) return DGRP_INFLATE_EINPUT;
            rep += 11;
        }
        if (index + (int)rep > total) return DGRP_INFLATE_ECODES;
        while (rep--) t->lengths[index++] = len;
    }
    if (t->lengths[256] == 0) return DGRP_INFLATE_ECODES;          // no end-of-block code
    int err = dgrp_huff_build(&t->lencode, t->offs, t->lengths, (int)nlen);
    if (!dgrp_code_ok(err, &t->lencode, (int)nlen)) return DGRP_INFLATE_ECODES;
    err = dgrp_huff_build(&t->distcode, t->offs, t->lengths + nlen, (int)ndist);
    if (!dgrp_code_ok(err, &t->distcode, (int)ndist)) return DGRP_INFLATE_ECODES;
    t->fixed = 0;
    return DGRP_INFLATE_OK;
}

DGRP_HD static void dgrp_build_fixed(dgrp_inflate_tables *t)
{
    for (int i = 0; i < 288; ++i) t->lengths[i] = (int16_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    dgrp_huff_build(&t->lencode, t->offs, t->lengths, 288);
    for (int i = 0; i < 30; ++i) t->lengths[i] = 5;
    dgrp_huff_build(&t->distcode, t->offs, t->lengths, 30);
    t->fixed = 1;
}

// ---- the one block decoder.  Output goes through `sink`, positions relative to the first byte the decoder produces:
//   sink.literal(pos, byte)           out[pos] = byte
//   sink.match(pos, dist, len)        out[pos + j] = out[pos - dist + j] for j = 0 .. len-1 in order (dist <= pos + window checked)
//   sink.stored(pos, src, len)        out[pos + j] = src[j]            (src inside the input slice, checked)
// the counting sink stores nothing
struct dgrp_count_sink {
    DGRP_HD void literal(uint64_t, uint32_t) {}
    DGRP_HD void match(uint64_t, uint32_t, uint32_t) {}
    DGRP_HD void stored(uint64_t, const uint8_t *, uint32_t) {}
};

// The body of a Huffman block, with the codes of t, up to its end-of-block symbol.  `pos` may go up to `cap`; a match may reach
// `window` bytes in front of position 0.  Pos is 32 bits wide where bytes are written (the position sits in the per-symbol loop of
// a latency-bound wave) and 64 bits in the candidate filter, which counts one block without a cap.
template <class Pos, class Sink>
DGRP_HD static inline int dgrp_huff_block(dgrp_bits &s, const dgrp_inflate_tables *t, Sink &sink, Pos &pos, Pos cap, uint32_t window)
{
    uint32_t v;
    for (;;) {
        int sym = dgrp_huff_decode(s, &t->lencode);
        if (sym < 0) return -sym;
        if (sym < 256) {
            if (pos >= cap) return DGRP_INFLATE_EOUTPUT;
            sink.literal(pos, (uint32_t)sym);
            ++pos;
            continue;
        }
        if (sym == 256) return DGRP_INFLATE_OK;
        sym -= 257;
        if (sym >= 29) return DGRP_INFLATE_ESYMBOL;
        int base, extra;
        dgrp_len_code(sym, base, extra);
        if (!dgrp_bits_get(s, extra, v)) return DGRP_INFLATE_EINPUT;
        const uint32_t len = (uint32_t)base + v;
        const int dsym = dgrp_huff_decode(s, &t->distcode);
        if (dsym < 0) return -dsym;
        if (dsym >= 30) return DGRP_INFLATE_ESYMBOL;
        dgrp_dist_code(dsym, base, extra);
        if (!dgrp_bits_get(s, extra, v)) return DGRP_INFLATE_EINPUT;
        const uint32_t dist = (uint32_t)base + v;
        if ((uint64_t)dist > (uint64_t)pos + window) return DGRP_INFLATE_EDIST;
        if (len > cap - pos) return DGRP_INFLATE_EOUTPUT;
        sink.match(pos, dist, len);
        pos += len;
    }
}

// A stored block behind its three header bits: on to a byte boundary, LEN and NLEN, LEN bytes as they are.  An error leaves s.pos
// at the byte dgrp_inflate_core reports as *in_used.
template <class Sink>
DGRP_HD static inline int dgrp_stored_block(dgrp_bits &s, Sink &sink, uint32_t &pos, uint32_t cap)
{
    const uint32_t at = s.pos - (uint32_t)(s.cnt >> 3);          // first byte not consumed
    s.buf = 0;
    s.cnt = 0;
    s.pos = s.len;
    if (at + 4 > s.len || at + 4 < at) return DGRP_INFLATE_EINPUT;
    const uint32_t len = (uint32_t)s.in[at] | ((uint32_t)s.in[at + 1] << 8);
    const uint32_t nlen = (uint32_t)s.in[at + 2] | ((uint32_t)s.in[at + 3] << 8);
    if (len != (~nlen & 0xffffu)) {
        s.pos = at + 4;
        return DGRP_INFLATE_ESTORED;
    }
    if (len > s.len - (at + 4)) return DGRP_INFLATE_EINPUT;
    s.pos = at + 4;
    if (len > cap - pos) return DGRP_INFLATE_EOUTPUT;
    sink.stored(pos, s.in + at + 4, len);
    pos += len;
    s.pos += len;
    return DGRP_INFLATE_OK;
}

// Whole blocks from the reader's position (dgrp_bits_open: any bit of a byte) through `sink`, up to `out_cap` bytes.  Stops in
// front of the first block that starts at or after slice bit `stop`, and behind the final block (*fin = 1).  *land = slice bit of
// the last block boundary reached, *out_len = bytes produced up to there or to the error.  Every decoder is this loop: a member
// is start bit 0, no stop and window 0 (dgrp_inflate_core); a span of a stream has all three (inflate_stream.h).
template <class Sink>
DGRP_HD static int dgrp_inflate_blocks(dgrp_bits &s, int64_t stop, uint32_t window, uint32_t out_cap, dgrp_inflate_tables *t, Sink &sink,
                                       int64_t *land, uint32_t *out_len, int *fin)
{
    t->fixed = 0;
    uint32_t pos = 0, last = 0, type;
    int rc = DGRP_INFLATE_OK;
    for (;;) {
        *land = dgrp_bits_tell(s);
        if (last || *land >= stop) break;
        if (!dgrp_bits_get(s, 1, last) || !dgrp_bits_get(s, 2, type)) rc = DGRP_INFLATE_EINPUT;
        else if (type == 0) rc = dgrp_stored_block(s, sink, pos, out_cap);
        else if (type == 3) rc = DGRP_INFLATE_EBLOCK;
        else {
            if (type == 2) rc = dgrp_read_dynamic(s, t);
            else if (!t->fixed) dgrp_build_fixed(t);
            if (rc == DGRP_INFLATE_OK) rc = dgrp_huff_block(s, t, sink, pos, out_cap, window);
        }
        if (rc != DGRP_INFLATE_OK) break;
    }
    *out_len = pos;
    *fin = (rc == DGRP_INFLATE_OK && last) ? 1 : 0;
    return rc;
}

// One raw DEFLATE stream in[0, in_len) -> output [0, out_cap).  On return *out_len = bytes produced, *in_used = whole input
// bytes consumed up to the end of the last block, or up to the error.
template <class Sink>
DGRP_HD static int dgrp_inflate_core(const uint8_t *in, uint32_t in_len, uint32_t out_cap, dgrp_inflate_tables *t, Sink &sink,
                                     uint32_t *out_len, uint32_t *in_used)
{
    dgrp_bits s;
    dgrp_bits_open(s, in, in_len, 0);
    int64_t land;
    int fin;
    const int rc = dgrp_inflate_blocks(s, INT64_MAX, 0, out_cap, t, sink, &land, out_len, &fin);
    *in_used = s.pos - (uint32_t)(s.cnt >> 3);
    return rc;
}

// the byte sink of the host
struct dgrp_host_sink {
    uint8_t *out;
    void literal(uint32_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
    void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        for (uint32_t j = 0; j < len; ++j) out[pos + j] = out[pos - dist + j];
    }
    void stored(uint32_t pos, const uint8_t *src, uint32_t len)
    {
        for (uint32_t j = 0; j < len; ++j) out[pos + j] = src[j];
    }
};

// what dgrp_last_error() says of a DGRP_INFLATE_E* reason; code 9 reads differently for a span of a stream than for a member
static inline const char *dgrp_inflate_reason_text(int r, bool span)
{
    switch (r) {
    case DGRP_INFLATE_EINPUT: return "input ends inside the stream";
    case DGRP_INFLATE_EBLOCK: return "invalid block type";
    case DGRP_INFLATE_ESTORED: return "stored block LEN/NLEN mismatch";
    case DGRP_INFLATE_ECODES: return "invalid code lengths";
    case DGRP_INFLATE_ESYMBOL: return "invalid symbol";
    case DGRP_INFLATE_EDIST: return "distance too far back";
    case DGRP_INFLATE_EOUTPUT: return "output beyond its size";
    case DGRP_INFLATE_ECRC: return "CRC-32 mismatch";
    case DGRP_INFLATE_EISIZE: return span ? "a span decoded differently than it was counted" : "output shorter than ISIZE";
    case DGRP_INFLATE_ETRAIL: return "stream ends before the trailer";
    case DGRP_INFLATE_ESPAN: return "a span longer than max_span_bytes";
    case DGRP_INFLATE_EROUNDS: return "the chain is not closed after max_rounds rounds";
    default: return "unknown";
    }
}

