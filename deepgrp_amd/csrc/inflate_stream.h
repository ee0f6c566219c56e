// One DEFLATE stream decoded as many spans, written once for the host and the device on the decode core of inflate.h.
//
// A plain gzip file is one DEFLATE stream; its blocks start at arbitrary bit offsets and every match may reach 32 KiB back.  The
// stream is cut into chunks of compressed bytes.  For every chunk the finder looks for the first bit offset at which a non-final
// dynamic block starts (dgrp_stream_screen, then dgrp_stream_candidate); a span is decoded from such a start, block after block,
// up to the first block boundary at or after the next chunk's range (dgrp_span_decode), without the 32 KiB of text in front of it:
// first only counted, then into 16-bit symbols where a value of 256 + w stands for "byte w of the 32 KiB window in front of this
// span".  Which starts are true is decided by the chain (stream_chain_run): span 0 starts at bit 0, and a start is confirmed when
// the span before it lands on it.
//
// A span addresses its input through a slice of its own (dgrp_stream_slice): the 32-bit pos and len of dgrp_bits bound a span,
// bit positions in the stream are int64_t.  Every read is checked against the slice and every write against out_cap.
#pragma once
#include "inflate.h"

#define DGRP_STREAM_WINDOW 32768
#define DGRP_STREAM_MARK 256                     // symbol of window byte 0

// The slice of the stream in[0, n) a span from bit `bit` (0 <= bit < 8 n) reads: at most `clip` bytes from the byte of its start.
struct dgrp_stream_slice {
    const uint8_t *in;
    uint32_t len, skip;
    int64_t bit0;                                // stream bit of the slice's bit 0
    int clipped;                                 // the slice ends before the stream does
};
DGRP_HD static inline dgrp_stream_slice dgrp_stream_slice_at(const uint8_t *in, int64_t n, int64_t bit, int64_t clip)
{
    dgrp_stream_slice sl;
    const int64_t byte0 = bit >> 3, rem = n - byte0;
    sl.in = in + byte0;
    sl.len = (uint32_t)(rem < clip ? rem : clip);
    sl.skip = (uint32_t)(bit & 7);
    sl.bit0 = byte0 * 8;
    sl.clipped = rem > clip;
    return sl;
}

// ---- the register-only part of the candidate filter: BFINAL = 0, BTYPE = 2, HLIT and HDIST in range, the header inside the
// input, and a complete code length code (an over-subscribed or incomplete one is what dgrp_read_dynamic refuses first)
DGRP_HD static inline bool dgrp_stream_screen(const uint8_t *in, int64_t n, int64_t bit)
{
    const int64_t byte0 = bit >> 3;
    const int sh = (int)(bit & 7);
    uint64_t lo = 0;
    uint32_t hi = 0;
    for (int i = 0; i < 8; ++i)
        if (byte0 + i < n) lo |= (uint64_t)in[byte0 + i] << (8 * i);
    if ((((uint32_t)lo >> sh) & 7u) != 4u) return false;
    for (int i = 0; i < 3; ++i)
        if (byte0 + 8 + i < n) hi |= (uint32_t)in[byte0 + 8 + i] << (8 * i);
    const uint64_t w = sh ? (lo >> sh) | ((uint64_t)hi << (64 - sh)) : lo;          // stream bits bit .. bit + 63
    const uint32_t w2 = hi >> sh;                                                  // bit + 64 ..
    const uint32_t hlit = (uint32_t)(w >> 3) & 31u, hdist = (uint32_t)(w >> 8) & 31u, ncode = ((uint32_t)(w >> 13) & 15u) + 4;
    if (hlit > 29 || hdist > 29) return false;
    if ((n - byte0) * 8 - sh < 17 + 3 * (int64_t)ncode) return false;
    const uint64_t cl = (w >> 17) | ((uint64_t)w2 << 47);
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        const uint32_t l = (uint32_t)(cl >> (3 * i)) & 7u;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// ---- the full filter: a non-final dynamic block whose header dgrp_read_dynamic accepts, whose body decodes to its end-of-block
// symbol with no distance above what a 32 KiB window in front could serve, and behind which the next block's type is not 3
DGRP_HD static bool dgrp_stream_candidate(const dgrp_stream_slice &sl, dgrp_inflate_tables *t)
{
    dgrp_bits s;
    dgrp_bits_open(s, sl.in, sl.len, sl.skip);
    dgrp_count_sink sink;
    uint64_t pos = 0;                            // one block of a span of up to 2^31 bytes may hold more than 2^32 bytes of text
    uint32_t v;
    return dgrp_bits_get(s, 3, v) && v == 4u && dgrp_read_dynamic(s, t) == DGRP_INFLATE_OK &&
           dgrp_huff_block(s, t, sink, pos, UINT64_MAX, DGRP_STREAM_WINDOW) == DGRP_INFLATE_OK && dgrp_bits_get(s, 3, v) && (v >> 1) != 3u;
}

// ---- the span decoder: the block loop of inflate.h (dgrp_inflate_blocks) over a slice, with a match reaching up to
// DGRP_STREAM_WINDOW bytes in front of the span's first byte.  `stop` and *land are stream bits.
template <class Sink>
DGRP_HD static int dgrp_span_decode(const dgrp_stream_slice &sl, int64_t stop, uint32_t out_cap, dgrp_inflate_tables *t, Sink &sink,
                                    int64_t *land, uint32_t *out_len, int *fin)
{
    dgrp_bits s;
    dgrp_bits_open(s, sl.in, sl.len, sl.skip);
    const int rc = dgrp_inflate_blocks(s, stop - sl.bit0, DGRP_STREAM_WINDOW, out_cap, t, sink, land, out_len, fin);
    *land += sl.bit0;
    return rc;
}

// the symbol a match copies from j bytes into its source, which starts `dist` bytes in front of span position `pos`
DGRP_HD static inline uint16_t dgrp_stream_match_symbol(const uint16_t *sym, uint32_t pos, uint32_t dist, uint32_t j)
{
    const int64_t src = (int64_t)pos - (int64_t)dist + (int64_t)(j < dist ? j : j % dist);
    return src >= 0 ? sym[src] : (uint16_t)(DGRP_STREAM_MARK + DGRP_STREAM_WINDOW + src);
}

// what the counting pass knows of a span
struct dgrp_span_count {
    int64_t land;                                // stream bit of the boundary it stopped at (or the last one before its error)
    uint32_t bytes;
    int32_t rc_fin;                              // DGRP_INFLATE_* reason | final block seen << 8
};

// most bytes a span may produce (a match of 258 bytes must still fit into the 32-bit position)
#define DGRP_SPAN_MAX_OUT 0xfffffe00u

// The span from stream bit `start` of in[0, n) to the first boundary at or after stream bit `stop`, counted.  A span that would
// read more than `clip` bytes is DGRP_INFLATE_ESPAN.
DGRP_HD static dgrp_span_count dgrp_stream_count(const uint8_t *in, int64_t n, int64_t start, int64_t stop, int64_t clip,
                                                 dgrp_inflate_tables *t)
{
    dgrp_span_count r;
    const dgrp_stream_slice sl = dgrp_stream_slice_at(in, n, start, clip);
    dgrp_count_sink sink;
    int fin = 0;
    int rc = dgrp_span_decode(sl, stop, DGRP_SPAN_MAX_OUT, t, sink, &r.land, &r.bytes, &fin);
    if (rc == DGRP_INFLATE_EINPUT && sl.clipped) rc = DGRP_INFLATE_ESPAN;
    r.rc_fin = rc | (fin << 8);
    return r;
}

struct stream_span {                             // one confirmed span (the table has one more entry: out_off = total)
    int64_t start, stop, out_off, land;
};

// The confirmed span `sp` of in[0, n) once more, through `sink` into exactly `cap` positions: DGRP_INFLATE_EISIZE when it gives
// other bytes or another landing than the counting pass saw.
template <class Sink>
DGRP_HD static int dgrp_stream_span(const uint8_t *in, int64_t n, int64_t clip, const stream_span &sp, uint32_t cap,
                                    dgrp_inflate_tables *t, Sink &sink)
{
    int64_t land = 0;
    uint32_t bytes = 0;
    int fin = 0;
    const int rc = dgrp_span_decode(dgrp_stream_slice_at(in, n, sp.start, clip), sp.stop, cap, t, sink, &land, &bytes, &fin);
    return rc == DGRP_INFLATE_OK && (bytes != cap || land != sp.land) ? DGRP_INFLATE_EISIZE : rc;
}

// ================================================================================================ the host side (plain C++)
#include <algorithm>
#include <vector>

struct stream_host_sym_sink {
    uint16_t *sym;
    void literal(uint32_t pos, uint32_t b) { sym[pos] = (uint16_t)b; }
    void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        for (uint32_t j = 0; j < len; ++j) sym[pos + j] = dgrp_stream_match_symbol(sym, pos, dist, j);
    }
    void stored(uint32_t pos, const uint8_t *src, uint32_t len)
    {
        for (uint32_t j = 0; j < len; ++j) sym[pos + j] = src[j];
    }
};

// symbol v of a span whose first byte is out[span_off] -> its byte; a marker reads the 32 KiB in front of the span
DGRP_HD static inline int stream_resolve_symbol(uint32_t v, int64_t span_off, const uint8_t *out, uint8_t *b)
{
    if (v < DGRP_STREAM_MARK) {
        *b = (uint8_t)v;
        return DGRP_INFLATE_OK;
    }
    const int64_t tgt = span_off - DGRP_STREAM_WINDOW + ((int64_t)v - DGRP_STREAM_MARK);
    if (v >= DGRP_STREAM_MARK + DGRP_STREAM_WINDOW || tgt < 0) return DGRP_INFLATE_EDIST;
    *b = out[tgt];
    return DGRP_INFLATE_OK;
}
// first symbol of span [o0, o1) that the window walk resolves
DGRP_HD static inline int64_t stream_tail_begin(int64_t o0, int64_t o1)
{
    return o1 - o0 > DGRP_STREAM_WINDOW ? o1 - DGRP_STREAM_WINDOW : o0;
}

struct stream_chain {
    int64_t n = 0, chunk = 0, nchunk = 0, clip = 0;
    bool single = false;                          // no candidate anywhere: one span from bit 0 to the end of the stream
    std::vector<int64_t> start, land;
    std::vector<uint32_t> bytes;
    std::vector<int32_t> rc_fin;
    std::vector<int64_t> spans;                   // the chunks of the confirmed spans, in order
    int64_t stop_of(int64_t k) const { return single ? INT64_MAX / 2 : 8 * (k + 1) * chunk; }
    void init(int64_t n_, int64_t chunk_, int64_t max_span)
    {
        n = n_;
        chunk = chunk_;
        nchunk = std::max<int64_t>(1, (n + chunk - 1) / chunk);
        clip = max_span + 16;
        start.assign((size_t)nchunk, -1);
        land.assign((size_t)nchunk, 0);
        bytes.assign((size_t)nchunk, 0);
        rc_fin.assign((size_t)nchunk, 0);
    }
};

// Span 0 starts at bit 0.  The landing of a confirmed span k lies in the range of a chunk j > k; when chunk j's start is that
// landing it is confirmed, otherwise it becomes the landing and is counted again in the next round.  Behind such a stall the walk
// goes on from the next start it has, unconfirmed, only to collect more starts to count in the same round; every round walks
// again from span 0, so nothing unconfirmed reaches the result.  An error of an unconfirmed span is no stream error.
// count(todo) fills land, bytes, rc_fin of the chunks in todo.  -> DGRP_OK, DGRP_EDATA with *reason, or count's error.
template <class Count>
static int stream_chain_run(stream_chain &c, int64_t max_span, int max_rounds, Count &&count, dgrp_inflate_stream_stats *st, int *reason)
{
    std::vector<int64_t> todo;
    st->chunks = c.nchunk;
    st->candidates = 0;
    c.start[0] = 0;
    for (int64_t k = 1; k < c.nchunk; ++k) st->candidates += c.start[(size_t)k] >= 0;
    c.single = st->candidates == 0;
    for (int64_t k = 0; k < c.nchunk; ++k)
        if (c.start[(size_t)k] >= 0) todo.push_back(k);
    for (int round = 1;; ++round) {
        if (round > max_rounds) {
            *reason = DGRP_INFLATE_EROUNDS;
            return DGRP_EDATA;
        }
        st->rounds = round;
        const int rc = count(todo);
        if (rc != DGRP_OK) return rc;
        todo.clear();
        c.spans.clear();
        bool confirmed = true, done = false;
        int64_t k = 0;
        for (;;) {
            const int r = c.rc_fin[(size_t)k] & 0xff, fin = c.rc_fin[(size_t)k] >> 8;
            if (confirmed) {
                c.spans.push_back(k);
                if (r != DGRP_INFLATE_OK) {
                    *reason = r;
                    return DGRP_EDATA;
                }
                if ((c.land[(size_t)k] - c.start[(size_t)k] + 7) / 8 > max_span) {
                    *reason = DGRP_INFLATE_ESPAN;
                    return DGRP_EDATA;
                }
            }
            if (r != DGRP_INFLATE_OK) break;
            if (fin) {
                done = confirmed;
                break;
            }
            const int64_t L = c.land[(size_t)k], j = L / (8 * c.chunk);
            if (j <= k || j >= c.nchunk) {                           // the stream ends without a final block
                if (confirmed) {
                    *reason = DGRP_INFLATE_EINPUT;
                    return DGRP_EDATA;
                }
                break;
            }
            if (c.start[(size_t)j] == L) {
                k = j;
                continue;
            }
            st->repaired += 1;
            st->false_starts += c.start[(size_t)j] >= 0 && c.start[(size_t)j] < L;
            c.start[(size_t)j] = L;
            todo.push_back(j);
            confirmed = false;
            int64_t m = j + 1;
            while (m < c.nchunk && c.start[(size_t)m] < 0) ++m;
            if (m >= c.nchunk) break;
            k = m;
        }
        if (done) break;
        if (todo.empty()) {                                          // an unconfirmed final block with nothing left to count
            *reason = DGRP_INFLATE_EINPUT;
            return DGRP_EDATA;
        }
    }
    st->spans = (int64_t)c.spans.size();
    st->longest_span = 0;
    for (int64_t k : c.spans) st->longest_span = std::max(st->longest_span, (c.land[(size_t)k] - c.start[(size_t)k] + 7) / 8);
    return DGRP_OK;
}

// the span table of a closed chain -> total
static int64_t stream_span_table(const stream_chain &c, std::vector<stream_span> &tab)
{
    int64_t off = 0;
    tab.clear();
    for (int64_t k : c.spans) {
        tab.push_back(stream_span{c.start[(size_t)k], c.stop_of(k), off, c.land[(size_t)k]});
        off += c.bytes[(size_t)k];
    }
    tab.push_back(stream_span{0, 0, off, 0});
    return off;
}

// The whole algorithm on the host: finder, counting rounds and chain, symbols, window walk, resolve (the order of the device).
// The outputs are preset by the caller; -> DGRP_OK or DGRP_EDATA with *h_reason.
static int dgrp_stream_inflate_host(const uint8_t *h_in, int64_t in_len, int64_t chunk_bytes, int64_t max_span_bytes, int max_rounds,
                                   uint8_t *h_out, int64_t out_cap, int64_t *h_out_len, int64_t *h_in_used,
                                   dgrp_inflate_stream_stats *h_stats, int *h_reason)
{
    dgrp_inflate_tables t;
    stream_chain c;
    c.init(in_len, chunk_bytes, max_span_bytes);
    for (int64_t k = 1; k < c.nchunk; ++k) {
        const int64_t hi = std::min(8 * (k + 1) * c.chunk, 8 * c.n);
        for (int64_t b = 8 * k * c.chunk; b < hi; ++b)
            if (dgrp_stream_screen(h_in, c.n, b) && dgrp_stream_candidate(dgrp_stream_slice_at(h_in, c.n, b, c.clip), &t)) {
                c.start[(size_t)k] = b;
                break;
            }
    }
    auto count = [&](const std::vector<int64_t> &todo) {
        for (int64_t k : todo) {
            const dgrp_span_count r = dgrp_stream_count(h_in, c.n, c.start[(size_t)k], c.stop_of(k), c.clip, &t);
            c.land[(size_t)k] = r.land;
            c.bytes[(size_t)k] = r.bytes;
            c.rc_fin[(size_t)k] = r.rc_fin;
        }
        return DGRP_OK;
    };
    int rc = stream_chain_run(c, max_span_bytes, max_rounds, count, h_stats, h_reason);
    std::vector<stream_span> tab;
    int64_t total = 0;
    if (rc == DGRP_OK) {
        total = stream_span_table(c, tab);
        if (total > out_cap) {
            *h_reason = DGRP_INFLATE_EOUTPUT;
            rc = DGRP_EDATA;
        }
    }
    if (rc == DGRP_OK) {
        std::vector<uint16_t> sym((size_t)total + 1);
        const size_t nspan = tab.size() - 1;
        for (size_t k = 0; k < nspan && rc == DGRP_OK; ++k) {
            stream_host_sym_sink sink{sym.data() + tab[k].out_off};
            const int r = dgrp_stream_span(h_in, c.n, c.clip, tab[k], (uint32_t)(tab[k + 1].out_off - tab[k].out_off), &t, sink);
            if (r != DGRP_INFLATE_OK) {
                *h_reason = r;
                rc = DGRP_EDATA;
            }
        }
        // the window walk, then everything in front of the tails: the order of the device
        for (int pass = 0; pass < 2 && rc == DGRP_OK; ++pass)
            for (size_t k = 0; k < nspan && rc == DGRP_OK; ++k) {
                const int64_t o0 = tab[k].out_off, o1 = tab[k + 1].out_off, head = stream_tail_begin(o0, o1);
                for (int64_t i = pass ? o0 : head; i < (pass ? head : o1); ++i) {
                    const int r = stream_resolve_symbol(sym[(size_t)i], o0, h_out, h_out + i);
                    if (r != DGRP_INFLATE_OK) {
                        *h_reason = r;
                        rc = DGRP_EDATA;
                        break;
                    }
                }
            }
        if (rc == DGRP_OK) {
            *h_out_len = total;
            *h_in_used = (tab[nspan - 1].land + 7) / 8;
        }
    }
    return rc;
}
