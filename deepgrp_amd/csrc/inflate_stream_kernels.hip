// Plain gzip input: ONE DEFLATE stream inflated on the device as many spans (inflate_stream.h), and the same algorithm on the host.
//
//   scan:  inflate_find_kernel    one wave per chunk of compressed bytes: the first bit offset in the chunk's own range that passes
//                                 the candidate filter (lanes screen 64 offsets at a time in registers; survivors, lowest first, get
//                                 the full test on one table set in LDS, every lane on the same state)
//          inflate_count_kernel   one wave per span start: the span decoded with the counting sink
//          chain (host)           which starts are true (stream_chain_run); wrong and missing starts are replaced by the landing of
//                                 the span in front and counted again, round after round
//   write: inflate_symbols_kernel one wave per confirmed span: 16-bit symbols, markers for bytes of the window in front of the span
//          inflate_window_kernel  one workgroup walks the spans in order and resolves the last 32 KiB of each into bytes
//          inflate_resolve_kernel every other symbol: its markers point into tails the walk has finished
//          inflate_crc_kernel     CRC-32 of 64 KiB pieces of the output, folded on the host
//
// Integers only, no atomics.  Every read is checked against the input slice, every write and marker target against the output.
#include "dgrp_common.h"
#include "inflate_stream.h"
#include <algorithm>
#include <vector>

#define STREAM_MAGIC 0x6470677273747231ll        // the workspace holds a chain scan left there
#define STREAM_CRC_PIECE 65536

// ------------------------------------------------------------------------------------------------------------------ sinks
struct stream_wave_sym_sink {
    uint16_t *sym;
    uint32_t lane;
    __device__ void literal(uint32_t pos, uint32_t b)
    {
        if (lane == 0) sym[pos] = (uint16_t)b;
    }
    // (as inflate_wave_sink: a copy reads only symbols in front of its own start, which the wave stored earlier in program order)
    __device__ void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < len; j += 64) sym[pos + j] = dgrp_stream_match_symbol(sym, pos, dist, j);
    }
    __device__ void stored(uint32_t pos, const uint8_t *src, uint32_t len)
    {
        for (uint32_t j = lane; j < len; j += 64) sym[pos + j] = src[j];
    }
};

// ------------------------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(64) inflate_find_kernel(const uint8_t *__restrict__ in, int64_t n, int64_t chunk, int64_t clip,
                                                          int64_t *__restrict__ cand)
{
    __shared__ dgrp_inflate_tables t;
    const uint32_t lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    if (k == 0) {
        if (lane == 0) cand[0] = 0;
        return;
    }
    const int64_t lo = 8 * k * chunk, hi = min(8 * (k + 1) * chunk, 8 * n);
    int64_t found = -1;
    for (int64_t base = lo; base < hi && found < 0; base += 64) {
        const int64_t b = base + lane;
        unsigned long long mask = __ballot(b < hi && dgrp_stream_screen(in, n, b));
        while (mask) {
            const int l = __ffsll(mask) - 1;
            mask &= mask - 1;
            const dgrp_stream_slice sl = dgrp_stream_slice_at(in, n, base + l, clip);
            if (dgrp_stream_candidate(sl, &t)) {
                found = base + l;
                break;
            }
        }
    }
    if (lane == 0) cand[k] = found;
}

// todo = start, stop of span i
__global__ void __launch_bounds__(64) inflate_count_kernel(const uint8_t *__restrict__ in, int64_t n, int64_t clip,
                                                           const int64_t *__restrict__ todo, dgrp_span_count *__restrict__ res)
{
    __shared__ dgrp_inflate_tables t;
    const int64_t i = blockIdx.x;
    const int64_t start = todo[2 * i], stop = todo[2 * i + 1];
    dgrp_span_count r;
    if (start < 0 || start > 8 * n) {
        r.land = 0;
        r.bytes = 0;
        r.rc_fin = DGRP_INFLATE_EINPUT;
    } else {
        r = dgrp_stream_count(in, n, start, stop, clip, &t);
    }
    if (threadIdx.x == 0) res[i] = r;
}

__global__ void __launch_bounds__(64) inflate_symbols_kernel(const uint8_t *__restrict__ in, int64_t n, int64_t clip,
                                                             const stream_span *__restrict__ tab, uint16_t *__restrict__ sym,
                                                             int64_t total, int32_t *__restrict__ status)
{
    __shared__ dgrp_inflate_tables t;
    const int64_t k = blockIdx.x;
    const stream_span sp = tab[k];
    const int64_t o1 = tab[k + 1].out_off;
    int rc = DGRP_INFLATE_OK;
    if (sp.start < 0 || sp.start > 8 * n || sp.out_off < 0 || o1 < sp.out_off || o1 > total || o1 - sp.out_off > (int64_t)DGRP_SPAN_MAX_OUT) {
        rc = DGRP_INFLATE_EOUTPUT;
    } else {
        stream_wave_sym_sink sink{sym + sp.out_off, threadIdx.x};
        rc = dgrp_stream_span(in, n, clip, sp, (uint32_t)(o1 - sp.out_off), &t, sink);
    }
    if (threadIdx.x == 0) status[k] = rc;
}

// one workgroup: span after span, the last 32 KiB of symbols (all of a shorter span) into bytes.  A marker of span k reads the
// 32 KiB of `out` in front of the span, which earlier iterations finished: they are the tails of the spans before it.
__global__ void __launch_bounds__(1024) inflate_window_kernel(const stream_span *__restrict__ tab, int64_t nspan,
                                                              const uint16_t *__restrict__ sym, uint8_t *out, int64_t total,
                                                              int32_t *__restrict__ status)
{
    int bad = DGRP_INFLATE_OK;
    for (int64_t k = 0; k < nspan; ++k) {
        const int64_t o0 = tab[k].out_off, o1 = tab[k + 1].out_off;
        if (o0 < 0 || o1 < o0 || o1 > total) {
            bad = DGRP_INFLATE_EOUTPUT;
            break;                                                   // (the same for every thread)
        }
        // a tail is at most 32 symbols a thread: all of them are loaded before the first is resolved, so one span costs one
        // round trip for the symbols and one for the window bytes its markers name, not thirty-two of each
        const int64_t t0 = stream_tail_begin(o0, o1) + threadIdx.x;
        uint32_t v[DGRP_STREAM_WINDOW / 1024];
#pragma unroll
        for (int r = 0; r < DGRP_STREAM_WINDOW / 1024; ++r) v[r] = t0 + r * 1024 < o1 ? sym[t0 + r * 1024] : 0;
#pragma unroll
        for (int r = 0; r < DGRP_STREAM_WINDOW / 1024; ++r) {
            uint8_t b = 0;
            const int rc = stream_resolve_symbol(v[r], o0, out, &b);
            if (rc != DGRP_INFLATE_OK) bad = rc;
            v[r] = b;
        }
#pragma unroll
        for (int r = 0; r < DGRP_STREAM_WINDOW / 1024; ++r)
            if (t0 + r * 1024 < o1) out[t0 + r * 1024] = (uint8_t)v[r];
        __threadfence_block();
        __syncthreads();
    }
    if (bad != DGRP_INFLATE_OK) *status = bad;                        // (every writer holds a reason)
}

// grid (span, piece): the symbols in front of the span's tail
__global__ void __launch_bounds__(256) inflate_resolve_kernel(const stream_span *__restrict__ tab, const uint16_t *__restrict__ sym,
                                                              uint8_t *out, int64_t total, int32_t *__restrict__ status)
{
    const int64_t k = blockIdx.x;
    const int64_t o0 = tab[k].out_off, o1 = tab[k + 1].out_off;
    if (o0 < 0 || o1 < o0 || o1 > total) return;                      // (the window kernel reports it)
    const int64_t head = stream_tail_begin(o0, o1);
    int bad = DGRP_INFLATE_OK;
    for (int64_t i = o0 + (int64_t)blockIdx.y * 256 + threadIdx.x; i < head; i += 256 * (int64_t)gridDim.y) {
        uint8_t b = 0;
        const int rc = stream_resolve_symbol(sym[i], o0, out, &b);
        if (rc != DGRP_INFLATE_OK) bad = rc;
        out[i] = b;
    }
    if (bad != DGRP_INFLATE_OK) status[k] = bad;                      // (every writer holds a reason)
}

// one wave per 64 KiB piece, 1 KiB a lane
__global__ void __launch_bounds__(64) inflate_crc_kernel(const uint8_t *__restrict__ out, int64_t total, uint32_t *__restrict__ crcs)
{
    __shared__ uint32_t crctab[256];
    const int64_t p0 = (int64_t)blockIdx.x * STREAM_CRC_PIECE;
    const int64_t p1 = min(p0 + STREAM_CRC_PIECE, total);
    const int64_t a = min(p0 + (int64_t)threadIdx.x * (STREAM_CRC_PIECE / 64), p1), b = min(a + STREAM_CRC_PIECE / 64, p1);
    const uint32_t crc = dgrp_crc_wave(out + a, out + b, crctab);
    if (threadIdx.x == 0) crcs[blockIdx.x] = crc;
}

static bool stream_sizes_ok(int64_t n, int64_t chunk, int64_t max_span, int max_rounds)
{
    return n >= 0 && n < (1ll << 40) && chunk >= 64 && chunk <= (1 << 28) && max_span >= 1 && max_span <= (1ll << 31) - 64 && max_rounds >= 1;
}

// ------------------------------------------------------------------------------------------------------------------ host entry
DGRP_EXPORT int dgrp_inflate_stream_host(const uint8_t *h_in, int64_t in_len, int64_t chunk_bytes, int64_t max_span_bytes, int max_rounds,
                                         uint8_t *h_out, int64_t out_cap, int64_t *h_out_len, int64_t *h_in_used,
                                         dgrp_inflate_stream_stats *h_stats, int *h_reason)
{
    DGRP_REQUIRE(h_out_len && h_in_used && h_stats && h_reason, "dgrp_inflate_stream_host: bad arguments");
    DGRP_REQUIRE(out_cap >= 0 && stream_sizes_ok(in_len, chunk_bytes, max_span_bytes, max_rounds),
                 "dgrp_inflate_stream_host: bad sizes (chunk_bytes 64 .. 2^28, max_span_bytes 1 .. 2^31 - 64, max_rounds >= 1)");
    DGRP_REQUIRE((h_in || in_len == 0) && (h_out || out_cap == 0), "dgrp_inflate_stream_host: NULL pointer");
    *h_out_len = 0;
    *h_in_used = 0;
    *h_reason = 0;
    *h_stats = dgrp_inflate_stream_stats{};
    const int rc = dgrp_stream_inflate_host(h_in, in_len, chunk_bytes, max_span_bytes, max_rounds, h_out, out_cap, h_out_len, h_in_used, h_stats,
                                            h_reason);
    if (rc == DGRP_EDATA)
        dgrp_set_error("dgrp_inflate_stream_host: %s (reason %d)", dgrp_inflate_reason_text(*h_reason, true), *h_reason);
    return rc;
}

// ------------------------------------------------------------------------------------------------------------------ device entries
struct stream_layout {
    int64_t nchunk, head, cand, todo, res, tab, status, crc, crc_cap, bytes;
};
static stream_layout stream_layout_of(int64_t in_bytes, int64_t chunk)
{
    stream_layout l;
    l.nchunk = std::max<int64_t>(1, (in_bytes + chunk - 1) / chunk);
    l.crc_cap = in_bytes / 32 + 16;               // pieces of 64 KiB of at most 1032 bytes of text per byte of the stream
    int64_t o = 0;
    l.head = o;   o += 256;
    l.cand = o;   o += dgrp_align_up(l.nchunk * 8, 256);
    l.todo = o;   o += dgrp_align_up(l.nchunk * 16, 256);
    l.res = o;    o += dgrp_align_up(l.nchunk * (int64_t)sizeof(dgrp_span_count), 256);
    l.tab = o;    o += dgrp_align_up((l.nchunk + 1) * (int64_t)sizeof(stream_span), 256);
    l.status = o; o += dgrp_align_up((l.nchunk + 1) * 4, 256);
    l.crc = o;    o += dgrp_align_up(l.crc_cap * 4, 256);
    l.bytes = o;
    return l;
}

DGRP_EXPORT int64_t dgrp_inflate_stream_workspace_bytes(int64_t in_bytes, int64_t chunk_bytes)
{
    if (!stream_sizes_ok(in_bytes, chunk_bytes, 1, 1)) return 0;
    return stream_layout_of(in_bytes, chunk_bytes).bytes;
}

DGRP_EXPORT int dgrp_inflate_stream_scan(const uint8_t *d_in, int64_t in_bytes, int64_t data_off, int64_t chunk_bytes,
                                         int64_t max_span_bytes, int max_rounds, int64_t *h_total, dgrp_inflate_stream_stats *h_stats,
                                         int *h_reason, void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_total && h_stats && h_reason, "dgrp_inflate_stream_scan: bad arguments");
    DGRP_REQUIRE(stream_sizes_ok(in_bytes, chunk_bytes, max_span_bytes, max_rounds) && data_off >= 0 && data_off <= in_bytes,
                 "dgrp_inflate_stream_scan: bad sizes (chunk_bytes 64 .. 2^28, max_span_bytes 1 .. 2^31 - 64, max_rounds >= 1, "
                 "0 <= data_off <= in_bytes)");
    DGRP_REQUIRE(d_in && d_work, "dgrp_inflate_stream_scan: NULL pointer");
    const stream_layout l = stream_layout_of(in_bytes, chunk_bytes);
    if (work_bytes < l.bytes) {
        dgrp_set_error("dgrp_inflate_stream_scan: workspace too small");
        return DGRP_ENOMEM;
    }
    *h_total = 0;
    *h_reason = 0;
    *h_stats = dgrp_inflate_stream_stats{};
    char *w = (char *)d_work;
    const uint8_t *in = d_in + data_off;
    stream_chain c;
    c.init(in_bytes - data_off, chunk_bytes, max_span_bytes);
    int64_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};                     // no chain until this call has closed one
    DGRP_HIP(hipMemcpyAsync(w + l.head, head, sizeof head, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(inflate_find_kernel, dim3((unsigned)c.nchunk), dim3(64), 0, stream, in, c.n, c.chunk, c.clip, (int64_t *)(w + l.cand));
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipMemcpyAsync(c.start.data(), w + l.cand, (size_t)c.nchunk * 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int64_t k = 0; k < c.nchunk; ++k) {                        // (what the kernel may give)
        const int64_t b = c.start[(size_t)k];
        if (b != -1 && (b < 8 * k * c.chunk || b >= 8 * (k + 1) * c.chunk || b >= 8 * std::max<int64_t>(c.n, 1))) c.start[(size_t)k] = -1;
    }
    std::vector<int64_t> pairs;
    std::vector<dgrp_span_count> res;
    auto count = [&](const std::vector<int64_t> &todo) -> int {
        pairs.clear();
        for (int64_t k : todo) {
            pairs.push_back(c.start[(size_t)k]);
            pairs.push_back(c.stop_of(k));
        }
        res.resize(todo.size());
        DGRP_HIP(hipMemcpyAsync(w + l.todo, pairs.data(), pairs.size() * 8, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(inflate_count_kernel, dim3((unsigned)todo.size()), dim3(64), 0, stream, in, c.n, c.clip,
                           (const int64_t *)(w + l.todo), (dgrp_span_count *)(w + l.res));
        DGRP_LAUNCH_CHECK();
        DGRP_HIP(hipMemcpyAsync(res.data(), w + l.res, res.size() * sizeof(dgrp_span_count), hipMemcpyDeviceToHost, stream));
        DGRP_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < todo.size(); ++i) {
            const size_t k = (size_t)todo[i];
            c.land[k] = res[i].land;
            c.bytes[k] = res[i].bytes;
            c.rc_fin[k] = res[i].rc_fin;
        }
        return DGRP_OK;
    };
    const int rc = stream_chain_run(c, max_span_bytes, max_rounds, count, h_stats, h_reason);
    if (rc == DGRP_EDATA)
        dgrp_set_error("dgrp_inflate_stream_scan: %s (reason %d)", dgrp_inflate_reason_text(*h_reason, true), *h_reason);
    if (rc != DGRP_OK) return rc;
    std::vector<stream_span> tab;
    const int64_t total = stream_span_table(c, tab);
    DGRP_HIP(hipMemcpyAsync(w + l.tab, tab.data(), tab.size() * sizeof(stream_span), hipMemcpyHostToDevice, stream));
    head[0] = STREAM_MAGIC;
    head[1] = in_bytes;
    head[2] = data_off;
    head[3] = chunk_bytes;
    head[4] = (int64_t)tab.size() - 1;
    head[5] = total;
    head[6] = tab[tab.size() - 2].land;
    head[7] = c.clip;
    DGRP_HIP(hipMemcpyAsync(w + l.head, head, sizeof head, hipMemcpyHostToDevice, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    *h_total = total;
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_inflate_stream_write(const uint8_t *d_in, int64_t in_bytes, int64_t data_off, int64_t chunk_bytes, uint16_t *d_sym,
                                          uint8_t *d_out, int64_t out_bytes, uint32_t *h_crc, int64_t *h_in_used, int *h_reason,
                                          void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_crc && h_in_used && h_reason, "dgrp_inflate_stream_write: bad arguments");
    DGRP_REQUIRE(stream_sizes_ok(in_bytes, chunk_bytes, 1, 1) && data_off >= 0 && data_off <= in_bytes && out_bytes >= 0,
                 "dgrp_inflate_stream_write: bad sizes");
    DGRP_REQUIRE(d_in && d_work && ((d_sym && d_out) || out_bytes == 0), "dgrp_inflate_stream_write: NULL pointer");
    const stream_layout l = stream_layout_of(in_bytes, chunk_bytes);
    if (work_bytes < l.bytes) {
        dgrp_set_error("dgrp_inflate_stream_write: workspace too small");
        return DGRP_ENOMEM;
    }
    *h_crc = 0;
    *h_in_used = 0;
    *h_reason = 0;
    char *w = (char *)d_work;
    int64_t head[8];
    DGRP_HIP(hipMemcpyAsync(head, w + l.head, sizeof head, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    const int64_t nspan = head[4], total = head[5], clip = head[7];
    DGRP_REQUIRE(head[0] == STREAM_MAGIC && head[1] == in_bytes && head[2] == data_off && head[3] == chunk_bytes && nspan >= 1 &&
                     nspan <= l.nchunk && clip >= 17 && clip <= (1ll << 31),
                 "dgrp_inflate_stream_write: the workspace holds no chain of dgrp_inflate_stream_scan for this input");
    DGRP_REQUIRE(total == out_bytes, "dgrp_inflate_stream_write: out_bytes %lld is not the total %lld that scan reported",
                 (long long)out_bytes, (long long)total);
    const int64_t npiece = (total + STREAM_CRC_PIECE - 1) / STREAM_CRC_PIECE;
    if (npiece > l.crc_cap) {
        dgrp_set_error("dgrp_inflate_stream_write: workspace too small for the CRC pieces");
        return DGRP_ENOMEM;
    }
    const uint8_t *in = d_in + data_off;
    const int64_t n = in_bytes - data_off;
    const stream_span *tab = (const stream_span *)(w + l.tab);
    int32_t *status = (int32_t *)(w + l.status);
    uint32_t *crcs = (uint32_t *)(w + l.crc);
    DGRP_HIP(hipMemsetAsync(status, 0, (size_t)(nspan + 1) * 4, stream));
    hipLaunchKernelGGL(inflate_symbols_kernel, dim3((unsigned)nspan), dim3(64), 0, stream, in, n, clip, tab, d_sym, total, status);
    DGRP_LAUNCH_CHECK();
    std::vector<int32_t> st((size_t)nspan + 1);
    std::vector<uint32_t> pc((size_t)npiece);
    if (total > 0) {
        hipLaunchKernelGGL(inflate_window_kernel, dim3(1), dim3(1024), 0, stream, tab, nspan, d_sym, d_out, total, status + nspan);
        DGRP_LAUNCH_CHECK();
        hipLaunchKernelGGL(inflate_resolve_kernel, dim3((unsigned)nspan, 4), dim3(256), 0, stream, tab, d_sym, d_out, total, status);
        DGRP_LAUNCH_CHECK();
        hipLaunchKernelGGL(inflate_crc_kernel, dim3((unsigned)npiece), dim3(64), 0, stream, d_out, total, crcs);
        DGRP_LAUNCH_CHECK();
        DGRP_HIP(hipMemcpyAsync(pc.data(), crcs, (size_t)npiece * 4, hipMemcpyDeviceToHost, stream));
    }
    DGRP_HIP(hipMemcpyAsync(st.data(), status, st.size() * 4, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (size_t k = 0; k < st.size(); ++k)
        if (st[k] != DGRP_INFLATE_OK) {
            *h_reason = st[k];
            dgrp_set_error("dgrp_inflate_stream_write: span %lld: %s (reason %d)", (long long)k, dgrp_inflate_reason_text(st[k], true), st[k]);
            return DGRP_EDATA;
        }
    uint32_t crc = 0;
    for (int64_t p = 0; p < npiece; ++p)
        crc = dgrp_crc_combine(crc, pc[(size_t)p], (uint64_t)std::min<int64_t>(STREAM_CRC_PIECE, total - p * STREAM_CRC_PIECE));
    *h_crc = crc;
    *h_in_used = data_off + (head[6] + 7) / 8;
    return DGRP_OK;
}
