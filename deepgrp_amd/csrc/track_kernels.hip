// Probability tracks (predict --track_dir): one class column of a record's merged probabilities [n, C] as 4-column bedGraph text,
// built in HBM.  Three passes: bin max + quantisation (reads the strided column), bytes of text per tile of bins, and the text itself;
// between them one scan of the tile sums.  Every index and byte offset is 64-bit.
// See include/deepgrp_hip.h.
#include "dgrp_common.h"
#include "scan.h"

namespace {

#define TRACK_WAVE_BIN 64         // bins wider than this are reduced by a whole wave, narrower ones by one lane

struct track_geom {
    int64_t offset, n, bin;       // span [offset, offset + n) in record coordinates, bin width
    int64_t kb0, nb;              // first bin (offset / bin), bins touching the span
};

// the coordinates [lo, hi) of bin j, clipped to the span
__device__ __forceinline__ void track_bin_span(const track_geom &g, int64_t j, int64_t &lo, int64_t &hi)
{
    const int64_t a = (g.kb0 + j) * g.bin, b = a + g.bin;
    lo = a > g.offset ? a : g.offset;
    hi = b < g.offset + g.n ? b : g.offset + g.n;
}

// floor(v * 10^D + 0.5) as two float32 roundings (this file is compiled with -ffp-contract=off), clamped to [0, 10^D]
__device__ __forceinline__ uint32_t track_quantise(float v, float scale, uint32_t qmax)
{
    const float t = v * scale;
    const float q = floorf(t + 0.5f);
    return q <= 0.0f ? 0u : q >= (float)qmax ? qmax : (uint32_t)q;
}

// one lane per bin (bins up to TRACK_WAVE_BIN wide).  The max starts from 0: a NaN never wins (fmaxf), values below 0 read as 0.
__global__ void __launch_bounds__(256) track_bin_lane_kernel(const float *__restrict__ probs, int C, int cls, track_geom g,
                                                             float scale, uint32_t qmax, uint32_t *__restrict__ q)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < g.nb; j += stride) {
        int64_t lo, hi;
        track_bin_span(g, j, lo, hi);
        float m = 0.0f;
        for (int64_t i = lo - g.offset; i < hi - g.offset; ++i) m = fmaxf(m, probs[i * C + cls]);
        q[j] = track_quantise(m, scale, qmax);
    }
}

// one wave per bin (wider bins)
__global__ void __launch_bounds__(256) track_bin_wave_kernel(const float *__restrict__ probs, int C, int cls, track_geom g,
                                                             float scale, uint32_t qmax, uint32_t *__restrict__ q)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < g.nb; j += waves) {
        int64_t lo, hi;
        track_bin_span(g, j, lo, hi);
        float m = 0.0f;
        for (int64_t i = lo - g.offset + lane; i < hi - g.offset; i += 64) m = fmaxf(m, probs[i * C + cls]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) q[j] = track_quantise(m, scale, qmax);
    }
}

__device__ __forceinline__ int track_decimal_width(uint64_t v)
{
    int w = 1;
    for (uint64_t p = 10; w < 19 && v >= p; p *= 10) ++w;
    return w;
}

// A line "name\tstart\tend\tv.vv\n" is written in two parts: the bin where its run starts writes "name\tstart\t", the bin where it
// ends writes "end\tv.vv\n" (one bin may do both).  The exclusive prefix sum of the parts' bytes over the bins is then where each
// part goes: no per-run arrays.  Bins outside [0, nb) read as q = 0.
struct track_part { uint32_t v; bool first, last; int64_t lo, hi; int64_t head, tail; };

__device__ __forceinline__ track_part track_part_of(const uint32_t *__restrict__ q, const track_geom &g, int64_t j, int64_t name_len,
                                                    int digits)
{
    track_part p;
    p.v = j < g.nb ? q[j] : 0u;
    p.first = p.last = false;
    p.head = p.tail = 0;
    if (p.v == 0) return p;
    p.first = j == 0 || q[j - 1] != p.v;
    p.last = j == g.nb - 1 || q[j + 1] != p.v;
    track_bin_span(g, j, p.lo, p.hi);
    if (p.first) p.head = name_len + track_decimal_width((uint64_t)p.lo) + 2;
    if (p.last) p.tail = track_decimal_width((uint64_t)p.hi) + digits + 4;
    return p;
}

#define TRACK_TILE 2048                  // bins per workgroup: 8 rounds of 256 consecutive bins

// bytes of text per tile
__global__ void __launch_bounds__(256) track_count_kernel(const uint32_t *__restrict__ q, track_geom g, int64_t name_len, int digits,
                                                          uint64_t *__restrict__ tilebytes)
{
    __shared__ uint64_t lds[4];
    uint64_t s = 0;
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const track_part p = track_part_of(q, g, (int64_t)blockIdx.x * TRACK_TILE + r * 256 + threadIdx.x, name_len, digits);
        s += (uint64_t)(p.head + p.tail);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tilebytes[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
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

// The text, in 8 rounds of 256 consecutive bins per tile: neighbouring lanes write neighbouring parts.  The name was copied to
// text[0, name_len) in front of this launch (the head of the first line): the other heads copy it from there, and no lane writes
// text[0, name_len), so no byte is both read and written.
__global__ void __launch_bounds__(256) track_write_kernel(const uint32_t *__restrict__ q, track_geom g, int64_t name_len, int digits,
                                                          uint32_t qmax, const uint64_t *__restrict__ tileoff, char *text)
{
    __shared__ uint64_t lds[4];
    int64_t at = (int64_t)tileoff[blockIdx.x];
    for (int r = 0; r < TRACK_TILE / 256; ++r) {
        const int64_t j = (int64_t)blockIdx.x * TRACK_TILE + r * 256 + threadIdx.x;
        const track_part p = track_part_of(q, g, j, name_len, digits);
        uint64_t round_bytes;
        char *o = text + at + (int64_t)block_exclusive_scan((uint64_t)(p.head + p.tail), &round_bytes, lds);
        at += (int64_t)round_bytes;
        if (p.first) {
            if (o - text >= name_len)
                for (int64_t c = 0; c < name_len; ++c) o[c] = text[c];
            o += name_len;
            *o++ = '\t';
            const int w = track_decimal_width((uint64_t)p.lo);
            track_put_decimal(o, (uint64_t)p.lo, w);
            o += w;
            *o++ = '\t';
        }
        if (p.last) {
            const int w = track_decimal_width((uint64_t)p.hi);
            track_put_decimal(o, (uint64_t)p.hi, w);
            o += w;
            *o++ = '\t';
            *o++ = (char)('0' + p.v / qmax);
            *o++ = '.';
            track_put_decimal(o, p.v % qmax, digits);
            o += digits;
            *o = '\n';
        }
    }
}

static inline int64_t track_bins_bound(int64_t n, int64_t bin) { return n / bin + 2; }

}   // namespace

#define TRACK_MAX_EXTENT (1ll << 40)     // n, offset and bin: far beyond any genome; no product overflows, tiles fit a grid

DGRP_EXPORT int64_t dgrp_track_workspace_bytes(int64_t n, int64_t bin)
{
    if (n < 0 || n > TRACK_MAX_EXTENT || bin < 1 || bin > TRACK_MAX_EXTENT) return 0;
    const int64_t nb = track_bins_bound(n, bin);
    return 256 + dgrp_align_up(nb * 4, 256) + dgrp_align_up((nb + TRACK_TILE - 1) / TRACK_TILE * 8, 256);
}

DGRP_EXPORT int dgrp_track_text(const float *d_probs, int64_t n, int C, int cls, int digits, int64_t bin, int64_t offset,
                                const char *name, int64_t name_len, char *d_text, int64_t cap, int64_t *h_bytes,
                                void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(h_bytes, "dgrp_track_text: NULL h_bytes");
    DGRP_REQUIRE(n >= 0 && n <= TRACK_MAX_EXTENT, "dgrp_track_text: bad n %lld", (long long)n);
    DGRP_REQUIRE(C >= 1 && C <= DGRP_MAXC && cls >= 0 && cls < C, "dgrp_track_text: bad C/cls (%d, %d)", C, cls);
    DGRP_REQUIRE(digits >= 1 && digits <= 4, "dgrp_track_text: digits must lie in 1..4, got %d", digits);
    DGRP_REQUIRE(bin >= 1 && bin <= TRACK_MAX_EXTENT, "dgrp_track_text: bad bin %lld", (long long)bin);
    DGRP_REQUIRE(offset >= 0 && offset <= TRACK_MAX_EXTENT, "dgrp_track_text: bad offset %lld", (long long)offset);
    DGRP_REQUIRE(name_len >= 0 && cap >= 0, "dgrp_track_text: bad name_len/cap");
    DGRP_REQUIRE((name || name_len == 0) && (d_text || cap == 0) && (n == 0 || (d_probs && d_work)),
                 "dgrp_track_text: NULL pointer");
    *h_bytes = 0;
    if (n == 0) return DGRP_OK;
    if (work_bytes < dgrp_track_workspace_bytes(n, bin)) {
        dgrp_set_error("dgrp_track_text: workspace %lld < %lld bytes", (long long)work_bytes,
                       (long long)dgrp_track_workspace_bytes(n, bin));
        return DGRP_ENOMEM;
    }
    track_geom g;
    g.offset = offset;
    g.n = n;
    g.bin = bin;
    g.kb0 = offset / bin;
    g.nb = (offset + n - 1) / bin - g.kb0 + 1;
    const int64_t ntiles = (g.nb + TRACK_TILE - 1) / TRACK_TILE;
    uint64_t *grand = (uint64_t *)d_work;                                    // total bytes
    uint32_t *q = (uint32_t *)((char *)d_work + 256);
    uint64_t *tiles = (uint64_t *)((char *)q + dgrp_align_up(track_bins_bound(n, bin) * 4, 256));   // bytes per tile -> offsets
    uint32_t qmax = 1;
    for (int k = 0; k < digits; ++k) qmax *= 10;
    const float scale = (float)qmax;

    if (bin <= TRACK_WAVE_BIN) {
        hipLaunchKernelGGL(track_bin_lane_kernel, dim3(grid_for(g.nb, 256)), dim3(256), 0, stream, d_probs, C, cls, g, scale, qmax, q);
    } else {
        hipLaunchKernelGGL(track_bin_wave_kernel, dim3(grid_for(g.nb * 64, 256)), dim3(256), 0, stream, d_probs, C, cls, g, scale, qmax, q);
    }
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(track_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, q, g, name_len, digits, tiles);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, tiles, ntiles, grand);
    DGRP_LAUNCH_CHECK();
    uint64_t total = 0;
    DGRP_HIP(hipMemcpyAsync(&total, grand, 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    *h_bytes = (int64_t)total;
    if (total == 0 || (int64_t)total > cap) return DGRP_OK;                 // (too small: the caller retries with room for all of it)
    if (name_len > 0) DGRP_HIP(hipMemcpyAsync(d_text, name, (size_t)name_len, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(track_write_kernel, dim3((unsigned)ntiles), dim3(256), 0, stream, q, g, name_len, digits, qmax, tiles, d_text);
    DGRP_LAUNCH_CHECK();
    DGRP_HIP(hipStreamSynchronize(stream));
    return DGRP_OK;
}
