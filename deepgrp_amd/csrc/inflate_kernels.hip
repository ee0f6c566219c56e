// Compressed input: gzip / BGZF members inflated on the device, one wave per member, with the decode core of inflate.h; and the
// same core on the host for one raw DEFLATE stream (include/deepgrp_hip.h).
//
// Plan: the Huffman decode is serial, so every lane of the wave runs it on the same state (the tables live in LDS, every lane reads
// the same entry), lane 0 writes the literals, and the copies of a match or a stored block are spread over the 64 lanes.  A match
// copy reads only bytes before its own start (out[pos + j] = out[pos - dist + j mod dist]), so the lanes of one copy never wait
// for each other.  Afterwards each lane takes the CRC-32 of 1/64 of the member's output and the 64 CRCs are combined into the
// member's, which is compared with the trailer on the device together with ISIZE.
#include "dgrp_common.h"
#include "inflate.h"
#include <vector>

struct inflate_wave_sink {
    uint8_t *out;
    uint32_t lane;
    __device__ void literal(uint32_t pos, uint32_t b)
    {
        if (lane == 0) out[pos] = (uint8_t)b;
    }
    // (lanes of one wave see each other's earlier global stores in program order; the fence keeps the compiler from moving the
    // loads of a copy above the stores in front of it)
    __device__ void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const uint8_t *src = out + pos - dist;
        uint8_t *dst = out + pos;
        for (uint32_t j = lane; j < len; j += 64) dst[j] = src[j < dist ? j : j % dist];
    }
    __device__ void stored(uint32_t pos, const uint8_t *src, uint32_t len)
    {
        uint8_t *dst = out + pos;
        for (uint32_t j = lane; j < len; j += 64) dst[j] = src[j];
    }
};

// one workgroup (one wave) per member; tab = in_off[nmem], in_len[nmem], out_off[nmem + 1]
__global__ void __launch_bounds__(64) inflate_member_kernel(const uint8_t *__restrict__ in, const int64_t *__restrict__ tab, int64_t nmem,
                                                            uint8_t *__restrict__ out, int32_t *__restrict__ status)
{
    __shared__ dgrp_inflate_tables t;
    __shared__ uint32_t crctab[256];
    const uint32_t lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    const uint8_t *src = in + tab[m];
    const uint32_t n_in = (uint32_t)tab[nmem + m];
    const int64_t o0 = tab[2 * nmem + m];
    uint8_t *dst = out + o0;
    const uint32_t cap = (uint32_t)(tab[2 * nmem + m + 1] - o0);
    inflate_wave_sink sink{dst, lane};
    uint32_t produced = 0, used = 0;
    int rc = dgrp_inflate_core(src, n_in, cap, &t, sink, &produced, &used);
    if (rc == DGRP_INFLATE_OK && used != n_in) rc = DGRP_INFLATE_ETRAIL;
    const uint32_t crc_want = dgrp_le32(src + n_in), isize = dgrp_le32(src + n_in + 4);
    if (rc == DGRP_INFLATE_OK && produced != isize) rc = produced < isize ? DGRP_INFLATE_EISIZE : DGRP_INFLATE_EOUTPUT;
    if (rc == DGRP_INFLATE_OK) {                         // (the same for every lane)
        const uint32_t seg = (produced + 63) / 64;
        const uint32_t a = min(lane * seg, produced), b = min(a + seg, produced);
        if (dgrp_crc_wave(dst + a, dst + b, crctab) != crc_want) rc = DGRP_INFLATE_ECRC;
    }
    if (lane == 0) status[m] = rc;
}

DGRP_EXPORT int dgrp_inflate_raw_host(const uint8_t *h_in, int64_t in_len, uint8_t *h_out, int64_t out_cap, int64_t *h_out_len,
                                      int64_t *h_in_used, int *h_reason)
{
    DGRP_REQUIRE(h_out_len && h_in_used && h_reason, "dgrp_inflate_raw_host: bad arguments");
    DGRP_REQUIRE(in_len >= 0 && out_cap >= 0 && in_len <= INT32_MAX && out_cap <= INT32_MAX, "dgrp_inflate_raw_host: bad sizes");
    DGRP_REQUIRE((h_in || in_len == 0) && (h_out || out_cap == 0), "dgrp_inflate_raw_host: NULL pointer");
    dgrp_inflate_tables t;
    dgrp_host_sink sink{h_out};
    uint32_t produced = 0, used = 0;
    const int rc = dgrp_inflate_core(h_in, (uint32_t)in_len, (uint32_t)out_cap, &t, sink, &produced, &used);
    *h_out_len = produced;
    *h_in_used = used;
    *h_reason = rc;
    if (rc != DGRP_INFLATE_OK) {
        dgrp_set_error("dgrp_inflate_raw_host: %s (reason %d) near input byte %u", dgrp_inflate_reason_text(rc, false), rc, used);
        return DGRP_EDATA;
    }
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_inflate_workspace_bytes(int64_t nmem)
{
    if (nmem < 0) return 0;
    return dgrp_align_up((3 * nmem + 1) * 8, 256) + dgrp_align_up(nmem * 4, 256);
}

DGRP_EXPORT int dgrp_inflate_batch(const uint8_t *d_in, int64_t in_bytes, int64_t nmem, const int64_t *h_in_off, const int64_t *h_in_len,
                                   const int64_t *h_out_off, uint8_t *d_out, int64_t out_bytes, int64_t *h_bad, int *h_reason,
                                   void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(nmem >= 0 && nmem <= INT32_MAX && in_bytes >= 0 && out_bytes >= 0 && h_bad && h_reason,
                 "dgrp_inflate_batch: bad arguments");
    *h_bad = -1;
    *h_reason = 0;
    if (nmem == 0) return DGRP_OK;
    DGRP_REQUIRE(h_in_off && h_in_len && h_out_off, "dgrp_inflate_batch: NULL member table");
    DGRP_REQUIRE(h_out_off[0] >= 0 && h_out_off[nmem] <= out_bytes, "dgrp_inflate_batch: output offsets outside the output");
    for (int64_t m = 0; m < nmem; ++m) {
        DGRP_REQUIRE(h_in_off[m] >= 0 && h_in_len[m] >= 0 && h_in_len[m] <= INT32_MAX && h_in_off[m] <= in_bytes - 8 - h_in_len[m],
                     "dgrp_inflate_batch: member %lld: input range outside the input", (long long)m);
        const int64_t n = h_out_off[m + 1] - h_out_off[m];
        DGRP_REQUIRE(n >= 0 && n <= INT32_MAX, "dgrp_inflate_batch: member %lld: bad output range", (long long)m);
    }
    DGRP_REQUIRE(d_in && d_work && (d_out || h_out_off[nmem] == h_out_off[0]), "dgrp_inflate_batch: NULL pointer");
    if (work_bytes < dgrp_inflate_workspace_bytes(nmem)) {
        dgrp_set_error("dgrp_inflate_batch: workspace too small");
        return DGRP_ENOMEM;
    }
    std::vector<int64_t> tab((size_t)(3 * nmem + 1));
    std::copy(h_in_off, h_in_off + nmem, tab.begin());
    std::copy(h_in_len, h_in_len + nmem, tab.begin() + nmem);
    std::copy(h_out_off, h_out_off + nmem + 1, tab.begin() + 2 * nmem);
    int64_t *d_tab = (int64_t *)d_work;
    int32_t *d_status = (int32_t *)((char *)d_work + dgrp_align_up((3 * nmem + 1) * 8, 256));
    DGRP_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(inflate_member_kernel, dim3((unsigned)nmem), dim3(64), 0, stream, d_in, d_tab, nmem, d_out, d_status);
    DGRP_LAUNCH_CHECK();
    std::vector<int32_t> status((size_t)nmem);
    DGRP_HIP(hipMemcpyAsync(status.data(), d_status, (size_t)nmem * 4, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    for (int64_t m = 0; m < nmem; ++m) {
        if (status[(size_t)m] != DGRP_INFLATE_OK) {
            *h_bad = m;
            *h_reason = status[(size_t)m];
            dgrp_set_error("dgrp_inflate_batch: member %lld: %s (reason %d)", (long long)m, dgrp_inflate_reason_text(status[(size_t)m], false),
                           status[(size_t)m]);
            return DGRP_EDATA;
        }
    }
    return DGRP_OK;
}
