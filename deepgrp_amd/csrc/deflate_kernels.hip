// BGZF output: members deflated on the device, one workgroup per member, with the encode core of deflate.h; and the same core on
// the host (dgrp_bgzf_compress_host), which gives the same bytes.
//
// Plan per member (at most 0xff00 input bytes, read twice):
//   1. every thread takes 16-byte runs of the input (run r of thread t: r = t, t + 256, ...): byte histogram in LDS (one per wave,
//      integer atomics) and the raw CRC-32 of its runs, carried from one run to the next by a multiplication with x^(8 * 4096);
//   2. the symbols are ranked by (count, value), one thread per symbol; thread 0 runs the serial plan (code lengths, codes, header);
//   3. the runs again: a run's bit count is the sum of its code lengths, the workgroup scans the counts (scan.h), and every thread
//      packs its codes into a 64-bit accumulator and writes whole 32-bit words into an LDS image of the member -- words it shares
//      with a neighbouring run, the header or the end-of-block code through ds_or_b32 on the zeroed image, its own words as stores;
//   4. the image (header, block, CRC-32, ISIZE) leaves LDS as 16-byte stores into the member's fixed-stride slot.
// Then the member sizes are scanned and a second kernel places the members back to back (16-byte stores where the destination
// allows), with the EOF member behind them on request.  Only the total is read back.
#include "dgrp_common.h"
#include "deflate.h"
#include "scan.h"
#include <string.h>
#include <mutex>
#include <vector>

namespace {

#define DEFLATE_THREADS 256
#define DEFLATE_RUN 16
#define DEFLATE_ROUND (DEFLATE_THREADS * DEFLATE_RUN)      // input bytes between two runs of one thread

struct deflate_lds {
    uint32_t image[DGRP_BGZF_SLOT / 4];                    // the member as it leaves
    dgrp_deflate_plan plan;
    uint32_t hist[DEFLATE_THREADS / 64][DGRP_DEFLATE_NSYM];
    uint32_t crctab[256];
    uint64_t scan[4];
    uint32_t crc[DEFLATE_THREADS / 64];
};

// the (at most 16) bytes of a run: one 16-byte load when it is whole (any address: the input may start anywhere)
struct deflate_run {
    uint32_t w[4];
    __device__ __forceinline__ uint32_t byte(int j) const { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }   // j: a constant
};
__device__ __forceinline__ deflate_run deflate_load_run(const uint8_t *p, uint32_t k)
{
    deflate_run v;
    if (k == DEFLATE_RUN) {
        __builtin_memcpy(v.w, p, 16);
    } else {
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
#pragma unroll
        for (int j = 0; j < DEFLATE_RUN; ++j)
            if ((uint32_t)j < k) v.w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    return v;
}

// x^(8 * 16 * j) modulo the CRC polynomial, j < 4096: a product over the bits of j of constants
__device__ __forceinline__ uint32_t deflate_x128n(uint32_t j)
{
    constexpr uint32_t c[12] = {dgrp_crc_x8n(16u << 0), dgrp_crc_x8n(16u << 1), dgrp_crc_x8n(16u << 2),  dgrp_crc_x8n(16u << 3),
                                dgrp_crc_x8n(16u << 4), dgrp_crc_x8n(16u << 5), dgrp_crc_x8n(16u << 6),  dgrp_crc_x8n(16u << 7),
                                dgrp_crc_x8n(16u << 8), dgrp_crc_x8n(16u << 9), dgrp_crc_x8n(16u << 10), dgrp_crc_x8n(16u << 11)};
    uint32_t p = 0x80000000u;
#pragma unroll
    for (int b = 0; b < 12; ++b)
        if (j & (1u << b)) p = dgrp_crc_multmodp(c[b], p);
    return p;
}

// one workgroup per member m: in[m * 0xff00 ...) -> slots[m * DGRP_BGZF_SLOT ...), sizes[m]
__global__ void __launch_bounds__(DEFLATE_THREADS) deflate_member_kernel(const uint8_t *__restrict__ in, int64_t n,
                                                                         uint8_t *__restrict__ slots, uint64_t *__restrict__ sizes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char deflate_smem[];
    deflate_lds &L = *reinterpret_cast<deflate_lds *>(deflate_smem);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    const uint8_t *src = in + m * DGRP_BGZF_BLOCK;
    const int64_t left = n - m * DGRP_BGZF_BLOCK;
    const uint32_t len = left < DGRP_BGZF_BLOCK ? (uint32_t)left : DGRP_BGZF_BLOCK;
    const uint32_t nrun = (len + DEFLATE_RUN - 1) / DEFLATE_RUN;

    for (uint32_t i = tid; i < DGRP_BGZF_SLOT / 4; i += DEFLATE_THREADS) L.image[i] = 0;
    for (uint32_t i = tid; i < (DEFLATE_THREADS / 64) * DGRP_DEFLATE_NSYM; i += DEFLATE_THREADS) (&L.hist[0][0])[i] = 0;
    L.crctab[tid] = dgrp_crc_table_entry(tid);
    __syncthreads();

    // ---- 1. histogram and CRC-32
    constexpr uint32_t x_round = dgrp_crc_x8n(DEFLATE_ROUND);
    uint32_t crc = 0, end = 0;                               // raw CRC (register starts at 0) of this thread's runs up to byte `end`
    for (uint32_t r = tid; r < nrun; r += DEFLATE_THREADS) {
        const uint32_t at = r * DEFLATE_RUN, k = min(len - at, (uint32_t)DEFLATE_RUN);
        const deflate_run v = deflate_load_run(src + at, k);
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < DEFLATE_RUN; ++j) {
            if ((uint32_t)j < k) {
                const uint32_t b = v.byte(j);
                atomicAdd(&L.hist[wave][b], 1u);
                c = L.crctab[(c ^ b) & 0xffu] ^ (c >> 8);
            }
        }
        if (r != tid) crc = dgrp_crc_multmodp(k == DEFLATE_RUN ? x_round : dgrp_crc_x8n(at + k - end), crc);
        crc ^= c;
        end = at + k;
    }
    if (end != 0 && end != len) {
        // the bytes behind this thread's last run: whole runs, then the member's last run of 1..16 bytes
        const uint32_t tail = len - (nrun - 1) * DEFLATE_RUN;
        crc = dgrp_crc_multmodp(deflate_x128n((len - tail - end) / DEFLATE_RUN), crc);
        crc = dgrp_crc_multmodp(dgrp_crc_x8n(tail), crc);
    }
    for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o);
    if (lane == 0) L.crc[wave] = crc;
    __syncthreads();
    for (uint32_t s = tid; s < DGRP_DEFLATE_NSYM; s += DEFLATE_THREADS) {
        uint32_t f = 0;
        for (int w = 0; w < DEFLATE_THREADS / 64; ++w) f += L.hist[w][s];
        L.plan.freq[s] = s == 256 ? 1u : f;
    }
    __syncthreads();

    // ---- 2. the plan
    for (uint32_t s = tid; s < DGRP_DEFLATE_NSYM; s += DEFLATE_THREADS) dgrp_deflate_place(&L.plan, (int)s);
    __syncthreads();
    if (tid == 0) dgrp_deflate_plan_member(&L.plan, len);
    __syncthreads();
    const uint32_t hdr_end = L.plan.hdr_end, deflate_bytes = L.plan.deflate_bytes;
    const bool stored = L.plan.stored != 0;
    if (tid < 4) L.image[tid] = dgrp_bgzf_head_word((int)tid);
    if (tid < (hdr_end + 31) / 32) L.image[4 + tid] = L.plan.hdr[tid];
    __syncthreads();

    // ---- 3. the body
    if (stored) {
        uint8_t *body = reinterpret_cast<uint8_t *>(L.image) + 16 + hdr_end / 8;
        for (uint32_t i = tid; i < len; i += DEFLATE_THREADS) body[i] = src[i];
    } else {
        uint32_t *img = L.image + 4;
        uint64_t carry = hdr_end;
        for (uint32_t base = 0; base < nrun; base += DEFLATE_THREADS) {
            const uint32_t r = base + tid, at = r * DEFLATE_RUN;
            const uint32_t k = r < nrun ? min(len - at, (uint32_t)DEFLATE_RUN) : 0;
            deflate_run v;
            v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
            if (k) v = deflate_load_run(src + at, k);
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j)
                if ((uint32_t)j < k) bits += L.plan.table[v.byte(j)] >> 16;
            uint64_t total;
            const uint64_t pos = block_exclusive_scan(bits, &total, L.scan) + carry;
            carry += total;
            uint32_t w = (uint32_t)(pos >> 5), nb = (uint32_t)pos & 31u;
            uint64_t acc = 0;
            bool shared = true;                               // the run's first word may hold a neighbour's bits as well
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j) {
                const uint32_t e = (uint32_t)j < k ? L.plan.table[v.byte(j)] : 0u;     // (nothing behind the run: no bits)
                acc |= (uint64_t)(e & 0xffffu) << nb;
                nb += e >> 16;
                if (nb >= 32) {
                    if (shared) atomicOr(&img[w], (uint32_t)acc);
                    else img[w] = (uint32_t)acc;
                    shared = false;
                    ++w;
                    acc >>= 32;
                    nb -= 32;
                }
            }
            if (nb && k) atomicOr(&img[w], (uint32_t)acc);
        }
        if (tid == 0) {
            const uint32_t e = L.plan.table[256], s = (uint32_t)carry & 31u, w = (uint32_t)(carry >> 5);
            const uint64_t acc = (uint64_t)(e & 0xffffu) << s;
            atomicOr(&img[w], (uint32_t)acc);
            if (s + (e >> 16) > 32) atomicOr(&img[w + 1], (uint32_t)(acc >> 32));
        }
    }
    __syncthreads();

    // ---- 4. trailer, and out
    const uint32_t total = 18 + deflate_bytes + 8;
    if (tid < 8) {
        uint32_t c = L.crc[0];
        for (int w = 1; w < DEFLATE_THREADS / 64; ++w) c ^= L.crc[w];
        c ^= dgrp_crc_multmodp(dgrp_crc_x8n(len), 0xffffffffu) ^ 0xffffffffu;     // the register's start value carried over len bytes
        const uint32_t word = tid < 4 ? c : len;
        reinterpret_cast<uint8_t *>(L.image)[18 + deflate_bytes + tid] = (uint8_t)(word >> (8 * (tid & 3)));
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(slots + m * DGRP_BGZF_SLOT);
    const uint4 *img16 = reinterpret_cast<const uint4 *>(L.image);
    for (uint32_t q = tid; q < (total + 15) / 16; q += DEFLATE_THREADS) dst[q] = img16[q];
    if (tid == 0) sizes[m] = total;
}

__device__ __forceinline__ uint8_t bgzf_eof_byte(uint32_t i)
{
    if (i < 16) return (uint8_t)(dgrp_bgzf_head_word((int)(i >> 2)) >> (8 * (i & 3)));
    return i == 16 ? 0x1b : i == 18 ? 0x03 : 0;
}

// offs = exclusive scan of the member sizes with the total at offs[nmem]; workgroup m < nmem copies member m, workgroup nmem
// writes the EOF member.  Nothing is written when the whole does not fit out_cap.
__global__ void __launch_bounds__(256) bgzf_place_kernel(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ offs, int64_t nmem,
                                                        int eof, uint8_t *__restrict__ out, int64_t out_cap)
{
    const uint64_t all = offs[nmem];
    if ((int64_t)all + (eof ? DGRP_BGZF_EOF_BYTES : 0) > out_cap) return;
    const int64_t m = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    if (m == nmem) {
        if (tid < DGRP_BGZF_EOF_BYTES) out[all + tid] = bgzf_eof_byte(tid);
        return;
    }
    const uint8_t *src = slots + m * DGRP_BGZF_SLOT;
    uint8_t *dst = out + offs[m];
    const uint32_t size = (uint32_t)(offs[m + 1] - offs[m]);
    const uint32_t head = min(size, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    const uint32_t nq = (size - head) / 16, tail0 = head + nq * 16;
    if (tid < head) dst[tid] = src[tid];
    for (uint32_t q = tid; q < nq; q += 256) {
        uint4 v;
        __builtin_memcpy(&v, src + head + q * 16, 16);
        *reinterpret_cast<uint4 *>(dst + head + q * 16) = v;
    }
    if (tid < size - tail0) dst[tail0 + tid] = src[tail0 + tid];
}

static inline int64_t bgzf_members(int64_t n) { return (n + DGRP_BGZF_BLOCK - 1) / DGRP_BGZF_BLOCK; }

static const uint8_t BGZF_EOF_MEMBER[DGRP_BGZF_EOF_BYTES] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0,
                                                            0,    0,    0, 0, 0, 0, 0, 0};

}   // namespace

DGRP_EXPORT int64_t dgrp_bgzf_bound(int64_t n, int eof)
{
    if (n < 0) return 0;
    return n + 31 * bgzf_members(n) + (eof ? DGRP_BGZF_EOF_BYTES : 0);
}

DGRP_EXPORT int64_t dgrp_bgzf_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    const int64_t nmem = bgzf_members(n);
    return dgrp_align_up(nmem * DGRP_BGZF_SLOT, 256) + dgrp_align_up((nmem + 1) * 8, 256);
}

DGRP_EXPORT int dgrp_bgzf_compress(const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                                   void *d_work, int64_t work_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DGRP_REQUIRE(n >= 0 && out_cap >= 0 && work_bytes >= 0 && h_out_bytes, "dgrp_bgzf_compress: bad arguments");
    *h_out_bytes = 0;
    const int64_t nmem = bgzf_members(n);
    DGRP_REQUIRE(nmem <= INT32_MAX - 1, "dgrp_bgzf_compress: too many members");
    DGRP_REQUIRE(n == 0 || (d_in && d_work), "dgrp_bgzf_compress: NULL pointer");
    DGRP_REQUIRE(d_out || (n == 0 && !eof) || out_cap == 0, "dgrp_bgzf_compress: NULL pointer");
    if (n == 0) {
        if (!eof) return DGRP_OK;
        *h_out_bytes = DGRP_BGZF_EOF_BYTES;
        if (out_cap < DGRP_BGZF_EOF_BYTES) {
            dgrp_set_error("dgrp_bgzf_compress: output of %lld bytes, the EOF member takes %d", (long long)out_cap, DGRP_BGZF_EOF_BYTES);
            return DGRP_ENOMEM;
        }
        DGRP_HIP(hipMemcpyAsync(d_out, BGZF_EOF_MEMBER, DGRP_BGZF_EOF_BYTES, hipMemcpyHostToDevice, stream));
        DGRP_HIP(hipStreamSynchronize(stream));
        return DGRP_OK;
    }
    if (work_bytes < dgrp_bgzf_workspace_bytes(n)) {
        dgrp_set_error("dgrp_bgzf_compress: workspace too small");
        return DGRP_ENOMEM;
    }
    DGRP_REQUIRE(((uintptr_t)d_work & 15) == 0, "dgrp_bgzf_compress: d_work must be 16-byte aligned");
    static std::once_flag configured;
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] {
        cfg_err = hipFuncSetAttribute((const void *)deflate_member_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(deflate_lds));
    });
    DGRP_HIP(cfg_err);
    uint8_t *slots = (uint8_t *)d_work;
    uint64_t *sizes = (uint64_t *)(slots + dgrp_align_up(nmem * DGRP_BGZF_SLOT, 256));
    hipLaunchKernelGGL(deflate_member_kernel, dim3((unsigned)nmem), dim3(DEFLATE_THREADS), sizeof(deflate_lds), stream, d_in, n, slots, sizes);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, sizes, nmem, sizes + nmem);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bgzf_place_kernel, dim3((unsigned)(nmem + (eof ? 1 : 0))), dim3(256), 0, stream, slots, sizes, nmem, eof, d_out, out_cap);
    DGRP_LAUNCH_CHECK();
    uint64_t all = 0;
    DGRP_HIP(hipMemcpyAsync(&all, sizes + nmem, 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    *h_out_bytes = (int64_t)all + (eof ? DGRP_BGZF_EOF_BYTES : 0);
    if (*h_out_bytes > out_cap) {
        dgrp_set_error("dgrp_bgzf_compress: output of %lld bytes, %lld needed (nothing written)", (long long)out_cap, (long long)*h_out_bytes);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_bgzf_compress_host(const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes, int eof)
{
    DGRP_REQUIRE(n >= 0 && out_cap >= 0 && h_out_bytes, "dgrp_bgzf_compress_host: bad arguments");
    *h_out_bytes = 0;
    DGRP_REQUIRE(h_in || n == 0, "dgrp_bgzf_compress_host: NULL pointer");
    DGRP_REQUIRE(h_out || (n == 0 && !eof) || out_cap == 0, "dgrp_bgzf_compress_host: NULL pointer");
    std::vector<uint32_t> slot(DGRP_BGZF_SLOT / 4);
    dgrp_deflate_plan plan;
    int64_t pos = 0;
    bool fits = true;                                        // once a member does not fit nothing more is written, only counted
    for (int64_t o = 0; o < n; o += DGRP_BGZF_BLOCK) {
        const uint32_t k = (uint32_t)(n - o < DGRP_BGZF_BLOCK ? n - o : DGRP_BGZF_BLOCK);
        const uint32_t size = dgrp_bgzf_member_serial(h_in + o, k, slot.data(), &plan);
        fits = fits && pos + size <= out_cap;
        if (fits) memcpy(h_out + pos, slot.data(), size);
        pos += size;
    }
    if (eof) {
        fits = fits && pos + DGRP_BGZF_EOF_BYTES <= out_cap;
        if (fits) memcpy(h_out + pos, BGZF_EOF_MEMBER, DGRP_BGZF_EOF_BYTES);
        pos += DGRP_BGZF_EOF_BYTES;
    }
    *h_out_bytes = pos;
    if (!fits) {
        dgrp_set_error("dgrp_bgzf_compress_host: output of %lld bytes, %lld needed", (long long)out_cap, (long long)pos);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}
