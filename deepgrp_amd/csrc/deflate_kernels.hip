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
// Level 1 (deflate_lz_member_kernel, deflate.h's second level) puts four stages in front of the body, with the text in LDS:
//   a. candidates and lengths, in tiles of 256 positions (one per thread): a tile reads the bucket table in LDS (its state is every
//      earlier tile), looks for the nearest equal key among the tile's own earlier positions, and the last position of each key in
//      the tile stores itself into the table -- one writer per bucket and tile, so no atomics and no order; then the common prefix
//      at the nearer candidate, four bytes a step; one word per position goes to the member's part of the workspace;
//   b. the parse, tile by tile: reachability inside a tile by pointer doubling over the tile's jumps (at most 8 rounds, fewer when
//      a round adds nothing), the position that jumps out of the tile carries the entry into the next one; the positions reached
//      count their symbols into the two histograms;
//   c. both plans side by side (level 0's on one wave, level 1's on another), and the smaller block is the member;
//   d. the body as in 3., a run's bits now being those of its tokens (up to 20 bits of literal/length, up to 28 of distance).
// The image shares its LDS with the bucket table, which is dead by then.
// Then the member sizes are scanned and a second kernel places the members back to back (16-byte stores where the destination
// allows), with the EOF member behind them on request.  Only the total is read back.
#include "dgrp_common.h"
#include "deflate.h"
#include "deflate_blocks.h"
#include "scan.h"
#include <string.h>
#include <mutex>
#include <vector>

namespace {

#define DEFLATE_THREADS 256
#define DEFLATE_RUN 16
#define DEFLATE_ROUND (DEFLATE_THREADS * DEFLATE_RUN)      // input bytes between two runs of one thread

struct deflate_shared {
    dgrp_deflate_plan plan;
    uint32_t hist[DEFLATE_THREADS / 64][DGRP_DEFLATE_NSYM];
    uint32_t crctab[256];
    uint64_t scan[4];
    uint32_t crc[DEFLATE_THREADS / 64];
};
struct deflate_lds {
    uint32_t image[DGRP_BGZF_SLOT / 4];                    // the member as it leaves
    deflate_shared s;
};
#define DEFLATE_LZ_TILE DEFLATE_THREADS
struct deflate_lz_lds {
    union {
        uint32_t image[DGRP_BGZF_SLOT / 4];
        uint16_t table[1 << DGRP_LZ_HASH_BITS];            // bucket -> its last position so far, 0xffff: none
    };
    deflate_shared s;
    dgrp_lz_plan lz;
    alignas(16) uint32_t text[(DGRP_BGZF_BLOCK + 16) / 4]; // the member's bytes, zeros behind them
    alignas(16) uint32_t tkey[DEFLATE_LZ_TILE];            // the tile's keys (read four at a time)
    uint16_t jump[DEFLATE_LZ_TILE];
    uint8_t flag[DEFLATE_LZ_TILE];                         // a: a later position of the tile has this key; b: reached
    uint32_t entry;
};
static_assert(sizeof(deflate_lz_lds) <= 160 * 1024, "deflate_lz_lds exceeds the CU's LDS");

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

// ---- 1. histogram and CRC-32 of src[0, len) (hist and crctab are set, the workgroup in step): S.plan.freq and S.crc
__device__ __forceinline__ void deflate_hist_crc(const uint8_t *__restrict__ src, uint32_t len, uint32_t nrun, deflate_shared &S)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
                atomicAdd(&S.hist[wave][b], 1u);
                c = S.crctab[(c ^ b) & 0xffu] ^ (c >> 8);
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
    if (lane == 0) S.crc[wave] = crc;
    __syncthreads();
    for (uint32_t s = tid; s < DGRP_DEFLATE_NSYM; s += DEFLATE_THREADS) {
        uint32_t f = 0;
        for (int w = 0; w < DEFLATE_THREADS / 64; ++w) f += S.hist[w][s];
        S.plan.freq[s] = s == 256 ? 1u : f;
    }
    __syncthreads();
}

// ---- 3. level 0's body into the zeroed image that holds the header (S.plan is made)
__device__ __forceinline__ void deflate_body_literals(const uint8_t *__restrict__ src, uint32_t len, uint32_t nrun, uint32_t *image,
                                                      deflate_shared &S)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t hdr_end = S.plan.hdr_end;
    if (S.plan.stored != 0) {
        uint8_t *body = reinterpret_cast<uint8_t *>(image) + 16 + hdr_end / 8;
        for (uint32_t i = tid; i < len; i += DEFLATE_THREADS) body[i] = src[i];
    } else {
        uint32_t *img = image + 4;
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
                if ((uint32_t)j < k) bits += S.plan.table[v.byte(j)] >> 16;
            uint64_t total;
            const uint64_t pos = block_exclusive_scan(bits, &total, S.scan) + carry;
            carry += total;
            uint32_t w = (uint32_t)(pos >> 5), nb = (uint32_t)pos & 31u;
            uint64_t acc = 0;
            bool shared = true;                               // the run's first word may hold a neighbour's bits as well
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j) {
                const uint32_t e = (uint32_t)j < k ? S.plan.table[v.byte(j)] : 0u;     // (nothing behind the run: no bits)
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
            const uint32_t e = S.plan.table[256], s = (uint32_t)carry & 31u, w = (uint32_t)(carry >> 5);
            const uint64_t acc = (uint64_t)(e & 0xffffu) << s;
            atomicOr(&img[w], (uint32_t)acc);
            if (s + (e >> 16) > 32) atomicOr(&img[w + 1], (uint32_t)(acc >> 32));
        }
    }
    __syncthreads();
}

// ---- 4. trailer, and out
__device__ __forceinline__ void deflate_finish(uint32_t len, uint32_t deflate_bytes, uint32_t *image, deflate_shared &S, uint8_t *__restrict__ slot,
                                               uint64_t *__restrict__ size)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t total = 18 + deflate_bytes + 8;
    if (tid < 8) {
        uint32_t c = S.crc[0];
        for (int w = 1; w < DEFLATE_THREADS / 64; ++w) c ^= S.crc[w];
        c ^= dgrp_crc_multmodp(dgrp_crc_x8n(len), 0xffffffffu) ^ 0xffffffffu;     // the register's start value carried over len bytes
        const uint32_t word = tid < 4 ? c : len;
        reinterpret_cast<uint8_t *>(image)[18 + deflate_bytes + tid] = (uint8_t)(word >> (8 * (tid & 3)));
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(slot);
    const uint4 *img16 = reinterpret_cast<const uint4 *>(image);
    for (uint32_t q = tid; q < (total + 15) / 16; q += DEFLATE_THREADS) dst[q] = img16[q];
    if (tid == 0) *size = total;
}

// where member m's bytes lie: in[m * 0xff00 ...) of n bytes, or, with a block table (rows of `stride` bytes that begin with int64
// offset and int64 length <= 0xff00), in[offset ...); a row that does not lie in in[0, n) reads as empty
__device__ __forceinline__ const uint8_t *deflate_member_src(const uint8_t *__restrict__ in, int64_t n, const char *__restrict__ rows,
                                                             int64_t stride, int64_t m, uint32_t &len)
{
    if (rows) {
        const int64_t *row = reinterpret_cast<const int64_t *>(rows + m * stride);
        const bool ok = row[0] >= 0 && row[1] >= 0 && row[1] <= DGRP_BGZF_BLOCK && row[0] <= n - row[1];
        len = ok ? (uint32_t)row[1] : 0u;
        return in + (ok ? row[0] : 0);
    }
    const int64_t left = n - m * DGRP_BGZF_BLOCK;
    len = left < DGRP_BGZF_BLOCK ? (uint32_t)left : DGRP_BGZF_BLOCK;
    return in + m * DGRP_BGZF_BLOCK;
}

// one workgroup per member m: its bytes (deflate_member_src) -> slots[m * DGRP_BGZF_SLOT ...), sizes[m]
__global__ void __launch_bounds__(DEFLATE_THREADS) deflate_member_kernel(const uint8_t *__restrict__ in, int64_t n,
                                                                         const char *__restrict__ rows, int64_t stride,
                                                                         uint8_t *__restrict__ slots, uint64_t *__restrict__ sizes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char deflate_smem[];
    deflate_lds &L = *reinterpret_cast<deflate_lds *>(deflate_smem);
    const uint32_t tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    uint32_t len;
    const uint8_t *src = deflate_member_src(in, n, rows, stride, m, len);
    if (len == 0) {                                           // (uniform; a table's empty block: no member, the caller frames it)
        if (tid == 0) sizes[m] = 0;
        return;
    }
    const uint32_t nrun = (len + DEFLATE_RUN - 1) / DEFLATE_RUN;

    for (uint32_t i = tid; i < DGRP_BGZF_SLOT / 4; i += DEFLATE_THREADS) L.image[i] = 0;
    for (uint32_t i = tid; i < (DEFLATE_THREADS / 64) * DGRP_DEFLATE_NSYM; i += DEFLATE_THREADS) (&L.s.hist[0][0])[i] = 0;
    L.s.crctab[tid] = dgrp_crc_table_entry(tid);
    __syncthreads();
    deflate_hist_crc(src, len, nrun, L.s);

    // ---- 2. the plan
    for (uint32_t s = tid; s < DGRP_DEFLATE_NSYM; s += DEFLATE_THREADS) dgrp_deflate_place(&L.s.plan, (int)s);
    __syncthreads();
    if (tid == 0) dgrp_deflate_plan_member(&L.s.plan, len);
    __syncthreads();
    const uint32_t hdr_end = L.s.plan.hdr_end, deflate_bytes = L.s.plan.deflate_bytes;
    if (tid < 4) L.image[tid] = dgrp_bgzf_head_word((int)tid);
    if (tid < (hdr_end + 31) / 32) L.image[4 + tid] = L.s.plan.hdr[tid];
    __syncthreads();
    deflate_body_literals(src, len, nrun, L.image, L.s);
    deflate_finish(len, deflate_bytes, L.image, L.s, slots + m * DGRP_BGZF_SLOT, sizes + m);
}

// four bytes of the text at any position (text: little-endian words)
__device__ __forceinline__ uint32_t deflate_lz_ld4(const uint32_t *text, uint32_t p)
{
    const uint32_t i = p >> 2;
    const uint64_t w = (uint64_t)text[i] | ((uint64_t)text[i + 1] << 32);
    return (uint32_t)(w >> (8 * (p & 3)));
}

// level 1: as deflate_member_kernel, with lz[m * 0xff00 ...) for the member's word per position
__global__ void __launch_bounds__(DEFLATE_THREADS) deflate_lz_member_kernel(const uint8_t *__restrict__ in, int64_t n,
                                                                            const char *__restrict__ rows, int64_t stride,
                                                                            uint8_t *__restrict__ slots, uint64_t *__restrict__ sizes,
                                                                            uint32_t *lz)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char deflate_smem[];
    deflate_lz_lds &L = *reinterpret_cast<deflate_lz_lds *>(deflate_smem);
    const uint32_t tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    uint32_t len;
    const uint8_t *src = deflate_member_src(in, n, rows, stride, m, len);
    if (len == 0) {                                           // (uniform; a table's empty block: no member, the caller frames it)
        if (tid == 0) sizes[m] = 0;
        return;
    }
    const uint32_t nrun = (len + DEFLATE_RUN - 1) / DEFLATE_RUN, ntile = (len + DEFLATE_LZ_TILE - 1) / DEFLATE_LZ_TILE;
    uint32_t *ws = lz + m * DGRP_BGZF_BLOCK;

    for (uint32_t i = tid; i < (1u << DGRP_LZ_HASH_BITS) / 2; i += DEFLATE_THREADS) reinterpret_cast<uint32_t *>(L.table)[i] = 0xffffffffu;
    for (uint32_t i = tid; i < (DEFLATE_THREADS / 64) * DGRP_DEFLATE_NSYM; i += DEFLATE_THREADS) (&L.s.hist[0][0])[i] = 0;
    for (uint32_t i = tid; i < DGRP_LZ_NSYM; i += DEFLATE_THREADS) L.lz.freq[i] = i == 256;
    L.s.crctab[tid] = dgrp_crc_table_entry(tid);
    for (uint32_t r = tid; r < (DGRP_BGZF_BLOCK + 16) / DEFLATE_RUN; r += DEFLATE_THREADS) {
        const uint32_t at = r * DEFLATE_RUN, k = at < len ? min(len - at, (uint32_t)DEFLATE_RUN) : 0;
        deflate_run v;
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
        if (k) v = deflate_load_run(src + at, k);
#pragma unroll
        for (int j = 0; j < 4; ++j) L.text[at / 4 + j] = v.w[j];
    }
    __syncthreads();
    deflate_hist_crc(src, len, nrun, L.s);

    // ---- a. candidates and lengths
    for (uint32_t t = 0; t < ntile; ++t) {
        const uint32_t p = t * DEFLATE_LZ_TILE + tid;
        const bool keyed = p + 4 <= len;
        uint32_t key = 0xffff0000u | tid, cand = 0xffffu;     // (a position without a key equals nobody)
        if (keyed) {
            key = dgrp_lz_key(deflate_lz_ld4(L.text, p));
            cand = L.table[key];
        }
        L.tkey[tid] = key;
        L.flag[tid] = 0;
        __syncthreads();
        if (keyed) {
            // the nearest earlier position of the tile with this key, four keys a step
            const uint4 *k4 = reinterpret_cast<const uint4 *>(L.tkey);
            for (int c = (int)(tid >> 2); c >= 0; --c) {
                const uint4 q = k4[c];
                const int j0 = 4 * c;
                int hit = -1;
                if (q.x == key && j0 < (int)tid) hit = j0;
                if (q.y == key && j0 + 1 < (int)tid) hit = j0 + 1;
                if (q.z == key && j0 + 2 < (int)tid) hit = j0 + 2;
                if (q.w == key && j0 + 3 < (int)tid) hit = j0 + 3;
                if (hit >= 0) {
                    cand = t * DEFLATE_LZ_TILE + (uint32_t)hit;
                    L.flag[hit] = 1;
                    break;
                }
            }
        }
        __syncthreads();
        if (keyed && !L.flag[tid]) L.table[key] = (uint16_t)p;
        uint32_t e = 0;
        if (cand != 0xffffu && p - cand <= DGRP_LZ_WINDOW) {
            const uint32_t cap = min(len - p, (uint32_t)DGRP_LZ_MAX);
            uint32_t l = 0;
            while (l < cap) {
                const uint32_t x = deflate_lz_ld4(L.text, p + l) ^ deflate_lz_ld4(L.text, cand + l);
                if (x) {
                    l += (uint32_t)__builtin_ctz(x) >> 3;
                    break;
                }
                l += 4;
            }
            e = min(l, cap) | ((p - cand - 1) << 9);
        }
        if (p < len) ws[p] = e;
        __syncthreads();
    }

    // ---- b. the parse and the histograms of its tokens
    uint32_t entry = 0;
    for (uint32_t t = 0; t < ntile; ++t) {
        if (entry >= DEFLATE_LZ_TILE) {                        // a match jumped over the whole tile
            entry -= DEFLATE_LZ_TILE;
            continue;
        }
        const uint32_t p = t * DEFLATE_LZ_TILE + tid;
        const bool valid = p < len;
        const uint32_t e = valid ? ws[p] : 0u;
        const uint32_t out = valid ? tid + dgrp_lz_step(e) : 2u * DEFLATE_LZ_TILE;     // next(p) relative to the tile
        uint32_t jump = out;                                    // next^(2^k)(p), or some position behind the tile
        L.flag[tid] = tid == entry;
        for (;;) {
            L.jump[tid] = (uint16_t)jump;
            const bool reached = L.flag[tid] != 0;
            __syncthreads();
            int added = 0;
            if (reached && jump < DEFLATE_LZ_TILE) {
                added = L.flag[jump] == 0;
                L.flag[jump] = 1;
            }
            if (jump < DEFLATE_LZ_TILE) jump = L.jump[jump];
            if (!__syncthreads_or(added)) break;              // the first 2^k positions of the path are in: none added, all in
        }
        if (L.flag[tid] != 0 && valid) {
            ws[p] = e | DGRP_LZ_TOKEN;
            if (dgrp_lz_len(e) < DGRP_LZ_MIN) {
                atomicAdd(&L.lz.freq[(L.text[p >> 2] >> (8 * (p & 3))) & 0xffu], 1u);
            } else {
                atomicAdd(&L.lz.freq[dgrp_lz_len_sym(dgrp_lz_len(e)) & 0xffffu], 1u);
                atomicAdd(&L.lz.freq[DGRP_LZ_NLIT + (dgrp_lz_dist_sym(dgrp_lz_dist(e)) & 0xffu)], 1u);
            }
            if (out >= DEFLATE_LZ_TILE) L.entry = out - DEFLATE_LZ_TILE;
        }
        __syncthreads();
        entry = L.entry;
    }

    // ---- c. both plans, the smaller block
    for (uint32_t s = tid; s < DGRP_DEFLATE_NSYM; s += DEFLATE_THREADS) dgrp_deflate_place(&L.s.plan, (int)s);
    for (uint32_t s = tid; s < DGRP_LZ_NSYM; s += DEFLATE_THREADS) dgrp_lz_place(&L.lz, (int)s);
    for (uint32_t i = tid; i < DGRP_BGZF_SLOT / 4; i += DEFLATE_THREADS) L.image[i] = 0;      // (the bucket table is done)
    __syncthreads();
    if (tid == 0) dgrp_deflate_plan_member(&L.s.plan, len);
    if (tid == 64) dgrp_lz_plan_member(&L.lz);
    __syncthreads();
    const bool matches = dgrp_lz_wins(&L.lz, &L.s.plan);
    const uint32_t hdr_end = matches ? L.lz.hdr_end : L.s.plan.hdr_end;
    const uint32_t deflate_bytes = matches ? L.lz.deflate_bytes : L.s.plan.deflate_bytes;
    if (tid < 4) L.image[tid] = dgrp_bgzf_head_word((int)tid);
    if (tid < (hdr_end + 31) / 32) L.image[4 + tid] = matches ? L.lz.hdr[tid] : L.s.plan.hdr[tid];
    __syncthreads();

    // ---- d. the body
    if (!matches) {
        deflate_body_literals(src, len, nrun, L.image, L.s);
    } else {
        uint32_t *img = L.image + 4;
        uint64_t carry = hdr_end;
        for (uint32_t base = 0; base < nrun; base += DEFLATE_THREADS) {
            const uint32_t r = base + tid, at = r * DEFLATE_RUN;
            const uint32_t k = r < nrun ? min(len - at, (uint32_t)DEFLATE_RUN) : 0;
            uint32_t ent[DEFLATE_RUN];
            deflate_run v;
            v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j) ent[j] = 0;
            if (k) {
                const uint4 *e4 = reinterpret_cast<const uint4 *>(ws + at);       // (whole: 0xff00 is a multiple of the run)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint4 q = e4[j];
                    ent[4 * j] = q.x, ent[4 * j + 1] = q.y, ent[4 * j + 2] = q.z, ent[4 * j + 3] = q.w;
                    v.w[j] = L.text[at / 4 + j];
                }
            }
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j) {
                if ((uint32_t)j < k && (ent[j] & DGRP_LZ_TOKEN)) {
                    uint32_t lo, nlo, hi, nhi;
                    dgrp_lz_token_bits(L.lz.table, ent[j], v.byte(j), lo, nlo, hi, nhi);
                    bits += nlo + nhi;
                }
            }
            uint64_t total;
            const uint64_t pos = block_exclusive_scan(bits, &total, L.s.scan) + carry;
            carry += total;
            uint32_t w = (uint32_t)(pos >> 5), nb = (uint32_t)pos & 31u;
            uint64_t acc = 0;
            bool shared = true;                               // the run's first word may hold a neighbour's bits as well
#pragma unroll
            for (int j = 0; j < DEFLATE_RUN; ++j) {
                uint32_t lo = 0, nlo = 0, hi = 0, nhi = 0;
                if ((uint32_t)j < k && (ent[j] & DGRP_LZ_TOKEN)) dgrp_lz_token_bits(L.lz.table, ent[j], v.byte(j), lo, nlo, hi, nhi);
#pragma unroll
                for (int half = 0; half < 2; ++half) {        // at most 20 bits, then at most 28: either fits behind nb < 32
                    acc |= (uint64_t)(half ? hi : lo) << nb;
                    nb += half ? nhi : nlo;
                    if (nb >= 32) {
                        if (shared) atomicOr(&img[w], (uint32_t)acc);
                        else img[w] = (uint32_t)acc;
                        shared = false;
                        ++w;
                        acc >>= 32;
                        nb -= 32;
                    }
                }
            }
            if (nb && k) atomicOr(&img[w], (uint32_t)acc);
        }
        if (tid == 0) {
            const uint32_t e = L.lz.table[256], s = (uint32_t)carry & 31u, w = (uint32_t)(carry >> 5);
            const uint64_t acc = (uint64_t)(e & 0xffffu) << s;
            atomicOr(&img[w], (uint32_t)acc);
            if (s + (e >> 16) > 32) atomicOr(&img[w + 1], (uint32_t)(acc >> 32));
        }
        __syncthreads();
    }
    deflate_finish(len, deflate_bytes, L.image, L.s, slots + m * DGRP_BGZF_SLOT, sizes + m);
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

// The member kernel of `level` for nmem members (contiguous blocks of d_in[0, n), or the blocks of a table: deflate_member_src), on the
// stream: slots (nmem * DGRP_BGZF_SLOT bytes, 16-byte aligned), sizes[nmem], lz (level 1: nmem * 0xff00 words).  Also for
// bigwig_kernels.hip, which reframes the members as zlib streams (deflate_blocks.h).
int dgrp_deflate_members(const uint8_t *d_in, int64_t n, const char *d_rows, int64_t stride, int64_t nmem, int level, uint8_t *slots,
                         uint64_t *sizes, uint32_t *lz, hipStream_t stream)
{
    static std::once_flag configured;
    static hipError_t cfg_err = hipSuccess;
    std::call_once(configured, [] {
        cfg_err = hipFuncSetAttribute((const void *)deflate_member_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(deflate_lds));
        if (cfg_err == hipSuccess)
            cfg_err = hipFuncSetAttribute((const void *)deflate_lz_member_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)sizeof(deflate_lz_lds));
    });
    DGRP_HIP(cfg_err);
    if (level == 0) {
        hipLaunchKernelGGL(deflate_member_kernel, dim3((unsigned)nmem), dim3(DEFLATE_THREADS), sizeof(deflate_lds), stream, d_in, n, d_rows,
                           stride, slots, sizes);
    } else {
        hipLaunchKernelGGL(deflate_lz_member_kernel, dim3((unsigned)nmem), dim3(DEFLATE_THREADS), sizeof(deflate_lz_lds), stream, d_in, n,
                           d_rows, stride, slots, sizes, lz);
    }
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}

DGRP_EXPORT int64_t dgrp_bgzf_bound(int64_t n, int eof)
{
    if (n < 0) return 0;
    return n + 31 * bgzf_members(n) + (eof ? DGRP_BGZF_EOF_BYTES : 0);
}

static int64_t bgzf_workspace(int64_t n, int level)
{
    const int64_t nmem = bgzf_members(n);
    const int64_t base = dgrp_align_up(nmem * DGRP_BGZF_SLOT, 256) + dgrp_align_up((nmem + 1) * 8, 256);
    return level == 0 ? base : base + nmem * DGRP_BGZF_BLOCK * (int64_t)sizeof(uint32_t);
}

DGRP_EXPORT int64_t dgrp_bgzf_workspace_bytes(int64_t n) { return n < 0 ? 0 : bgzf_workspace(n, 0); }

DGRP_EXPORT int64_t dgrp_bgzf_workspace_bytes_level(int64_t n, int level)
{
    return n < 0 || level < 0 || level > 1 ? 0 : bgzf_workspace(n, level);
}

static int bgzf_compress_device(const char *who, const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                                int level, void *d_work, int64_t work_bytes, hipStream_t stream)
{
    if (!(n >= 0 && out_cap >= 0 && work_bytes >= 0 && h_out_bytes)) {
        dgrp_set_error("%s: bad arguments", who);
        return DGRP_EINVAL;
    }
    *h_out_bytes = 0;
    const int64_t nmem = bgzf_members(n);
    if (level < 0 || level > 1) {
        dgrp_set_error("%s: level %d (0: literals, 1: matches)", who, level);
        return DGRP_EINVAL;
    }
    if (nmem > INT32_MAX - 1) {
        dgrp_set_error("%s: too many members", who);
        return DGRP_EINVAL;
    }
    if (!(n == 0 || (d_in && d_work)) || !(d_out || (n == 0 && !eof) || out_cap == 0)) {
        dgrp_set_error("%s: NULL pointer", who);
        return DGRP_EINVAL;
    }
    if (n == 0) {
        if (!eof) return DGRP_OK;
        *h_out_bytes = DGRP_BGZF_EOF_BYTES;
        if (out_cap < DGRP_BGZF_EOF_BYTES) {
            dgrp_set_error("%s: output of %lld bytes, the EOF member takes %d", who, (long long)out_cap, DGRP_BGZF_EOF_BYTES);
            return DGRP_ENOMEM;
        }
        DGRP_HIP(hipMemcpyAsync(d_out, BGZF_EOF_MEMBER, DGRP_BGZF_EOF_BYTES, hipMemcpyHostToDevice, stream));
        DGRP_HIP(hipStreamSynchronize(stream));
        return DGRP_OK;
    }
    if (work_bytes < bgzf_workspace(n, level)) {
        dgrp_set_error("%s: workspace too small", who);
        return DGRP_ENOMEM;
    }
    if (((uintptr_t)d_work & 15) != 0) {
        dgrp_set_error("%s: d_work must be 16-byte aligned", who);
        return DGRP_EINVAL;
    }
    uint8_t *slots = (uint8_t *)d_work;
    uint64_t *sizes = (uint64_t *)(slots + dgrp_align_up(nmem * DGRP_BGZF_SLOT, 256));
    uint32_t *lz = level == 0 ? nullptr : (uint32_t *)((uint8_t *)sizes + dgrp_align_up((nmem + 1) * 8, 256));
    const int rc = dgrp_deflate_members(d_in, n, nullptr, 0, nmem, level, slots, sizes, lz, stream);
    if (rc != DGRP_OK) return rc;
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, sizes, nmem, sizes + nmem);
    DGRP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bgzf_place_kernel, dim3((unsigned)(nmem + (eof ? 1 : 0))), dim3(256), 0, stream, slots, sizes, nmem, eof, d_out, out_cap);
    DGRP_LAUNCH_CHECK();
    uint64_t all = 0;
    DGRP_HIP(hipMemcpyAsync(&all, sizes + nmem, 8, hipMemcpyDeviceToHost, stream));
    DGRP_HIP(hipStreamSynchronize(stream));
    *h_out_bytes = (int64_t)all + (eof ? DGRP_BGZF_EOF_BYTES : 0);
    if (*h_out_bytes > out_cap) {
        dgrp_set_error("%s: output of %lld bytes, %lld needed (nothing written)", who, (long long)out_cap, (long long)*h_out_bytes);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}

static int bgzf_compress_host(const char *who, const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                              int level)
{
    if (!(n >= 0 && out_cap >= 0 && h_out_bytes)) {
        dgrp_set_error("%s: bad arguments", who);
        return DGRP_EINVAL;
    }
    *h_out_bytes = 0;
    if (level < 0 || level > 1) {
        dgrp_set_error("%s: level %d (0: literals, 1: matches)", who, level);
        return DGRP_EINVAL;
    }
    if (!(h_in || n == 0) || !(h_out || (n == 0 && !eof) || out_cap == 0)) {
        dgrp_set_error("%s: NULL pointer", who);
        return DGRP_EINVAL;
    }
    std::vector<uint32_t> slot(DGRP_BGZF_SLOT / 4), lz(level ? DGRP_BGZF_BLOCK : 0);
    std::vector<uint16_t> head(level ? 1 << DGRP_LZ_HASH_BITS : 0);
    dgrp_deflate_plan plan;
    dgrp_lz_plan lzplan;
    int64_t pos = 0;
    bool fits = true;                                        // once a member does not fit nothing more is written, only counted
    for (int64_t o = 0; o < n; o += DGRP_BGZF_BLOCK) {
        const uint32_t k = (uint32_t)(n - o < DGRP_BGZF_BLOCK ? n - o : DGRP_BGZF_BLOCK);
        const uint32_t size = level ? dgrp_bgzf_member_serial_lz(h_in + o, k, slot.data(), &plan, &lzplan, lz.data(), head.data())
                                    : dgrp_bgzf_member_serial(h_in + o, k, slot.data(), &plan);
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
        dgrp_set_error("%s: output of %lld bytes, %lld needed", who, (long long)out_cap, (long long)pos);
        return DGRP_ENOMEM;
    }
    return DGRP_OK;
}

DGRP_EXPORT int dgrp_bgzf_compress(const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                                   void *d_work, int64_t work_bytes, void *stream)
{
    return bgzf_compress_device("dgrp_bgzf_compress", d_in, n, d_out, out_cap, h_out_bytes, eof, 0, d_work, work_bytes, (hipStream_t)stream);
}

DGRP_EXPORT int dgrp_bgzf_compress_level(const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                                         int level, void *d_work, int64_t work_bytes, void *stream)
{
    return bgzf_compress_device("dgrp_bgzf_compress_level", d_in, n, d_out, out_cap, h_out_bytes, eof, level, d_work, work_bytes,
                                (hipStream_t)stream);
}

DGRP_EXPORT int dgrp_bgzf_compress_host(const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes, int eof)
{
    return bgzf_compress_host("dgrp_bgzf_compress_host", h_in, n, h_out, out_cap, h_out_bytes, eof, 0);
}

DGRP_EXPORT int dgrp_bgzf_compress_host_level(const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes,
                                              int eof, int level)
{
    return bgzf_compress_host("dgrp_bgzf_compress_host_level", h_in, n, h_out, out_cap, h_out_bytes, eof, level);
}
