// CRC-32 of the gzip trailer, written once for the host and the device, for the decoder (inflate.h) and the encoder (deflate.h).
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define DGRP_HD __host__ __device__
#else
#define DGRP_HD
#endif

// ---- CRC-32 (ISO-HDLC, the gzip trailer's): reflected polynomial 0xedb88320.  Byte-table update, and the combination of the CRCs
// of two adjacent pieces (crc(A B) from crc(A), crc(B), |B|) by multiplication with x^(8|B|) modulo the polynomial.
DGRP_HD static constexpr uint32_t dgrp_crc_table_entry(uint32_t n)
{
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
    return c;
}
// a * b modulo the polynomial (bit 31 = x^0)
DGRP_HD static constexpr uint32_t dgrp_crc_multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
// x^(8 n) modulo the polynomial
DGRP_HD static constexpr uint32_t dgrp_crc_x8n(uint64_t n)
{
    uint32_t p = 0x80000000u, q = 0x00800000u;   // x^0, x^8
    while (n) {
        if (n & 1) p = dgrp_crc_multmodp(q, p);
        q = dgrp_crc_multmodp(q, q);
        n >>= 1;
    }
    return p;
}
DGRP_HD static constexpr uint32_t dgrp_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return dgrp_crc_multmodp(dgrp_crc_x8n(len_b), crc_a) ^ crc_b;
}

#if defined(__HIP__) || defined(__HIPCC__)
// One wave of 64 lanes: the CRC-32 of the bytes that the lanes' slices [a, b) make up in lane order (they are adjacent; a slice may
// be empty).  tab = 256 words of LDS, filled here; the barrier behind the fill also makes the wave's own earlier stores to the
// bytes visible to every lane.
__device__ static inline uint32_t dgrp_crc_wave(const uint8_t *a, const uint8_t *b, uint32_t *tab)
{
    for (uint32_t i = threadIdx.x; i < 256; i += 64) tab[i] = dgrp_crc_table_entry(i);
    __syncthreads();
    uint32_t c = 0xffffffffu;
    for (const uint8_t *p = a; p < b; ++p) c = tab[(c ^ *p) & 0xff] ^ (c >> 8);
    c ^= 0xffffffffu;
    const uint32_t px = dgrp_crc_x8n((uint64_t)(b - a));
    uint32_t crc = __shfl(c, 0);
    for (int i = 1; i < 64; ++i) crc = dgrp_crc_multmodp(__shfl(px, i), crc) ^ __shfl(c, i);
    return crc;
}
#endif
