// The device deflate of a table of blocks, shared by deflate_kernels.hip (BGZF members, where it is defined) and bigwig_kernels.hip
// (zlib streams of the same blocks): one copy of the member kernels in the library.
#pragma once
#include "dgrp_common.h"

int dgrp_deflate_members(const uint8_t *d_in, int64_t n, const char *d_rows, int64_t stride, int64_t nmem, int level, uint8_t *slots,
                         uint64_t *sizes, uint32_t *lz, hipStream_t stream);
