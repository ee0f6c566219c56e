// What every entry that walks rows over flat per-base buffers starts with: `evaluate` (eval_kernels.hip) and its strata
// (strata_kernels.hip).  eval_prepare and eval_spans are defined once, in eval_kernels.hip (hidden symbols of the library).
#pragma once
#include "eval_paint.h"
#include "bed_rows.h"
#include "scan.h"
#include <vector>

struct eval_plan {
    std::vector<int64_t> tab;          // off[nrec], len[nrec], origin[nrec], row_off[nrec + 1]
    int64_t nrows = 0;
    int64_t *d_off = nullptr, *d_len, *d_origin, *d_row_off, *d_dst;
    uint64_t *d_cl = nullptr, *d_tiles = nullptr;
    char *d_extra = nullptr;           // `extra_bytes` behind the tables, for the caller
    unsigned long long tot[128];       // clipped length per label
};

// argument checks, tables to the device, the row check (one synchronisation): DGRP_EINVAL on a bad row before anything is written.
// d_scores: the rows are scored rows, checked as eval_check_kernel says; extra_bytes: more workspace, 256-byte aligned, at pl.d_extra;
// d_row_key: the rows carry keys of their own (dgrp_paint_keys_batch) -- the label is not read, a key must lie below 0xFFFFFFFF, and
// every clipped length is summed into pl.tot[1]
int eval_prepare(const char *what, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                 const dgrp_segment *d_rows, const int64_t *h_row_off, void *d_work, int64_t work_bytes, hipStream_t stream,
                 eval_plan &pl, int max_label = 127, const dgrp_row_score *d_scores = nullptr, int64_t extra_bytes = 0,
                 const uint32_t *d_row_key = nullptr);

// the pass's clipped lengths and first positions, scanned: d_cl[0..nrows] = exclusive scan, d_cl[nrows] = the pass's total
int eval_spans(const eval_plan &pl, const dgrp_segment *d_rows, int64_t nrec, int label, hipStream_t stream);
