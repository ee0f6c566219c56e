"""Shared by tests/test_gpu_rmout_text.py: dgrp_rmout_text_batch called through ctypes on the guarded device buffers of
bed_device.py (a plain helper, no tests here)."""
import ctypes as C

import numpy as np
import torch

from bed_device import Arena, _upload
from deepgrp_amd import rmout
from deepgrp_amd._lib import lib, name_blob
from deepgrp_amd.pipeline import stream_ptr


def tables(names, pairs):
    """-> (names, blob, offsets, class blob, its offsets: two entries per label)"""
    raw, blob, off = name_blob(names)
    _c, cblob, coff = name_blob([x for pair in pairs for x in pair])
    return raw, blob, off, cblob, coff


def text_call(names, by_contig, rows, scores, min_score, rec_end, pairs, join=-1, id0=0, cap=None, short_work=0, slack=64):
    """-> (return code, *h_bytes, *h_lines, *h_ids, the text arena, the workspace arena); runs on the current stream and waits for
    it.  cap None: the statement's length and `slack` bytes (which must stay untouched)."""
    L = lib()
    raw, blob, off, cblob, coff = tables(names, pairs)
    ends = np.ascontiguousarray(rec_end, np.int64)
    n = len(rows)
    if cap is None:
        cap = len(rmout.reference_lines(names, by_contig, rows, scores, min_score, rec_end, pairs, join, id0)[0]) + slack
    wb = int(L.dgrp_rmout_text_workspace_bytes(n, len(raw), len(blob), len(pairs), len(cblob), len(ends)))
    assert wb > 0
    text, work = Arena(cap), Arena(wb - short_work)
    keep_r, p_rows = _upload(rows)
    keep_s, p_scores = _upload(scores)
    got, lines, ids = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    rc = L.dgrp_rmout_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, coff.ctypes.data, len(pairs), p_rows, p_scores, n,
                                 int(min_score), len(ends), ends.ctypes.data, int(join), int(id0), text.ptr, cap, C.byref(got),
                                 C.byref(lines), C.byref(ids), work.ptr, work.n, stream_ptr())
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, lines.value, ids.value, text, work
