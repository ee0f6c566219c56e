"""Shared by tests/test_gpu_gff_text.py and tests/test_gpu_gff_index.py: dgrp_gff_text_batch and dgrp_gff_index_batch called through
ctypes on the guarded device buffers of bed_device.py.  Names and class names are given as they come and escaped here, as
ContigPipeline does it: the device copies them verbatim."""
import ctypes as C

import torch

from bed_device import Arena, _upload, window_prefix
from deepgrp_amd import gff
from deepgrp_amd._lib import lib, name_blob
from deepgrp_amd.pipeline import stream_ptr
from deepgrp_amd.tabix import CHUNK_DTYPE


def tables(names, class_names):
    """-> (escaped names, blob, offsets, class blob or None, its offsets or None, class-name count)"""
    raw, blob, off = name_blob([gff.escape_seqid(nm) for nm in names])
    if not class_names:
        return raw, blob, off, None, None, 0
    _c, cblob, coff = name_blob([gff.escape_value(nm) for nm in class_names])
    return raw, blob, off, cblob, coff, len(class_names)


def bound(names, by_contig, rows, scores, min_score, class_names, id0):
    """The exact length of the text (the statement's): what a caller that knew it would allocate."""
    return len(gff.reference_lines(names, by_contig, rows, scores, min_score, class_names, id0)[0])


def text_call(names, by_contig, rows, scores, min_score=0, class_names=None, id0=0, cap=None, short_work=0, slack=64):
    """-> (return code, *h_bytes, *h_lines, the text arena, the workspace arena); runs on the current stream and waits for it.
    cap None: the statement's length and `slack` bytes (which must stay untouched)."""
    L = lib()
    raw, blob, off, cblob, coff, nc = tables(names, class_names)
    n = len(rows)
    if cap is None:
        cap = bound(names, by_contig, rows, scores, min_score, class_names, id0) + slack
    wb = int(L.dgrp_gff_text_workspace_bytes(n, len(raw), len(blob), nc, len(cblob or b"")))
    assert wb > 0
    text, work = Arena(cap), Arena(wb - short_work)
    keep_r, p_rows = _upload(rows)
    keep_s, p_scores = _upload(scores)
    got, lines = C.c_int64(-7), C.c_int64(-7)
    rc = L.dgrp_gff_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, None if coff is None else coff.ctypes.data, nc,
                               p_rows, p_scores, n, int(min_score), int(id0), text.ptr, cap, C.byref(got), C.byref(lines), work.ptr,
                               work.n, stream_ptr())
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, lines.value, text, work


def index_call(names, by_contig, rows, scores, min_score, rec_end, class_names=None, id0=0, chunk_cap=None, short_work=0):
    """-> (return code, *h_nchunks, arenas of chunks, linear index, last ends and workspace, wpref)"""
    import numpy as np
    L = lib()
    raw, blob, off, cblob, coff, nc = tables(names, class_names)
    n, nrec = len(rows), len(rec_end)
    ends = np.ascontiguousarray(rec_end, np.int64)
    wpref = window_prefix([min(max(int(e), 1), 1 << 29) for e in rec_end])
    nwin = int(wpref[-1])
    if chunk_cap is None:
        chunk_cap = max(n, 1)
    wb = int(L.dgrp_gff_index_workspace_bytes(n, len(raw), len(blob), nc, len(cblob or b""), nrec))
    assert wb > 0
    chunks, linear, last, work = Arena(chunk_cap * CHUNK_DTYPE.itemsize), Arena(nwin * 8), Arena(nrec * 8), Arena(wb - short_work)
    keep_r, p_rows = _upload(rows)
    keep_s, p_scores = _upload(scores)
    got = C.c_int64(-7)
    rc = L.dgrp_gff_index_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, None if coff is None else coff.ctypes.data, nc,
                                p_rows, p_scores, n, int(min_score), int(id0), nrec, ends.ctypes.data, chunks.ptr, chunk_cap,
                                C.byref(got), linear.ptr, nwin, last.ptr, work.ptr, work.n, stream_ptr())
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, chunks, linear, last, work, wpref
