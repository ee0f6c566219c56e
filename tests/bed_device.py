"""Shared by tests/test_gpu_bed_text.py and tests/test_gpu_bed_index.py: dgrp_bed_text_batch and dgrp_bed_index_batch called through
ctypes on guarded device buffers (a sentinel page in front of and behind the text, the chunks, the linear index and the workspace),
and the builders of synthetic rows and scores."""
import ctypes as C

import numpy as np
import torch

from deepgrp_amd._lib import lib, name_blob
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE, stream_ptr
from deepgrp_amd.tabix import CHUNK_DTYPE, MIN_SHIFT

ONE = 1 << 24
EINVAL, ENOMEM = -1, -3
GUARD, FILL = 4096, 0xA5


class Arena:
    """`nbytes` of device memory between two sentinel pages."""

    def __init__(self, nbytes: int):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD

    def body(self, n=None):
        return self.t[GUARD:GUARD + (self.n if n is None else n)]

    def guards_intact(self) -> bool:
        return bool((self.t[:GUARD] == FILL).all()) and bool((self.t[GUARD + self.n:] == FILL).all())

    def untouched(self) -> bool:
        return bool((self.t == FILL).all())


def segs(rows):
    """(start, end, label, contig) tuples -> SEGMENT_DTYPE"""
    a = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def scores_of(rows):
    """(sum, bases, agree, qmin) tuples -> ROW_SCORE_DTYPE"""
    a = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for i, (s, b, g, m) in enumerate(rows):
        a[i] = (s, b, g, m, 0)
    return a


def random_scores(n, rng, filtered=0.0):
    """Consistent random scores (sum <= bases * 2^24, agree <= bases); a share `filtered` of them with sum 0 (score 0)."""
    sc = np.zeros(n, ROW_SCORE_DTYPE)
    sc["bases"] = rng.integers(1, 1 << 20, n)
    sc["qmin"] = rng.integers(0, ONE + 1, n)
    sc["sum"] = [int(b) * int(rng.integers(int(m), ONE + 1)) for b, m in zip(sc["bases"], sc["qmin"])]
    sc["agree"] = [int(rng.integers(0, int(b) + 1)) for b in sc["bases"]]
    sc["sum"][rng.random(n) < filtered] = 0
    return sc


def _upload(a):
    if len(a) == 0:
        return None, None
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    return t, t.data_ptr()


def text_call(names, by_contig, rows, scores, min_score=0, cap=None, short_work=0):
    """-> (return code, *h_bytes, the text arena, the workspace arena); runs on the current stream and waits for it."""
    L = lib()
    raw, blob, off = name_blob(names)
    n = len(rows)
    if cap is None:
        cap = int(L.dgrp_format_bed_bound(n, max(len(x) for x in raw)))
    wb = int(L.dgrp_bed_text_workspace_bytes(n, len(raw), len(blob)))
    assert wb > 0
    text, work = Arena(cap), Arena(wb - short_work)
    keep_r, p_rows = _upload(rows)
    keep_s, p_scores = _upload(scores)
    got = C.c_int64(-7)
    rc = L.dgrp_bed_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), p_rows, p_scores, n, int(min_score), text.ptr, cap,
                               C.byref(got), work.ptr, work.n, stream_ptr())
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, text, work


def window_prefix(rec_end):
    wpref = np.zeros(len(rec_end) + 1, np.int64)
    np.cumsum([((int(e) - 1) >> MIN_SHIFT) + 1 for e in rec_end], out=wpref[1:])
    return wpref


def index_call(names, by_contig, rows, scores, min_score, rec_end, chunk_cap=None, short_work=0):
    """-> (return code, *h_nchunks, arenas of chunks, linear index, last ends and workspace, wpref)"""
    L = lib()
    raw, blob, off = name_blob(names)
    n, nrec = len(rows), len(rec_end)
    ends = np.ascontiguousarray(rec_end, np.int64)
    wpref = window_prefix([min(max(int(e), 1), 1 << 29) for e in rec_end])
    nwin = int(wpref[-1])
    if chunk_cap is None:
        chunk_cap = max(n, 1)
    wb = int(L.dgrp_bed_index_workspace_bytes(n, len(raw), len(blob), nrec))
    assert wb > 0
    chunks, linear, last, work = Arena(chunk_cap * CHUNK_DTYPE.itemsize), Arena(nwin * 8), Arena(nrec * 8), Arena(wb - short_work)
    keep_r, p_rows = _upload(rows)
    keep_s, p_scores = _upload(scores)
    got = C.c_int64(-7)
    rc = L.dgrp_bed_index_batch(blob, off.ctypes.data, len(raw), int(by_contig), p_rows, p_scores, n, int(min_score), nrec, ends.ctypes.data,
                                chunks.ptr, chunk_cap, C.byref(got), linear.ptr, nwin, last.ptr, work.ptr, work.n, stream_ptr())
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, chunks, linear, last, work, wpref


def index_parts(chunks: Arena, nchunks: int, linear: Arena, last: Arena):
    """The arenas' contents as bed.reference_index_parts lays them out."""
    c = chunks.body(nchunks * CHUNK_DTYPE.itemsize).cpu().numpy().view(CHUNK_DTYPE)
    return c, linear.body().cpu().numpy().view(np.int64), last.body().cpu().numpy().view(np.int64)
