"""Shared by the CSI index tests (tests/test_csi_host.py, tests/test_gpu_csi_index.py, tests/test_gpu_csi_cli.py): hand-written
spans with the bins they must get at depth 6 and depth 5, a corpus of scored BED rows whose coordinates reach 2^32 (rows, scores,
record ends; the large numbers are coordinates, never sizes), its split into two writes, and restatements in Python integers of what
the device entries hand out at a depth."""
import numpy as np

from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE

ONE = 1 << 24
T26, T29, T31, T32 = 1 << 26, 1 << 29, 1 << 31, 1 << 32
FIRST6 = (0, 1, 9, 73, 585, 4681, 37449)            # the first bin of levels 0..6 at depth 6
FIRST5 = (0, 1, 9, 73, 585, 4681)
NBINS6 = 299_593
MIN_SCORE = 500

# (beg, end, bin at depth 6, bin at depth 5 or None where a .tbi cannot hold the span)
SPANS = [
    (0, 1, 37449, 4681),                                          # inside one 16 kb window, at offset 0
    (100, 200, 37449, 4681),
    (T29 - 1, T29, 37449 + 32767, 4681 + 32767),                  # the last window of a .tbi
    (T29, T29 + 1, 37449 + 32768, None),                          # the first window behind it
    (T31 - 1, T31, 37449 + 131071, None),
    (T31, T31 + 1, 37449 + 131072, None),
    (T32 - 1, T32, 299592, None),                                 # the last bin there is
    (T32 - 100, T32, 299592, None),                               # end == 2^32
    (T29 - 5, T29 + 5, 0, None),                                  # across 2^29: the two halves of level 1 at depth 6
    (T31 - 1, T31 + 1, 0, None),
    (0, T32, 0, None),
    (T26 - 5, T26 + 5, 1, 0),                                     # across 2^26 inside [0, 2^29): level 1 at depth 6, the root at depth 5
    (16_383, 16_385, 4681, 585),                                  # across a window edge: one level up
    (3 << 17, (3 << 17) + 1, 37449 + 24, 4681 + 24),
    ((3 << 20) - 1, (3 << 20) + 1, 73 + 0, 9 + 0),                # across 2^20 * 3 inside the first 2^23
    ((5 << 23) - 1, (5 << 23) + 1, 9 + 0, 1 + 0),                 # across a 2^23 edge inside the first 2^26
]
REFUSED_SPAN = (T32 - 100, T32 + 1)                               # end == 2^32 + 1


def corpus():
    """-> names, rows (SEGMENT_DTYPE), scores (ROW_SCORE_DTYPE), rec_end.  Record 0 reaches 2^32: filtered rows at its head and
    inside a run, a line across 2^29 and 2^31 with rows nested in it whose ends descend, one window on each side of 2^29 and 2^31,
    the last window, end == 2^32; 1: only a filtered row; 2: no row (two records without a line between records with lines); 3 and
    4: consecutive records of one name, a filtered row at the end of a run; 5: a short tail record."""
    spans = [(3, 9, True), (10, 20, True)]                                            # filtered rows that would start the first run
    spans += [(30, 40, False), (50, 60, True), (70, 80, False)]                       # a filtered row inside a run of one bin
    spans += [(1000, 3_000_000_000, False)]                                           # bin 0: 183 106 windows; what follows is nested
    spans += [(2000, 2_000_000_000, False), (3000, 1_000_000_000, False), (4000, 5000, False)]     # ... and their ends descend
    spans += [(T26 - 5, T26 + 5, False), (T29 - 1, T29, False), (T29 - 1, T29 + 5, False), (T29, T29 + 1, False)]
    spans += [(T31 - 1, T31, False), (T31 - 1, T31 + 1, False), (T31, T31 + 1, False), (T31 + 1, T31 + 2, True)]
    spans += [(3_000_000_000 - 1, 3_000_000_000 + 20_000, False)]                     # the first line behind the long one
    spans += [(T32 - 16_384, T32 - 1, False), (T32 - 100, T32, False), (T32 - 1, T32, False), (T32 - 1, T32, True)]
    assert spans == sorted(spans, key=lambda t: t[0])
    rows = [(a, b, 1 + i % 4, 0) for i, (a, b, _f) in enumerate(spans)]
    filt = [f for _a, _b, f in spans]
    rows += [(100, 200, 2, 1)]                                                        # record 1: its only row is filtered
    filt += [True]
    rows += [(0, 16_384, 1, 3), (16_383, 16_385, 2, 3), (T29 + 10, T29 + 139_000, 3, 3), (T29 + 20, T29 + 30, 3, 3)]   # "twin"
    filt += [False, False, False, True]                                               # (the last would end the record's last run)
    rows += [(5, 20_000, 1, 4), (6, 8, 2, 4), (T31, T31 + 5, 3, 4)]                   # "twin" again: its first line is long
    filt += [False, False, False]
    rows += [(7, 9, 1, 5)]
    filt += [False]
    seg, sc = _rows_and_scores(rows, filt)
    names = [b"chrBig", b"quiet", b"norows", b"twin", b"twin", b"tail"]
    return names, seg, sc, [T32, 1000, 5000, T29 + 140_000, T31 + 5, 16_384]


def _rows_and_scores(rows, filt):
    seg = np.zeros(len(rows), SEGMENT_DTYPE)
    sc = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for i, (r, f) in enumerate(zip(rows, filt)):
        seg[i] = r
        bases = 1 + 37 * i
        sc[i] = (0 if f else bases * (ONE // 2 + ONE // 8 + 1000 * i), bases, bases // 2, 0, 0)
    return seg, sc


def tbi_corpus():
    """-> names, rows, scores, rec_end inside 2^29, for the equality of the entries at depth 5: rows in and across a bin boundary of
    every level of a `.tbi`, a line over 1 832 windows with rows nested in it, a row ending at 2^29, filtered rows at the head of a
    record and inside a run, records without a line, consecutive records of one name."""
    spans = [(3, 9, True), (10, 20, True), (30, 40, False), (50, 60, True), (70, 80, False), (1000, 1000 + 30_000_000, False)]
    for shift in (14, 17, 20, 23, 26):
        edge = 3 << shift
        spans += [(edge - 50, edge - 40, False), (edge - 5, edge + 5, False), (edge + 7, edge + 19, False), (edge + 19, edge + 30, True)]
    spans += [(40_000_000, 40_000_100, False), (T29 - 16_384, T29 - 1, False), (T29 - 100, T29, False)]
    spans.sort(key=lambda t: t[0])
    rows = [(a, b, 1 + i % 5, 0) for i, (a, b, _f) in enumerate(spans)]
    filt = [f for _a, _b, f in spans]
    rows += [(100, 200, 2, 1), (0, 16_384, 1, 3), (16_383, 16_385, 2, 3), (16_385, 140_000, 3, 3), (5, 20_000, 1, 4), (6, 8, 2, 4),
             (150_000, 150_001, 3, 4), (7, 9, 1, 5)]
    filt += [True] + [False] * 7
    seg, sc = _rows_and_scores(rows, filt)
    return [b"chrA", b"quiet", b"norows", b"twin", b"twin", b"tail"], seg, sc, [T29, 1000, 5000, 140_000, 150_001, 16_384]


def writes(names, rows, scores, rec_end, cut=4):
    """The corpus as two writes, records [0, cut) and [cut, ...): the name "twin" goes on in the second one."""
    out = []
    for a, b in ((0, cut), (cut, len(names))):
        m = (rows["contig"] >= a) & (rows["contig"] < b)
        r = rows[m].copy()
        r["contig"] -= a
        out.append((names[a:b], r, scores[m], rec_end[a:b]))
    return out


def track_like(rec_texts, depth):
    """tabix_corpus.device_like at a depth: what dgrp_track_csi_batch gives for one class of a write whose records have the bedGraph
    texts `rec_texts` -> (chunks [[beg, end, rec, bin]], linear: one list per record up to its last line)."""
    from deepgrp_amd.tabix import csi_reg2bin
    chunks, linear, u = [], [], 0
    for r, t in enumerate(rec_texts):
        lin, prev = [], None
        for line in t.split(b"\n")[:-1]:
            f = line.split(b"\t")
            s, e = int(f[1]), int(f[2])
            b = csi_reg2bin(s, e, depth)
            if prev == b:
                chunks[-1][1] = u + len(line) + 1
            else:
                chunks.append([u, u + len(line) + 1, r, b])
            prev = b
            lin += [u] * (((e - 1) >> 14) + 1 - len(lin))
            u += len(line) + 1
        linear.append(lin)
    return chunks, linear


def scan(lines, name, beg, end, cols=(0, 1, 2), one_based=False):
    """The brute-force overlap filter over split lines (lists of fields)."""
    return [b"\t".join(f) for f in lines
            if f[cols[0]] == name and int(f[cols[1]]) - (1 if one_based else 0) < end and int(f[cols[2]]) > beg]
