"""Synthetic rows and scores for the bigBed tests (not a test): consistent dgrp_row_score arrays (sum <= bases * 2^24, 0 <= agree <=
bases, qmin <= 2^24) without running a model, and a host-side bigbed.BigBedWrite made of the reference statements."""
import numpy as np

ONE = 1 << 24
LABELS = (1, 9, 10, 63)                             # one and two digits: `rest` changes length
# per-base mean in units of 2^-24: scores that print 0, 7, 1000 (mean 1.0000) and ordinary ones
MEANS = (0, int(0.007 * ONE), ONE, int(0.8123 * ONE), int(0.55 * ONE), int(0.9996 * ONE))
LOW = int(0.1 * ONE)                                # score 100: what a min_score of 300 drops


HIGH = MEANS[2:]                                    # means no min_score up to 500 drops


def rows_scores(spans, contigs=None, low=(), means=MEANS):
    """(rows SEGMENT_DTYPE, scores ROW_SCORE_DTYPE) for [(start, end)]; row i gets label LABELS[i % 4] and mean means[i % len(means)],
    or LOW where i is in `low`."""
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE
    n = len(spans)
    rows, scores = np.zeros(n, SEGMENT_DTYPE), np.zeros(n, ROW_SCORE_DTYPE)
    low = {i % n for i in low} if n else set()
    for i, (a, b) in enumerate(spans):
        bases = b - a
        mean = LOW if i in low else means[i % len(means)]
        rows[i] = (a, b, LABELS[i % len(LABELS)], 0 if contigs is None else contigs[i])
        scores[i] = (mean * bases, bases, (bases * (i % 5)) // 4, mean // 2 if i % 3 else mean, 0)
    return rows, scores


def ladder(n, start=5, step=40, width=30):
    """n spans that do not touch."""
    return [(start + step * i, start + step * i + width) for i in range(n)]


def host_write(names, sizes, by_contig, rows, scores, min_score=0, chrom0=0, level=1):
    """The BigBedWrite ContigPipeline.bigbed_write gives for these rows, from bigbed.reference_* and the host zlib entry."""
    from deepgrp_amd import bigbed as bb
    from deepgrp_amd.bigwig import zlib_compress_host
    data, table = bb.reference_blocks(by_contig, rows, scores, min_score, chrom0)
    blob, bsizes = zlib_compress_host(data, table["off"], table["bytes"], level)
    zdata, _roff, ztable, _boff = bb.reference_zoom(by_contig, rows, scores, min_score, chrom0)
    zblob, zsizes = zlib_compress_host(zdata, ztable["off"], ztable["bytes"], level)
    return bb.BigBedWrite(list(names), list(sizes), None, blob, bsizes, table, zblob, zsizes, ztable,
                          bb.reference_totals(by_contig, rows, scores, min_score), chrom0)
