"""Scored BED of the predicted repeats (`predict --bed_dir`): for every input file one `DIR/<basename>.bed` with a line per TSV row,

    name<TAB>start<TAB>end<TAB>class<label><TAB>score<TAB>.<TAB>mean<TAB>min<TAB>agree<LF>

name is the record's name (evaluation.record_name, the first word of the header, as the tracks use it), start and end the TSV's
coordinates.  The figures say how sure the model is of the element, from the merged probabilities of the row's own class over the
row's bases (ContigPipeline.merged, the array the labels are computed from): `mean` and `min` are the mean and the smallest of them,
`agree` the fraction of the bases at which that class is the largest column, `score` the mean on BED's 0..1000 scale.

Everything is exact integer arithmetic.  A probability p becomes q(p) = round-half-up(p * 2^24) clamped to [0, 2^24] (0 for a NaN);
the device sums, minimises and counts per row (dgrp_row_scores_batch, ROW_SCORE_DTYPE), the host formatter (dgrp_format_bed_rows)
rounds the quotients half up.  `reference_scores` and `reference_lines` restate both in numpy and Python integers."""
from __future__ import annotations

import ctypes as C
import os
import sys
import tempfile
from typing import NamedTuple, Optional, Sequence

import numpy as np

ONE = 1 << 24                                       # q(1.0): the fixed-point unit


class BedPlan(NamedTuple):
    directory: str
    min_score: int
    paths: dict                                     # input file -> its BED file


def bed_path(directory: str, filename: str) -> str:
    from .tracks import input_basename
    return os.path.join(directory, input_basename(filename) + ".bed")


def refuse_on_evaluate(args) -> None:
    if getattr(args, "bed_dir", None) is not None or getattr(args, "bed_min_score", None) is not None:
        sys.exit("--bed_dir belongs to predict, not evaluate")


def plan(args) -> Optional[BedPlan]:
    """--bed_dir and --bed_min_score, or None without the flag.  Every refusal is made here (sys.exit), before the model is read or
    the GPU is touched."""
    bdir = getattr(args, "bed_dir", None)
    low = getattr(args, "bed_min_score", None)
    if bdir is None:
        if low is not None:
            sys.exit("--bed_min_score needs --bed_dir")
        return None
    low = 0 if low is None else low
    if not 0 <= low <= 1000:
        sys.exit(f"--bed_min_score must lie in 0..1000, not {low}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or getattr(args, "split_contigs", False):
        sys.exit("--bed_dir runs in one process (WORLD_SIZE > 1 and --split_contigs are not supported: the scores are summed on the "
                 "rank that holds the merged probabilities)")
    paths, seen = {}, {}
    for f in args.FASTA:
        out = bed_path(bdir, f)
        base = os.path.basename(out)
        if base in seen and os.path.realpath(seen[base]) != os.path.realpath(f):
            sys.exit(f"--bed_dir: the BED files of {seen[base]} and {f} have the same file name {base}; they would collide")
        seen[base] = f
        if f != "-" and os.path.exists(f) and os.path.realpath(out) == os.path.realpath(f):
            sys.exit(f"--bed_dir: the BED file {out} would overwrite the input {f}")
        paths[f] = out
    if len(paths) != len(args.FASTA):
        sys.exit("--bed_dir: an input file is given twice")
    return BedPlan(bdir, int(low), paths)


class BedFiles:
    """The BED file of one input: written to a temporary file next to it, renamed by `commit`, removed by `abort`."""

    def __init__(self, p: BedPlan, filename: str):
        os.makedirs(p.directory, exist_ok=True)
        self.final = p.paths[filename]
        self.min_score = p.min_score
        fd, self.tmp = tempfile.mkstemp(prefix="." + os.path.basename(self.final) + ".", suffix=".tmp", dir=p.directory)
        self.fh = os.fdopen(fd, "wb")

    def write(self, names: Sequence, by_contig: bool, rows, scores) -> None:
        """The lines of one record (by_contig false: names[0]) or of a batch (rows["contig"] indexes the names)."""
        if len(rows):
            self.fh.write(format_rows(names, by_contig, rows, scores, self.min_score))

    def commit(self) -> None:
        self.fh.close()
        os.replace(self.tmp, self.final)
        self.tmp = None

    def abort(self) -> None:
        self.fh.close()
        if self.tmp is not None and os.path.exists(self.tmp):
            os.remove(self.tmp)
        self.tmp = None


def format_rows(names: Sequence, by_contig: bool, rows, scores, min_score: int = 0) -> bytes:
    """dgrp_format_bed_rows (host code of the library): the BED lines of `rows` (SEGMENT_DTYPE) with `scores` (ROW_SCORE_DTYPE)."""
    from ._lib import check, lib, name_blob
    from .pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE
    L = lib()
    rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
    scores = np.ascontiguousarray(scores, dtype=ROW_SCORE_DTYPE)
    if len(rows) != len(scores):
        raise ValueError(f"{len(rows)} rows but {len(scores)} scores")
    raw, blob, off = name_blob(names)
    cap = int(L.dgrp_format_bed_bound(len(rows), max(len(x) for x in raw)))
    out = np.empty(cap, np.uint8)
    written = C.c_int64()
    check(L.dgrp_format_bed_rows(blob, off.ctypes.data, len(raw), int(by_contig), rows.ctypes.data, scores.ctypes.data, len(rows),
                                 int(min_score), out.ctypes.data, cap, C.byref(written)), "dgrp_format_bed_rows")
    return out[:written.value].tobytes()


# ---- the statements the kernels and the formatter are tested against ------------------------------------------------------------
def quantise(p: np.ndarray) -> np.ndarray:
    """q(p) of float32 values: 0 where !(p > 0), 2^24 where p * 2^24 >= 2^24, else floor(p * 2^24 + 0.5), in float64."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = p.astype(np.float64) * float(ONE)
        inside = (p > 0) & (x < float(ONE))
        q = np.floor(np.where(inside, x, 0.0) + 0.5).astype(np.uint32)
        q[(p > 0) & (x >= float(ONE))] = ONE
    return q


def first_max(probs: np.ndarray) -> np.ndarray:
    """best = 0; for c in 1 .. C-1: if P[i, c] > P[i, best]: best = c -- column by column, on raw floats (a NaN never wins)."""
    probs = np.asarray(probs, np.float32)
    best = np.zeros(len(probs), np.int64)
    vbest = probs[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, probs.shape[1]):
            win = probs[:, c] > vbest
            best[win] = c
            vbest[win] = probs[win, c]
    return best


def reference_scores(probs: np.ndarray, startpos: int, rows) -> np.ndarray:
    """ROW_SCORE_DTYPE per row of ONE record in plain numpy: `probs` float32 [n, C], its row i at coordinate startpos + i; `rows`
    SEGMENT_DTYPE in original coordinates, clipped to [startpos, startpos + n)."""
    from .pipeline import ROW_SCORE_DTYPE
    probs = np.asarray(probs, np.float32)
    n = len(probs)
    best = first_max(probs) if n else np.zeros(0, np.int64)
    out = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for k, row in enumerate(rows):
        a = min(max(int(row["start"]) - startpos, 0), n)
        b = min(max(int(row["end"]) - startpos, 0), n)
        if b <= a:
            continue
        lab = int(row["label"])
        q = quantise(probs[a:b, lab])
        out[k] = (int(q.astype(np.uint64).sum()), b - a, int((best[a:b] == lab).sum()), int(q.min()), 0)
    return out


def _half_up(num: int, den: int, k: int) -> int:
    return (2 * k * num + den) // (2 * den)


def reference_lines(names: Sequence, by_contig: bool, rows, scores, min_score: int = 0) -> bytes:
    """The BED lines in Python integers: the format's statement."""
    raw = [nm if isinstance(nm, bytes) else nm.encode("utf-8", "surrogateescape") for nm in names]
    out = []
    for row, sc in zip(rows, scores):
        total, bases, agree, qmin = int(sc["sum"]), int(sc["bases"]), int(sc["agree"]), int(sc["qmin"])
        if bases <= 0:
            raise ValueError("a row without a scored base")
        score = _half_up(total, bases << 24, 1000)
        if score < min_score:
            continue
        figs = (_half_up(total, bases << 24, 10000), _half_up(qmin, ONE, 10000), _half_up(agree, bases, 10000))
        name = raw[int(row["contig"]) if by_contig else 0]
        out.append(name + b"\t%d\t%d\tclass%d\t%d\t." % (int(row["start"]), int(row["end"]), int(row["label"]), score)
                   + b"".join(b"\t%d.%04d" % divmod(f, 10000) for f in figs) + b"\n")
    return b"".join(out)
