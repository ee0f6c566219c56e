"""Per-class probability tracks (`predict --track_dir`): for every input file and selected class, a bedGraph file of the merged class
probabilities the model computes for each base (ContigPipeline.merged), as text built on the GPU (dgrp_track_text).

A line is `name<TAB>start<TAB>end<TAB>value<LF>`: the record's name (evaluation.record_name, raw header bytes), a 0-based half-open
span in the TSV's coordinates, and the maximum probability of the class over the span's bins at `digits` decimals.  Bin k is
[k * bin, (k + 1) * bin) of the record's coordinates, clipped to the predicted span [startpos, startpos + n); consecutive bins of
equal value are one line, and spans of value 0 are left out.  `reference_text` restates the format in numpy.

Short records run as batches (ContigPipeline.run_batch_tracked: dgrp_predict_batch_probs, then dgrp_track_text_batch for all records
and classes of the batch); the text of a batch is the records' texts one after the other.

With `--track_gzip` the files are `<basename>.class<c>.bedGraph.gz`, BGZF as bgzip writes it: the text of a record (of a batch: of one
class of all its records) is deflated on the device where it was written (gz.bgzf_compress_device, --gzip_level, 1 unless given) and
only the members are read back and appended; a record or batch boundary is a short member, and the EOF member is written once, when
the file is committed."""
from __future__ import annotations

import os
import sys
import tempfile
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np


class TrackSpec(NamedTuple):
    """What to write per record: the classes (one file each), decimals of the values, bin width in bases."""
    classes: Tuple[int, ...]
    digits: int = 2
    bin: int = 1
    gzip_level: Optional[int] = None                # None: plain text; else BGZF members at this level


class TrackPlan(NamedTuple):
    directory: str
    classes: Optional[Tuple[int, ...]]              # None: every repeat class 1..C-1 (resolved by `resolve`)
    digits: int
    bin: int
    bases: dict                                     # input file -> basename of its track files
    gzip_level: Optional[int] = None                # --track_gzip: the level (None: plain bedGraph)


def input_basename(filename: str) -> str:
    return "stdin" if filename == "-" else os.path.basename(filename)


def track_path(directory: str, base: str, cls: int, gzip: bool = False) -> str:
    return os.path.join(directory, f"{base}.class{cls}.bedGraph" + (".gz" if gzip else ""))


GZIP_PIECE = 4096 * 0xff00                          # bytes deflated per call (the level-1 workspace is five times the piece)


def gzip_level(args, default: int) -> Optional[int]:
    """--gzip_level checked (sys.exit outside {0, 1}), or `default` without the flag."""
    from .gz import LEVELS
    level = getattr(args, "gzip_level", None)
    if level is None:
        return default
    if level not in LEVELS:
        sys.exit(f"--gzip_level must be 0 (literals only) or 1 (with matches), not {level}")
    return level


def check_gzip_flags(args) -> None:
    """The refusals of --track_gzip and --gzip_level that need nothing but the flags (sys.exit)."""
    if getattr(args, "track_gzip", False) and getattr(args, "track_dir", None) is None:
        sys.exit("--track_gzip needs --track_dir")
    if getattr(args, "gzip_level", None) is not None:
        if not (getattr(args, "mask_gzip", False) or getattr(args, "track_gzip", False)):
            sys.exit("--gzip_level needs --mask_gzip or --track_gzip")
        gzip_level(args, 0)


def plan(args) -> Optional[TrackPlan]:
    """--track_dir and its options, or None without the flag.  Everything that can be refused without the model is refused here
    (sys.exit), before any device work."""
    check_gzip_flags(args)
    tdir = getattr(args, "track_dir", None)
    classes, digits, width = (getattr(args, k, None) for k in ("track_classes", "track_digits", "track_bin"))
    if tdir is None:
        if classes is not None or digits is not None or width is not None:
            sys.exit("--track_classes, --track_digits and --track_bin need --track_dir")
        return None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("--track_dir runs in one process (WORLD_SIZE > 1 is not supported for probability tracks)")
    digits = 2 if digits is None else digits
    width = 1 if width is None else width
    if not 1 <= digits <= 4:
        sys.exit(f"--track_digits must lie in 1..4, not {digits}")
    if width < 1:
        sys.exit(f"--track_bin must be at least 1, not {width}")
    bases, seen = {}, {}
    for f in args.FASTA:
        base = input_basename(f)
        if base in seen:
            sys.exit(f"--track_dir: {seen[base]} and {f} have the same file name; their tracks would collide")
        seen[base] = f
        bases[f] = base
    level = gzip_level(args, 1) if getattr(args, "track_gzip", False) else None
    return TrackPlan(tdir, tuple(classes) if classes is not None else None, digits, width, bases, level)


def resolve(p: TrackPlan, nclasses: int) -> TrackSpec:
    """The classes checked against the model's class count (sys.exit on a label it lacks); the default is 1..C-1."""
    classes = p.classes if p.classes is not None else tuple(range(1, nclasses))
    bad = [c for c in classes if not 0 <= c < nclasses]
    if bad:
        sys.exit(f"--track_classes: label {bad[0]} is not a class of this model (labels 0..{nclasses - 1})")
    return TrackSpec(tuple(dict.fromkeys(classes)), p.digits, p.bin, p.gzip_level)


def record_texts(pipe, merged, startpos: int, name, spec: TrackSpec) -> List[bytes]:
    """The track text of every class of `spec` for one record (merged: ContigPipeline.merged of it); with spec.gzip_level its BGZF
    members instead (no EOF member), deflated on the device piece by piece."""
    if spec.gzip_level is None:
        return [pipe.track_text(merged, startpos, name, c, spec.digits, spec.bin) for c in spec.classes]
    from . import gz
    out = []
    for c in spec.classes:
        d_text = pipe.track_text_device(merged, startpos, name, c, spec.digits, spec.bin)
        pieces = [gz.bgzf_compress_device(d_text[o:o + GZIP_PIECE], eof=False, level=spec.gzip_level).cpu().numpy().tobytes()
                  for o in range(0, int(d_text.numel()), GZIP_PIECE)]
        out.append(b"".join(pieces))
        del d_text
    return out


class TrackFiles:
    """The track files of one input, written to temporary files in the directory and renamed by `commit` (`abort` removes them).
    With spec.gzip_level `write` takes BGZF members and `commit` puts the EOF member behind them."""

    def __init__(self, p: TrackPlan, spec: TrackSpec, filename: str):
        os.makedirs(p.directory, exist_ok=True)
        self.gzip = spec.gzip_level is not None
        self.final = [track_path(p.directory, p.bases[filename], c, self.gzip) for c in spec.classes]
        self.tmp, self.fh = [], []
        try:
            for path in self.final:
                fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(path) + ".", suffix=".tmp", dir=p.directory)
                self.tmp.append(tmp)
                self.fh.append(os.fdopen(fd, "wb"))
        except BaseException:
            self.abort()
            raise

    def write(self, texts: Sequence[bytes]) -> None:
        for fh, t in zip(self.fh, texts):
            if t:
                fh.write(t)

    def commit(self) -> None:
        for fh in self.fh:
            if self.gzip:
                from .gz import BGZF_EOF
                fh.write(BGZF_EOF)
            fh.close()
        for tmp, path in zip(self.tmp, self.final):
            os.replace(tmp, path)
        self.tmp = []

    def abort(self) -> None:
        for fh in self.fh:
            fh.close()
        for tmp in self.tmp:
            if os.path.exists(tmp):
                os.remove(tmp)
        self.tmp = []


def quantise(v: np.ndarray, digits: int) -> np.ndarray:
    """floor(v * 10^D + 0.5) in float32, as the kernel rounds (two roundings), clamped to [0, 10^D]."""
    v = np.asarray(v, np.float32)
    q = np.floor(v * np.float32(10 ** digits) + np.float32(0.5))
    return np.clip(q, 0, 10 ** digits).astype(np.int64)


def reference_text(column: np.ndarray, startpos: int, name: bytes, digits: int = 2, bin: int = 1) -> bytes:
    """The bedGraph text of one class column (float32 [n], values in [0, 1]) of one record, in numpy: the format's statement."""
    v = np.asarray(column, np.float32)
    n = v.size
    if n == 0:
        return b""
    pos = np.arange(startpos, startpos + n, dtype=np.int64)
    k = pos // bin
    cut = np.flatnonzero(np.diff(k)) + 1
    first = np.r_[0, cut]                                           # the first base of every bin
    vmax = np.maximum(np.maximum.reduceat(v, first), np.float32(0))
    q = quantise(vmax, digits)
    lo = pos[first]
    hi = np.r_[pos[cut], startpos + n]
    change = np.r_[True, q[1:] != q[:-1]]
    rs = np.flatnonzero(change)
    re = np.r_[rs[1:], q.size]
    keep = q[rs] != 0
    scale = 10 ** digits
    return b"".join(b"%s\t%d\t%d\t%d.%0*d\n" % (name, lo[a], hi[b - 1], q[a] // scale, digits, q[a] % scale)
                    for a, b in zip(rs[keep], re[keep]))
