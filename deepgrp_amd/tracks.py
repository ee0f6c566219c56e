"""Per-class probability tracks (`predict --track_dir`): for every input file and selected class, a bedGraph file of the merged class
probabilities the model computes for each base (ContigPipeline.merged), as text built on the GPU (dgrp_track_text).

A line is `name<TAB>start<TAB>end<TAB>value<LF>`: the record's name (evaluation.record_name, raw header bytes), a 0-based half-open
span in the TSV's coordinates, and the maximum probability of the class over the span's bins at `digits` decimals.  Bin k is
[k * bin, (k + 1) * bin) of the record's coordinates, clipped to the predicted span [startpos, startpos + n); consecutive bins of
equal value are one line, and spans of value 0 are left out.  `reference_text` restates the format in numpy.

Short records run as batches (ContigPipeline.run_batch_probs: dgrp_predict_batch_probs, then batch_track_texts: dgrp_track_text_batch
for all records and classes of the batch); the text of a batch is the records' texts one after the other.

With `--track_gzip` the files are `<basename>.class<c>.bedGraph.gz`, BGZF as bgzip writes it: the text of a record (of a batch: of one
class of all its records) is deflated on the device where it was written (gz.bgzf_compress_device, --gzip_level, 1 unless given) and
only the members are read back and appended; a record or batch boundary is a short member, and the EOF member is written once, when
the file is committed.

With `--track_index` every `.gz` gets its tabix index `<track>.gz.tbi` (tabix.py states the format): chunks and linear index come
from the device in text offsets (dgrp_track_index_batch, for the arguments of the text), `TrackFiles` turns them into virtual
offsets with the compressed size of every member it appends, and `commit` writes the index.

With `--track_bigwig` the files are `<basename>.class<c>.bw` instead, bigWig as bigwig.py states it: the same items in binary
sections with ten zoom levels at most, sections and zoom records written and deflated on the device (`bigwig_write`), the container
put around them by a bigwig.BigWigBuilder per class."""
from __future__ import annotations

import argparse
import logging
import os
import sys
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .outfiles import BgzfSink, StagedFile, StagedOutputs, class_list

_LOG = logging.getLogger(__name__)


class TrackSpec(NamedTuple):
    """What to write per record: the classes (one file each), decimals of the values, bin width in bases."""
    classes: Tuple[int, ...]
    digits: int = 2
    bin: int = 1
    gzip_level: Optional[int] = None                # None: plain text; else BGZF members at this level
    index: bool = False                             # --track_index: a tabix index beside every BGZF track
    bigwig: bool = False                            # --track_bigwig: bigWig files (zlib streams at gzip_level) instead of bedGraph
    index_format: str = "tbi"                       # --index_format: "csi" for <track>.gz.csi (tabix.CSI_DEPTH levels, up to 2^32)


class TrackPlan(NamedTuple):
    directory: str
    classes: Optional[Tuple[int, ...]]              # None: every repeat class 1..C-1 (resolved by `resolve`)
    digits: int
    bin: int
    bases: dict                                     # input file -> basename of its track files
    gzip_level: Optional[int] = None                # --track_gzip: the level (None: plain bedGraph)
    index: bool = False                             # --track_index
    bigwig: bool = False                            # --track_bigwig (gzip_level is then the level of its zlib streams)
    index_format: str = "tbi"                       # --index_format


def input_basename(filename: str) -> str:
    return "stdin" if filename == "-" else os.path.basename(filename)


def track_path(directory: str, base: str, cls: int, gzip: bool = False, bigwig: bool = False) -> str:
    if bigwig:
        return os.path.join(directory, f"{base}.class{cls}.bw")
    return os.path.join(directory, f"{base}.class{cls}.bedGraph" + (".gz" if gzip else ""))


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
    """The refusals of --track_gzip, --track_index, --track_bigwig and --gzip_level that need nothing but the flags (sys.exit)."""
    if getattr(args, "track_gzip", False) and getattr(args, "track_dir", None) is None:
        sys.exit("--track_gzip needs --track_dir")
    if getattr(args, "track_bigwig", False):
        if getattr(args, "track_dir", None) is None:
            sys.exit("--track_bigwig needs --track_dir")
        if getattr(args, "track_gzip", False) or getattr(args, "track_index", False):
            sys.exit("--track_bigwig writes bigWig files instead of bedGraph: it does not go with --track_gzip or --track_index")
    if getattr(args, "track_index", False) and not getattr(args, "track_gzip", False):
        sys.exit("--track_index needs --track_gzip (a tabix index belongs to a BGZF file)")
    if getattr(args, "index_format", None) is not None and not (getattr(args, "track_index", False) or getattr(args, "bed_index", False)):
        sys.exit("--index_format needs --track_index or --bed_index (it chooses the format of their index)")
    if getattr(args, "gzip_level", None) is not None:
        if not (getattr(args, "mask_gzip", False) or getattr(args, "track_gzip", False) or getattr(args, "track_bigwig", False)
                or getattr(args, "bed_gzip", False) or getattr(args, "bed_bigbed", False) or getattr(args, "seq_gzip", False)):
            sys.exit("--gzip_level needs --mask_gzip or --track_gzip or --bed_gzip")
        gzip_level(args, 0)


def add_options(parser) -> None:
    """The probability-track flags, like the masking flags on `predict` and on the main parser, set only where given."""
    s = argparse.SUPPRESS
    parser.add_argument("--track_dir", type=str, default=s,
                        help="(addition) also write the merged per-base probabilities of every selected class as bedGraph files "
                             "DIR/<basename of the input>.class<c>.bedGraph ('stdin' for '-'); with --fast they are those of the "
                             "fp16-operand kernels")
    parser.add_argument("--track_gzip", action="store_true", default=s,
                        help="(addition) with --track_dir: write every track as BGZF (bgzip's format, deflated on the GPU where the "
                             "text is made) to DIR/<basename>.class<c>.bedGraph.gz")
    parser.add_argument("--track_index", action="store_true", default=s,
                        help="(addition) with --track_gzip: write the tabix index <track>.gz.tbi of every track, built on the GPU "
                             "beside the text (records must end at or below 2^29 and names must not reappear after another name; "
                             "otherwise a warning and no index)")
    parser.add_argument("--index_format", choices=("tbi", "csi"), default=s,
                        help="(addition) with --track_index or --bed_index: the format of the index.  tbi (the default): <file>.gz.tbi, "
                             "records up to 2^29 bases.  csi: <file>.gz.csi, a CSI index of depth 6 with the same chunks and a "
                             "per-bin offset in place of the linear index, records up to 2^32 bases (the format tabix -C writes); "
                             "an index of the other format beside the file is removed")
    parser.add_argument("--track_bigwig", action="store_true", default=s,
                        help="(addition) with --track_dir: write every track as bigWig, DIR/<basename>.class<c>.bw, instead of bedGraph: "
                             "the same items in binary sections with zoom levels, built and deflated on the GPU (--gzip_level, 1 unless "
                             "given).  A chromosome's size is the end of its predicted span (trailing N are not counted).  Record "
                             "names must be non-empty and distinct and records must end at or below 2^32 - 1; otherwise a warning and "
                             "no bigWig for that input.  Not with --track_gzip or --track_index")
    parser.add_argument("--track_classes", type=class_list, default=s,
                        help="(addition) comma-separated classes to write tracks of, 0 included (default: every repeat class 1..C-1)")
    parser.add_argument("--track_digits", type=int, default=s,
                        help="(addition) decimals of the track values, 1..4 (default: 2)")
    parser.add_argument("--track_bin", type=int, default=s,
                        help="(addition) bin width of the tracks in bases, >= 1; a bin's value is the maximum over its bases "
                             "(default: 1)")


def index_format(args) -> str:
    """--index_format, "tbi" where it is not given."""
    return getattr(args, "index_format", None) or "tbi"


def index_depth(fmt: str) -> int:
    """The levels below the root of the index's binning scheme: 5 of a `.tbi`, tabix.CSI_DEPTH of a `.csi`."""
    from .tabix import CSI_DEPTH
    return CSI_DEPTH if fmt == "csi" else 5


def refuse_on_evaluate(args) -> None:
    if getattr(args, "index_format", None) is not None:
        sys.exit("--index_format belongs to predict, not evaluate")
    if (getattr(args, "track_dir", None) is not None or getattr(args, "track_gzip", False) or getattr(args, "track_index", False)
            or getattr(args, "track_bigwig", False)):
        sys.exit("--track_dir belongs to predict, not evaluate")


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
    bigwig = bool(getattr(args, "track_bigwig", False))
    level = gzip_level(args, 1) if getattr(args, "track_gzip", False) or bigwig else None
    return TrackPlan(tdir, tuple(classes) if classes is not None else None, digits, width, bases, level,
                     bool(getattr(args, "track_index", False)), bigwig, index_format(args))


def resolve(p: TrackPlan, nclasses: int) -> TrackSpec:
    """The classes checked against the model's class count (sys.exit on a label it lacks); the default is 1..C-1."""
    classes = p.classes if p.classes is not None else tuple(range(1, nclasses))
    bad = [c for c in classes if not 0 <= c < nclasses]
    if bad:
        sys.exit(f"--track_classes: label {bad[0]} is not a class of this model (labels 0..{nclasses - 1})")
    return TrackSpec(tuple(dict.fromkeys(classes)), p.digits, p.bin, p.gzip_level, p.index, p.bigwig, p.index_format)


def from_plan(p: TrackPlan, classes: int) -> "Tracks":
    return Tracks(p, resolve(p, classes))


class Tracks:
    """--track_dir as an output of `predict`: every work item's rows come with the track texts of its records, which go to the
    input's TrackFiles."""
    wants_rows = False

    def __init__(self, p: TrackPlan, spec: TrackSpec):
        self.plan, self.spec = p, spec
        self.runner = dict(tracks=spec)                 # what is asked of the RecordRunner

    def open(self, filename: str) -> "TrackFiles":
        return TrackFiles(self.plan, self.spec, filename)


class WriteIndex(NamedTuple):
    """What one write (a record, or a batch) adds to the indexes of its input: the records' names and, in offsets of every class's
    text, ContigPipeline.track_index_batch_device's arrays -- or why this input cannot have an index."""
    names: List[bytes]
    refused: Optional[str] = None
    chunks: Optional[np.ndarray] = None
    chunk_off: Optional[np.ndarray] = None
    linear: Optional[np.ndarray] = None
    wpref: Optional[np.ndarray] = None


class BigWigWrite(NamedTuple):
    """What one write (a record, or a batch) adds to the bigWig files of its input: the records' names and chromSizes (startpos + n)
    and, class by class, a bigwig.ClassWrite -- or why this input cannot have bigWig files."""
    names: List[bytes]
    sizes: List[int]
    refused: Optional[str] = None
    classes: Optional[list] = None                  # None: records without a predicted base (names and sizes only)
    chrom0: Optional[int] = None                    # the chromId of the first record, as the device wrote it (None: unchecked)


class TrackTexts(list):
    """The texts (or BGZF members) of one write, class by class; with --track_index `index` is its WriteIndex.  With
    --track_bigwig the entries are the compressed sections and `bigwig` is the write's BigWigWrite."""
    index: Optional[WriteIndex] = None
    bigwig: Optional[BigWigWrite] = None


ZLIB_PIECE = 4096                                   # blocks deflated per call (gz.GZIP_PIECE's reason: the level-1 workspace)


def _zlib_pieces(pipe, d_in, d_table, stride: int, level: int):
    """The blocks of a table as zlib streams, ZLIB_PIECE blocks a call: -> (bytes, int64 sizes)."""
    blobs, sizes = [], []
    for a in range(0, int(d_table.numel()), ZLIB_PIECE * stride):
        d_out, d_sizes = pipe.zlib_compress_device(d_in, d_table[a:a + ZLIB_PIECE * stride], stride, level)
        blobs.append(d_out.cpu().numpy().tobytes())
        sizes.append(d_sizes.cpu().numpy())
    return b"".join(blobs), (np.concatenate(sizes) if sizes else np.zeros(0, np.int64))


def empty_texts(spec: TrackSpec, name, startpos: int):
    """The write of a record without a predicted base: no text; with spec.bigwig its name and size for the chromosome tree."""
    from ._lib import name_blob
    out = TrackTexts(b"" for _ in spec.classes)
    out.bigwig = BigWigWrite(name_blob([name])[0], [int(startpos)], None, None) if spec.bigwig else None
    return out


def bigwig_write(pipe, d_probs, row0, lengths, startposes, names, spec: TrackSpec, chrom0: int = 0) -> TrackTexts:
    """The bigWig part of the records whose text track_text_batch_device gives for the same arguments: sections and zoom blocks
    from the device (dgrp_track_sections_batch, dgrp_track_zoom_batch), deflated there (dgrp_zlib_compress_batch).  chrom0 is
    the ordinal of the first record in its input: chromIds count from there."""
    from . import bigwig as bw
    from ._lib import name_blob
    raw = name_blob(names)[0]
    sizes = [int(sp) + int(n) for sp, n in zip(startposes, lengths)]
    out = TrackTexts(b"" for _ in spec.classes)
    for nm, end in zip(raw, sizes):
        if end > bw.MAX_END:
            out.bigwig = BigWigWrite(raw, sizes, f"record {nm.decode('utf-8', 'replace')!r} ends at {end}, above 2^32 - 1 = {bw.MAX_END}, "
                                                 "the largest coordinate of a bigWig")
            return out
    args = (d_probs, row0, lengths, startposes, spec.classes, spec.digits, spec.bin, chrom0)
    level = 1 if spec.gzip_level is None else spec.gzip_level
    d_sec, _off, d_stab, soff = pipe.track_sections_batch_device(*args)
    sec_blob, sec_sizes = _zlib_pieces(pipe, d_sec, d_stab, bw.SECTION_DTYPE.itemsize, level)
    stab = d_stab.cpu().numpy().view(bw.SECTION_DTYPE)
    del d_sec, d_stab
    d_zoom, _roff, d_ztab, boff, totals = pipe.track_zoom_batch_device(*args)
    zoom_blob, zoom_sizes = _zlib_pieces(pipe, d_zoom, d_ztab, bw.ZOOM_BLOCK_DTYPE.itemsize, level)
    ztab = d_ztab.cpu().numpy().view(bw.ZOOM_BLOCK_DTYPE)
    del d_zoom, d_ztab
    sat, zat = np.r_[0, np.cumsum(sec_sizes)], np.r_[0, np.cumsum(zoom_sizes)]
    writes = []
    for k in range(len(spec.classes)):
        a, b = int(soff[k]), int(soff[k + 1])
        za, zb = int(boff[k * bw.ZOOM_LEVELS]), int(boff[(k + 1) * bw.ZOOM_LEVELS])
        writes.append(bw.ClassWrite(sec_blob[int(sat[a]):int(sat[b])], sec_sizes[a:b], stab[a:b], zoom_blob[int(zat[za]):int(zat[zb])],
                                    zoom_sizes[za:zb], ztab[za:zb], tuple(int(x) for x in totals[k])))
        out[k] = writes[-1].sections
    out.bigwig = BigWigWrite(raw, sizes, None, writes, chrom0)
    return out


def write_index(pipe, d_probs, row0, lengths, startposes, names, spec: TrackSpec) -> WriteIndex:
    """The WriteIndex of the records whose text track_text_batch_device gives for the same arguments."""
    from ._lib import name_blob
    from .tabix import end_refusal
    raw = name_blob(names)[0]
    depth = index_depth(spec.index_format)
    refused = end_refusal([int(sp) + int(n) for sp, n in zip(startposes, lengths)], raw, depth)
    if refused is not None:
        return WriteIndex(raw, refused)
    return WriteIndex(raw, None, *pipe.track_index_batch_device(d_probs, row0, lengths, startposes, raw, spec.classes, spec.digits,
                                                                spec.bin, depth))


def record_texts(pipe, merged, startpos: int, name, spec: TrackSpec, chrom: int = 0) -> List[bytes]:
    """The track text of every class of `spec` for one record (merged: ContigPipeline.merged of it); with spec.gzip_level its BGZF
    members instead (no EOF member), deflated on the device piece by piece; with spec.index a TrackTexts with the record's index; with
    spec.bigwig the record's bigwig_write (chrom: its ordinal in the input)."""
    if spec.bigwig:
        return bigwig_write(pipe, merged, [0], [len(merged)], [startpos], [name], spec, chrom)
    if spec.gzip_level is None:
        return [pipe.track_text(merged, startpos, name, c, spec.digits, spec.bin) for c in spec.classes]
    from .gz import bgzf_members_device
    out = TrackTexts(bgzf_members_device(pipe.track_text_device(merged, startpos, name, c, spec.digits, spec.bin), spec.gzip_level)
                     for c in spec.classes)
    if spec.index and len(merged):
        out.index = write_index(pipe, merged, [0], [len(merged)], [startpos], [name], spec)
    return out


class _BigWigFile(StagedFile):
    """One `.bw` file: a bigwig.BigWigBuilder (`bw`) on the staged file."""

    def __init__(self, final: str, digits: int, bin: int):
        from .bigwig import BigWigBuilder
        super().__init__(final, "w+b")
        try:
            self.bw = BigWigBuilder(self.fh, digits, bin, os.path.dirname(final))
        except BaseException:
            super().abort()
            raise

    def finish(self) -> None:
        self.bw.finish()
        self.fh.close()

    def abort(self) -> None:
        self.bw.close()
        super().abort()


class TrackFiles(StagedOutputs):
    """The track files of one input: temporary files in the directory, renamed by `commit`, removed by `abort` (outfiles.py).  With
    spec.gzip_level `write` takes BGZF members, to an outfiles.BgzfSink per class, which with spec.index builds `<track>.gz.tbi`
    (`<track>.gz.csi` with spec.index_format "csi").  An input whose records cannot be indexed (WriteIndex.refused, an empty name, a name that comes back: one name_order for all
    classes) gets one warning and no index; its tracks are what they are without the flag.  With spec.bigwig the files are `.bw`,
    every class has a bigwig.BigWigBuilder on its temporary file, `write` takes TrackTexts with a BigWigWrite, and an input a
    bigWig cannot hold (an empty name, a name two records share, a record that ends above 2^32 - 1) gets one warning and no `.bw`
    files: `commit` then removes the temporary files and any `.bw` an earlier run left."""

    def __init__(self, p: TrackPlan, spec: TrackSpec, filename: str):
        os.makedirs(p.directory, exist_ok=True)
        self.bigwig = bool(spec.bigwig)
        self.gzip = spec.gzip_level is not None and not self.bigwig
        self.final = [track_path(p.directory, p.bases[filename], c, self.gzip, self.bigwig) for c in spec.classes]
        self.bw_refused = None
        super().__init__(_LOG, filename, "--track_index", self.gzip and spec.index,
                         (_BigWigFile(path, spec.digits, spec.bin) if self.bigwig else BgzfSink(path, spec.index, fmt=spec.index_format) if self.gzip
                          else StagedFile(path) for path in self.final))

    def _bigwig(self, texts: Sequence[bytes]) -> None:
        """The write's part of every class's bigWig, or the input's refusal (one warning)."""
        w = getattr(texts, "bigwig", None)
        if self.bw_refused is not None or (w is None and not any(texts)):
            return
        why = "a write came without its sections" if w is None else w.refused
        if why is None:
            why = self.distinct_names(w.names)
        if why is not None:
            self.bw_refused = why
            _LOG.warning("%s: no bigWig files are written (--track_bigwig): %s", self.filename, why)
            return
        have = len(self.parts[0].bw.names)
        if w.chrom0 is not None and w.chrom0 != have:
            raise ValueError(f"{self.filename}: a bigWig write of chromId {w.chrom0} arrived as record {have} of the input")
        for k, p in enumerate(self.parts):
            p.bw.add(w.names, w.sizes, None if w.classes is None else w.classes[k])

    def take(self, names, batch: bool, rows, scores, texts: Sequence[bytes]) -> None:
        self.write(texts)

    def commit(self, rows=None, log=None) -> None:
        if self.bw_refused is None:
            return super().commit()
        self.abort()
        for path in self.final:
            if os.path.exists(path):
                os.remove(path)

    def write(self, texts: Sequence[bytes]) -> None:
        """The write's text (or members) of every class; with an index, the names of its WriteIndex count in the order, and a
        write with text but no index ends the index."""
        if self.bigwig:
            return self._bigwig(texts)
        ix = getattr(texts, "index", None)
        if self.indexed and ix is None:
            self.no_index("a write came without its index" if any(texts) else None)
        elif self.indexed:
            self.no_index(self.name_order(ix.names) or ix.refused)
        for k, t in enumerate(texts):
            if t and self.indexed:
                self.append(k, t, ix.names, ix.chunks[ix.chunk_off[k]:ix.chunk_off[k + 1]], ix.linear[k], ix.wpref)
            else:
                self.append(k, t)


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
