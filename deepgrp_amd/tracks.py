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
the file is committed.

With `--track_index` every `.gz` gets its tabix index `<track>.gz.tbi` (tabix.py states the format): chunks and linear index come
from the device in text offsets (dgrp_track_index_batch, for the arguments of the text), `TrackFiles` turns them into virtual
offsets with the compressed size of every member it appends, and `commit` writes the index."""
from __future__ import annotations

import logging
import os
import sys
import tempfile
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

_LOG = logging.getLogger(__name__)


class TrackSpec(NamedTuple):
    """What to write per record: the classes (one file each), decimals of the values, bin width in bases."""
    classes: Tuple[int, ...]
    digits: int = 2
    bin: int = 1
    gzip_level: Optional[int] = None                # None: plain text; else BGZF members at this level
    index: bool = False                             # --track_index: a tabix index beside every BGZF track


class TrackPlan(NamedTuple):
    directory: str
    classes: Optional[Tuple[int, ...]]              # None: every repeat class 1..C-1 (resolved by `resolve`)
    digits: int
    bin: int
    bases: dict                                     # input file -> basename of its track files
    gzip_level: Optional[int] = None                # --track_gzip: the level (None: plain bedGraph)
    index: bool = False                             # --track_index


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
    """The refusals of --track_gzip, --track_index and --gzip_level that need nothing but the flags (sys.exit)."""
    if getattr(args, "track_gzip", False) and getattr(args, "track_dir", None) is None:
        sys.exit("--track_gzip needs --track_dir")
    if getattr(args, "track_index", False) and not getattr(args, "track_gzip", False):
        sys.exit("--track_index needs --track_gzip (a tabix index belongs to a BGZF file)")
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
    return TrackPlan(tdir, tuple(classes) if classes is not None else None, digits, width, bases, level,
                     bool(getattr(args, "track_index", False)))


def resolve(p: TrackPlan, nclasses: int) -> TrackSpec:
    """The classes checked against the model's class count (sys.exit on a label it lacks); the default is 1..C-1."""
    classes = p.classes if p.classes is not None else tuple(range(1, nclasses))
    bad = [c for c in classes if not 0 <= c < nclasses]
    if bad:
        sys.exit(f"--track_classes: label {bad[0]} is not a class of this model (labels 0..{nclasses - 1})")
    return TrackSpec(tuple(dict.fromkeys(classes)), p.digits, p.bin, p.gzip_level, p.index)


class WriteIndex(NamedTuple):
    """What one write (a record, or a batch) adds to the indexes of its input: the records' names and, in offsets of every class's
    text, ContigPipeline.track_index_batch_device's arrays -- or why this input cannot have an index."""
    names: List[bytes]
    refused: Optional[str] = None
    chunks: Optional[np.ndarray] = None
    chunk_off: Optional[np.ndarray] = None
    linear: Optional[np.ndarray] = None
    wpref: Optional[np.ndarray] = None


class TrackTexts(list):
    """The texts (or BGZF members) of one write, class by class; with --track_index `index` is its WriteIndex."""
    index: Optional[WriteIndex] = None


def write_index(pipe, d_probs, row0, lengths, startposes, names, spec: TrackSpec) -> WriteIndex:
    """The WriteIndex of the records whose text track_text_batch_device gives for the same arguments."""
    from .tabix import MAX_END
    raw = [nm if isinstance(nm, bytes) else nm.encode("utf-8", "surrogateescape") for nm in names]
    for nm, sp, n in zip(raw, startposes, lengths):
        if int(sp) + int(n) > MAX_END:
            return WriteIndex(raw, f"record {nm.decode('utf-8', 'replace')!r} ends at {int(sp) + int(n)}, above 2^29 = {MAX_END}, the "
                                   "largest coordinate of a tabix index")
    return WriteIndex(raw, None, *pipe.track_index_batch_device(d_probs, row0, lengths, startposes, raw, spec.classes, spec.digits, spec.bin))


def record_texts(pipe, merged, startpos: int, name, spec: TrackSpec) -> List[bytes]:
    """The track text of every class of `spec` for one record (merged: ContigPipeline.merged of it); with spec.gzip_level its BGZF
    members instead (no EOF member), deflated on the device piece by piece; with spec.index a TrackTexts with the record's index."""
    if spec.gzip_level is None:
        return [pipe.track_text(merged, startpos, name, c, spec.digits, spec.bin) for c in spec.classes]
    from . import gz
    out = TrackTexts()
    for c in spec.classes:
        d_text = pipe.track_text_device(merged, startpos, name, c, spec.digits, spec.bin)
        pieces = [gz.bgzf_compress_device(d_text[o:o + GZIP_PIECE], eof=False, level=spec.gzip_level).cpu().numpy().tobytes()
                  for o in range(0, int(d_text.numel()), GZIP_PIECE)]
        out.append(b"".join(pieces))
        del d_text
    if spec.index and len(merged):
        out.index = write_index(pipe, merged, [0], [len(merged)], [startpos], [name], spec)
    return out


class TrackFiles:
    """The track files of one input, written to temporary files in the directory and renamed by `commit` (`abort` removes them).
    With spec.gzip_level `write` takes BGZF members and `commit` puts the EOF member behind them.  With spec.index it keeps, per
    class, the file offset of every write and a tabix.IndexBuilder, and `commit` writes `<track>.gz.tbi` the same way.  An input
    whose records cannot be indexed (WriteIndex.refused, a name that reappears after another name, an empty name) gets one warning
    and no index; its tracks are what they are without the flag."""

    def __init__(self, p: TrackPlan, spec: TrackSpec, filename: str):
        os.makedirs(p.directory, exist_ok=True)
        self.gzip = spec.gzip_level is not None
        self.final = [track_path(p.directory, p.bases[filename], c, self.gzip) for c in spec.classes]
        self.tmp, self.fh = [], []
        self.filename, self.builders = filename, None
        if self.gzip and spec.index:
            from .tabix import IndexBuilder
            self.builders = [IndexBuilder() for _ in spec.classes]
            self.offs = [0] * len(spec.classes)
            self.seen, self.last = set(), None
        self.index_wanted = self.builders is not None
        try:
            for path in self.final:
                fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(path) + ".", suffix=".tmp", dir=p.directory)
                self.tmp.append(tmp)
                self.fh.append(os.fdopen(fd, "wb"))
        except BaseException:
            self.abort()
            raise

    def _no_index(self, why: str) -> None:
        if self.builders is not None:
            _LOG.warning("%s: no tabix index is written (--track_index): %s", self.filename, why)
            self.builders = None

    def _index(self, texts: Sequence[bytes]) -> None:
        """The write's part of every class's index; the members of class k go to file offset self.offs[k]."""
        from .tabix import IndexRefused, member_sizes
        ix = getattr(texts, "index", None)
        if ix is None:
            if any(texts):
                self._no_index("a write came without its index")
            return
        for nm in ix.names:
            if not nm:
                return self._no_index("a record with an empty name")
            if nm != self.last:
                if nm in self.seen:
                    return self._no_index(f"the record name {nm.decode('utf-8', 'replace')!r} reappears after another name")
                self.seen.add(nm)
                self.last = nm
        if ix.refused is not None:
            return self._no_index(ix.refused)
        for k, t in enumerate(texts):
            if t:
                sizes, text_len = member_sizes(t)
                try:
                    self.builders[k].add(self.offs[k], sizes, text_len, ix.names, ix.chunks[ix.chunk_off[k]:ix.chunk_off[k + 1]],
                                         ix.linear[k], ix.wpref)
                except IndexRefused as e:
                    return self._no_index(str(e))
                self.offs[k] += len(t)

    def write(self, texts: Sequence[bytes]) -> None:
        for fh, t in zip(self.fh, texts):
            if t:
                fh.write(t)
        if self.builders is not None:
            self._index(texts)

    def commit(self) -> None:
        for fh in self.fh:
            if self.gzip:
                from .gz import BGZF_EOF
                fh.write(BGZF_EOF)
            fh.close()
        if self.index_wanted:
            self._commit_index()
        for tmp, path in zip(self.tmp, self.final):
            os.replace(tmp, path)
        self.tmp = []

    def _commit_index(self) -> None:
        """`<track>.gz.tbi` of every class through a temporary file; without an index, one left by an earlier run goes."""
        from .tabix import index_file
        tbi = [path + ".tbi" for path in self.final]
        if self.builders is None:
            for path in tbi:
                if os.path.exists(path):
                    os.remove(path)
            return
        for b, path in zip(self.builders, tbi):
            fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path))
            self.tmp.append(tmp)
            self.final.append(path)
            with os.fdopen(fd, "wb") as fh:
                fh.write(index_file(b.payload()))

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
