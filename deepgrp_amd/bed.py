"""Scored BED of the predicted repeats (`predict --bed_dir`): for every input file one `DIR/<basename>.bed` with a line per TSV row,

    name<TAB>start<TAB>end<TAB>class<label><TAB>score<TAB>.<TAB>mean<TAB>min<TAB>agree<LF>

name is the record's name (evaluation.record_name, the first word of the header, as the tracks use it), start and end the TSV's
coordinates.  The figures say how sure the model is of the element, from the merged probabilities of the row's own class over the
row's bases (ContigPipeline.merged, the array the labels are computed from): `mean` and `min` are the mean and the smallest of them,
`agree` the fraction of the bases at which that class is the largest column, `score` the mean on BED's 0..1000 scale.

Everything is exact integer arithmetic.  A probability p becomes q(p) = round-half-up(p * 2^24) clamped to [0, 2^24] (0 for a NaN);
the device sums, minimises and counts per row (dgrp_row_scores_batch, ROW_SCORE_DTYPE), the host formatter (dgrp_format_bed_rows)
rounds the quotients half up.  `reference_scores` and `reference_lines` restate both in numpy and Python integers.

With `--bed_gzip` the file is `DIR/<basename>.bed.gz`, BGZF as bgzip writes it.  Rows and scores then stay on the device: the lines
are written there (dgrp_bed_text_batch, the host formatter's bytes), deflated there (gz.bgzf_compress_device, --gzip_level, 1
unless given) in pieces of gz.GZIP_PIECE, and only the members are read back; the text of one record, or of one batch, is one
write, so a record or batch boundary is a short member, and the EOF member is written at `commit`.  With `--bed_index` the file
gets its tabix index `<basename>.bed.gz.tbi`: chunks and linear index come from the device in text offsets (dgrp_bed_index_batch;
`reference_index_parts` restates them), `BedFiles` turns them into virtual offsets with the compressed size of every member it
appends (tabix.IndexBuilder).  The index is tabix.reference_index of the finished `.bed.gz`: that function reads name, start and
end of every line of a BGZF file and nothing else, so it states the index of a BED as it states a track's.

With `--bed_bigbed` the file is `DIR/<basename>.bb` instead, bigBed as bigbed.py states it: one item per BED line, the extra columns
typed by an autoSql declaration, 32-bit coordinates (a tabix index ends at 2^29), an R-tree over the item blocks and coverage zoom
levels.  Item blocks and zoom records are written and deflated on the device (ContigPipeline.bigbed_write); `BedFiles` puts the
container around them with a bigbed.BigBedBuilder.  An input a bigBed cannot hold (an empty record name, two records of one name,
a record that ends above 2^32 - 1) gets one warning and no `.bb`.

With `--bed_gff3` the file is `DIR/<basename>.gff3` instead (`.gff3.gz` with --bed_gzip, `.gff3.gz.tbi` with --bed_index), GFF3 as
gff.py states it: the same rows and figures, written on the device whether deflated or not (ContigPipeline.gff_write).  The `ID`
ordinals run through the file, so `BedFiles` counts the lines and hands every write its first ordinal (gff.GffWrite.render).  An
input with an empty record name gets one warning and no `.gff3`.

With `--bed_rmout` the file is `DIR/<basename>.out` instead (`.out.gz` with --bed_gzip), a RepeatMasker listing as rmout.py states
it: the same rows with the BED's score, named after the numbered families of `parse_rm` (--rmout_repeats) or after --bed_names,
written on the device whether deflated or not (ContigPipeline.rmout_write).  The IDs run through the file and fragments that
--rmout_join joins share one, so `BedFiles` counts the IDS used and hands every write its first (rmout.RmoutWrite.render).  An input
with a record name that cannot stand in a blank-separated column gets one warning and no `.out`."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import logging
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .outfiles import BgzfSink, StagedFile, StagedOutputs

_LOG = logging.getLogger(__name__)

ONE = 1 << 24                                       # q(1.0): the fixed-point unit


class BedPlan(NamedTuple):
    directory: str
    min_score: int
    paths: dict                                     # input file -> its BED file
    gzip_level: Optional[int] = None                # --bed_gzip: the level (None: plain text from the host formatter)
    index: bool = False                             # --bed_index
    bigbed: bool = False                            # --bed_bigbed (gzip_level is then the level of its zlib streams)
    gff3: bool = False                              # --bed_gff3 (gzip_level None: the device's text, not deflated)
    class_names: Optional[tuple] = None             # --bed_names: the name of label 1..C-1, as given (gff.py escapes them)
    rmout: bool = False                             # --bed_rmout (gzip_level None: the device's text, not deflated)
    rmout_repeats: Optional[tuple] = None           # --rmout_repeats: the repeat number of label 1..C-1 (None: 1..C-1)
    rmout_join: int = -1                            # --rmout_join: the largest gap inside one ID (-1: every line its own)
    rmout_pairs: Optional[tuple] = None             # (repeat, class/family) of label 1..C-1, once the class count is known (from_plan)
    index_format: str = "tbi"                       # --index_format: "csi" for <file>.gz.csi (tabix.CSI_DEPTH levels, up to 2^32)

    @property
    def on_device(self) -> bool:
        """Whether the write is made on the device (ContigPipeline.bed_write) rather than from scores on the host."""
        return self.gzip_level is not None or self.gff3 or self.rmout


class BedWrite(NamedTuple):
    """What one write (a record, or a batch) adds to a BGZF BED: its members (no EOF member), the records' names and, with
    --bed_index, ContigPipeline.bed_index_batch's arrays in offsets of the write's text -- or why this input cannot have an index."""
    members: bytes
    names: List[bytes]
    refused: Optional[str] = None
    chunks: Optional[np.ndarray] = None
    linear: Optional[np.ndarray] = None
    wpref: Optional[np.ndarray] = None
    last_end: Optional[np.ndarray] = None


def bed_path(directory: str, filename: str, gzip: bool = False, bigbed: bool = False, gff3: bool = False, rmout: bool = False) -> str:
    from .tracks import input_basename
    if bigbed:
        return os.path.join(directory, input_basename(filename) + ".bb")
    return os.path.join(directory, input_basename(filename) + (".out" if rmout else ".gff3" if gff3 else ".bed") + (".gz" if gzip else ""))


def empty_write(p: BedPlan, name, startpos: int, chrom: int = 0):
    """The device write of a record without a predicted base: no members; with p.bigbed its name and size for the chromosome tree
    (chrom: its ordinal in the input)."""
    from ._lib import name_blob
    raw = name_blob([name])[0]
    if p.bigbed:
        from .bigbed import BigBedWrite, end_refusal
        return BigBedWrite(raw, [int(startpos)], end_refusal(raw, [int(startpos)]), chrom0=chrom)
    if p.gff3:
        from .gff import GffWrite
        return GffWrite(raw)
    if p.rmout:
        from .rmout import RmoutWrite
        return RmoutWrite(raw)
    return BedWrite(b"", raw)


def add_options(parser) -> None:
    """The scored-BED flags, like the track flags on `predict` and on the main parser, set only where given."""
    s = argparse.SUPPRESS
    parser.add_argument("--bed_dir", type=str, default=s,
                        help="(addition) also write the predicted repeats of every input as BED, DIR/<basename of the input>.bed ('stdin' "
                             "for '-'): name, start, end, class<label>, score 0..1000, '.', then the mean and the smallest merged "
                             "probability of the row's class over its bases and the share of its bases at which that class is the "
                             "largest, four decimals each; summed on the GPU; one process only")
    parser.add_argument("--bed_min_score", type=int, default=s,
                        help="(addition) with --bed_dir: leave out BED lines whose score is below this, 0..1000 (the TSV is not filtered)")
    parser.add_argument("--bed_gzip", action="store_true", default=s,
                        help="(addition) with --bed_dir: write the BED as BGZF (bgzip's format) to DIR/<basename>.bed.gz; the lines are "
                             "written and deflated on the GPU (--gzip_level, 1 unless given)")
    parser.add_argument("--bed_index", action="store_true", default=s,
                        help="(addition) with --bed_gzip: write the tabix index <basename>.bed.gz.tbi, built on the GPU beside the text "
                             "(records must end at or below 2^29 and names must not reappear after another name; otherwise a warning "
                             "and no index)")
    parser.add_argument("--bed_bigbed", action="store_true", default=s,
                        help="(addition) with --bed_dir: write the scored repeats as bigBed, DIR/<basename>.bb, instead of BED text: one "
                             "item per BED line (bed6+3, the extra columns typed by an autoSql declaration) with coverage zoom levels, "
                             "built and deflated on the GPU (--gzip_level, 1 unless given); coordinates up to 2^32 - 1.  Record names "
                             "must be non-empty and distinct and records must end at or below 2^32 - 1; otherwise a warning and no "
                             "bigBed for that input.  Not with --bed_gzip or --bed_index")
    parser.add_argument("--bed_gff3", action="store_true", default=s,
                        help="(addition) with --bed_dir: write the scored repeats as GFF3, DIR/<basename>.gff3, instead of BED text: "
                             "'##gff-version 3', then per row seqid, deepgrp, repeat_region, start+1, end, mean, '.', '.', "
                             "ID=r<ordinal>;Name=class<label>;label=;score=;min=;agree= with the BED's figures, written on the GPU.  "
                             "With --bed_gzip DIR/<basename>.gff3.gz (BGZF), with --bed_index its tabix index (gff preset) beside it.  "
                             "A record with an empty name: a warning and no GFF3 for that input.  Not with --bed_bigbed")
    parser.add_argument("--bed_names", type=str, default=s,
                        help="(addition) with --bed_gff3: the names of the labels 1..classes-1, comma-separated, written as Name= in the "
                             "place of class<label> (each 1..255 bytes; reserved characters are %%-escaped); with --summary_dir: the "
                             "label column of its tables; with --bed_rmout: repeat#class/family per label, the naming of "
                             "RepeatMasker's libraries (exactly one '#', no blank)")
    parser.add_argument("--bed_rmout", action="store_true", default=s,
                        help="(addition) with --bed_dir: write the scored repeats as a RepeatMasker listing, DIR/<basename>.out, instead "
                             "of BED text: the two title lines, then per row the BED's score, 0.0 0.0 0.0 (no divergence is "
                             "predicted), the record's name, start+1, end, (left), +, repeat, class/family, 1, end-start, (0), ID, "
                             "written on the GPU.  With --bed_gzip DIR/<basename>.out.gz (BGZF).  A record name with a blank: a "
                             "warning and no listing for that input.  Not with --bed_bigbed, --bed_gff3 or --bed_index")
    parser.add_argument("--rmout_repeats", type=str, default=s, metavar="N,N,...",
                        help="(addition) with --bed_rmout: the repeat number (1..10, the numbered families of parse_rm) of the labels "
                             "1..classes-1, distinct; 1..classes-1 unless given.  Not with --bed_names")
    parser.add_argument("--rmout_join", type=int, default=s, metavar="G",
                        help="(addition) with --bed_rmout: consecutive lines of one record and one label at most G bases apart share "
                             "their ID, as RepeatMasker numbers the fragments of one element (every line its own ID unless given)")


def refuse_on_evaluate(args) -> None:
    if getattr(args, "bed_bigbed", False):
        sys.exit("--bed_bigbed belongs to predict, not evaluate")
    if getattr(args, "bed_gff3", False):
        sys.exit("--bed_gff3 belongs to predict, not evaluate")
    if getattr(args, "bed_names", None) is not None:
        sys.exit("--bed_names belongs to predict, not evaluate")
    if (getattr(args, "bed_dir", None) is not None or getattr(args, "bed_min_score", None) is not None
            or getattr(args, "bed_gzip", False) or getattr(args, "bed_index", False)):
        sys.exit("--bed_dir belongs to predict, not evaluate")
    if getattr(args, "bed_rmout", False):
        sys.exit("--bed_rmout belongs to predict, not evaluate or compare")
    if getattr(args, "rmout_repeats", None) is not None or getattr(args, "rmout_join", None) is not None:
        sys.exit("--rmout_repeats and --rmout_join belong to predict, not evaluate or compare")


def plan(args) -> Optional[BedPlan]:
    """--bed_dir and its options, or None without the flag.  Every refusal is made here (sys.exit), before the model is read or
    the GPU is touched."""
    bdir = getattr(args, "bed_dir", None)
    low = getattr(args, "bed_min_score", None)
    gzip, index = bool(getattr(args, "bed_gzip", False)), bool(getattr(args, "bed_index", False))
    bigbed = bool(getattr(args, "bed_bigbed", False))
    gff3, cnames = bool(getattr(args, "bed_gff3", False)), getattr(args, "bed_names", None)
    if gff3 and bdir is None:
        sys.exit("--bed_gff3 needs --bed_dir")
    if gff3 and bigbed:
        sys.exit("--bed_gff3 and --bed_bigbed each write their file instead of the BED text: they do not go together")
    rmout, repeats, join = bool(getattr(args, "bed_rmout", False)), getattr(args, "rmout_repeats", None), getattr(args, "rmout_join", None)
    if cnames is not None and not gff3 and not rmout:
        if getattr(args, "summary_dir", None) is None:
            sys.exit("--bed_names needs --bed_gff3")
        cnames = None                                   # (they name the labels of --summary_dir only)
    if cnames is not None:
        from . import gff, rmout as dgrmout
        cnames = tuple(nm.encode("utf-8", "surrogateescape") for nm in cnames.split(","))
        refusal = dgrmout.names_refusal if rmout and not gff3 else gff.names_refusal
        if refusal(cnames) is not None:
            sys.exit(refusal(cnames))
    if bigbed and bdir is None:
        sys.exit("--bed_bigbed needs --bed_dir")
    if bigbed and (gzip or index):
        sys.exit("--bed_bigbed writes a bigBed file instead of BED text: it does not go with --bed_gzip or --bed_index")
    if gzip and bdir is None:
        sys.exit("--bed_gzip needs --bed_dir")
    if index and not gzip:
        sys.exit("--bed_index needs --bed_gzip")
    if rmout and bdir is None:
        sys.exit("--bed_rmout needs --bed_dir")
    if rmout and (bigbed or gff3):
        sys.exit("--bed_rmout, --bed_gff3 and --bed_bigbed each write their file instead of the BED text: they do not go together")
    if rmout and index:
        sys.exit("--bed_rmout does not go with --bed_index: the listing is blank-separated, and tabix indexes tab-separated columns")
    if repeats is not None:
        if not rmout:
            sys.exit("--rmout_repeats needs --bed_rmout")
        if cnames is not None:
            sys.exit("--rmout_repeats and --bed_names both name the labels of the listing: they do not go together")
        from .rmout import repeats_refusal
        try:
            repeats = tuple(int(tok) for tok in repeats.split(","))
        except ValueError:
            sys.exit(f"--rmout_repeats: {repeats!r} is not a comma-separated list of numbers")
        if repeats_refusal(repeats) is not None:
            sys.exit(repeats_refusal(repeats))
    if join is not None:
        if not rmout:
            sys.exit("--rmout_join needs --bed_rmout")
        if join < 0:
            sys.exit(f"--rmout_join must be 0 or more, not {join}")
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
    from .outfiles import plan_inputs
    paths = plan_inputs("--bed_dir", args.FASTA, lambda f: bed_path(bdir, f, gzip, bigbed, gff3, rmout), "BED files", "BED file")
    level = None
    if gzip or bigbed:
        from .tracks import gzip_level
        level = gzip_level(args, 1)
    from .tracks import index_format
    return BedPlan(bdir, int(low), paths, level, index, bigbed, gff3, cnames, rmout, repeats, -1 if join is None else int(join),
                   index_format=index_format(args))


def from_plan(p: BedPlan, classes: int) -> "Bed":
    """The number of --bed_names checked against the model's class count (sys.exit); with --bed_rmout the number of
    --rmout_repeats as well, and the (repeat, class/family) pair of every label is settled."""
    if p.class_names is not None and len(p.class_names) != classes - 1:
        sys.exit(f"--bed_names gives {len(p.class_names)} names, but the model has {classes - 1} repeat classes "
                 f"(labels 1..{classes - 1})")
    if p.rmout:
        from . import rmout
        if p.class_names is not None:
            pairs = rmout.pairs_of_names(p.class_names)
        elif p.rmout_repeats is not None:
            if len(p.rmout_repeats) != classes - 1:
                sys.exit(f"--rmout_repeats gives {len(p.rmout_repeats)} numbers, but the model has {classes - 1} repeat classes "
                         f"(labels 1..{classes - 1})")
            pairs = rmout.pairs_of_repeats(p.rmout_repeats)
        elif classes - 1 > rmout.MAX_REPEATS:
            sys.exit(f"--bed_rmout: the model has {classes - 1} repeat classes, more than the {rmout.MAX_REPEATS} numbered families "
                     "of parse_rm: name the labels with --bed_names (repeat#class/family)")
        else:
            pairs = rmout.pairs_of_repeats(range(1, classes))
        p = p._replace(rmout_pairs=pairs)
    return Bed(p)


class Bed:
    """--bed_dir as an output of `predict`: every work item's rows come with their scores (with a plan that is on_device: with the
    device's write of them), which go to the input's BedFiles."""
    wants_rows = False

    def __init__(self, p: BedPlan):
        self.plan = p
        self.runner = dict(scores=True, bed=p)          # what is asked of the RecordRunner

    def open(self, filename: str) -> "BedFiles":
        return BedFiles(self.plan, filename)


class _BigBedFile(StagedFile):
    """One `.bb` file: a bigbed.BigBedBuilder (`bb`) on the staged file."""

    def __init__(self, final: str):
        from .bigbed import BigBedBuilder
        super().__init__(final, "w+b")
        try:
            self.bb = BigBedBuilder(self.fh, os.path.dirname(final))
        except BaseException:
            super().abort()
            raise

    def finish(self) -> None:
        self.bb.finish()
        self.fh.close()

    def abort(self) -> None:
        self.bb.close()
        super().abort()


class BedFiles(StagedOutputs):
    """The BED file of one input: a temporary file next to it, renamed by `commit`, removed by `abort` (outfiles.py).  With
    p.gzip_level `write` takes a BedWrite (BGZF members, to an outfiles.BgzfSink, which with p.index builds `<file>.tbi`; with
    p.index_format "csi" it builds `<file>.csi` instead, and the limit below is 2^32).  An
    input that cannot be indexed (a record that ends above 2^29, an empty name, a name that comes back: name_order) gets one
    warning and no index: the `.bed.gz` is what it is without the flag, and a `.tbi` an earlier run left is removed.  With
    p.bigbed the file is a `.bb` with a bigbed.BigBedBuilder on its temporary file and `write` takes a bigbed.BigBedWrite; an
    input a bigBed cannot hold (an empty name, a name two records share, a record that ends above 2^32 - 1) gets one warning and
    no `.bb`: `commit` then removes the temporary file and any `.bb` an earlier run left.  With p.gff3 the file is a `.gff3[.gz]`
    that begins with gff.HEADER (a BGZF member of its own), `write` takes a gff.GffWrite and renders it with the lines written so
    far (`lines`); the names of the index are the escaped seqids of column 1; an input with an empty record name gets one warning
    and no `.gff3`, as a bigBed does.  With p.rmout the file is a `.out[.gz]` that begins with rmout.HEADER (a BGZF member of its
    own), `write` takes an rmout.RmoutWrite and renders it with the IDs used so far (`ids`: joined fragments share one, so the count
    advances by the IDs, not by the lines); an input with a record name that cannot stand in a blank-separated column gets one
    warning and no `.out`."""

    def __init__(self, p: BedPlan, filename: str):
        os.makedirs(p.directory, exist_ok=True)
        self.final, self.min_score, self.bigbed = p.paths[filename], p.min_score, bool(p.bigbed)
        self.gzip = p.gzip_level is not None and not self.bigbed
        self.bb_refused = None
        self.gff3, self.lines = bool(getattr(p, "gff3", False)), 0
        self.rmout, self.ids = bool(getattr(p, "rmout", False)), 0
        preset = ()
        if self.gff3:
            from . import gff
            preset = (gff.PRESET,)
        super().__init__(_LOG, filename, "--bed_index", self.gzip and p.index,
                         [_BigBedFile(self.final) if self.bigbed else BgzfSink(self.final, p.index, *preset, fmt=p.index_format) if self.gzip
                          else StagedFile(self.final)])
        if self.gff3 or self.rmout:
            try:
                self._gff_header(p.gzip_level)
            except BaseException:
                self.abort()
                raise

    def _gff_header(self, level) -> None:
        """gff.HEADER (rmout.HEADER) in front of everything: in a BGZF file a member of its own, which no chunk of the index touches."""
        from . import gff, rmout
        form = rmout if self.rmout else gff
        if self.gzip:
            sink = self.parts[0]
            member = form.header_member(level)
            sink.data.fh.write(member)
            sink.off += len(member)
        else:
            self.parts[0].fh.write(form.HEADER)

    def _rmout(self, w) -> None:
        """The write's part of the listing, or the input's refusal (one warning)."""
        from . import rmout
        if not isinstance(w, rmout.RmoutWrite):
            raise ValueError(f"{self.filename}: a RepeatMasker listing is written from RmoutWrite, not from scores on the host")
        if self.bb_refused is not None:
            return
        for nm in w.names:
            why = rmout.record_name_refusal(nm)
            if why is not None:
                self.bb_refused = why
                _LOG.warning("%s: no RepeatMasker listing is written (--bed_rmout): %s", self.filename, why)
                return
        if w.render is None:
            return
        t = w.render(self.ids)
        self.lines += t.lines
        self.ids += t.ids
        if self.gzip:
            self.append(0, t.data, w.names)
        else:
            self.append(0, t.data)

    def _gff(self, w) -> None:
        """The write's part of the GFF3 file, or the input's refusal (one warning)."""
        from . import gff
        if not isinstance(w, gff.GffWrite):
            raise ValueError(f"{self.filename}: a GFF3 file is written from GffWrite, not from scores on the host")
        if self.bb_refused is not None:
            return
        if any(not nm for nm in w.names):
            self.bb_refused = "a record with an empty name"
            _LOG.warning("%s: no GFF3 file is written (--bed_gff3): %s", self.filename, self.bb_refused)
            return
        seqids = [gff.escape_seqid(nm) for nm in w.names]
        if self.indexed:                                # (the names count in the order even where the write has no line)
            self.no_index(self.name_order(seqids) or w.refused)
        if w.render is None:
            return
        t = w.render(self.lines)
        self.lines += t.lines
        if self.indexed and t.data and t.chunks is None:
            self.no_index("a write came without its index")
        if self.gzip:
            self.append(0, t.data, seqids, t.chunks, t.linear, t.wpref, t.last_end)
        else:
            self.append(0, t.data)

    def _bigbed(self, w) -> None:
        """The write's part of the bigBed, or the input's refusal (one warning)."""
        from .bigbed import BigBedWrite
        if not isinstance(w, BigBedWrite):
            raise ValueError(f"{self.filename}: a bigBed is written from BigBedWrite, not from scores on the host")
        if self.bb_refused is not None:
            return
        why = w.refused
        if why is None:
            why = self.distinct_names(w.names)
        if why is not None:
            self.bb_refused = why
            _LOG.warning("%s: no bigBed file is written (--bed_bigbed): %s", self.filename, why)
            return
        builder = self.parts[0].bb
        if w.chrom0 is not None and w.chrom0 != len(builder.names):
            raise ValueError(f"{self.filename}: a bigBed write of chromId {w.chrom0} arrived as record {len(builder.names)} of the input")
        builder.add(w.names, w.sizes, w)

    def take(self, names: Sequence, batch: bool, rows, scores, texts) -> None:
        self.write(names, batch, rows, scores)

    def commit(self, rows=None, log=None) -> None:
        if self.bb_refused is None:
            return super().commit()
        self.abort()
        for left in [self.final] + ([self.final + ".tbi"] if self.gff3 and self.gzip and self.parts[0].index_wanted else []):
            if os.path.exists(left):
                os.remove(left)

    def write(self, names: Sequence, by_contig: bool, rows, scores) -> None:
        """The lines of one record (by_contig false: names[0]) or of a batch (rows["contig"] indexes the names); `scores` is the
        rows' ROW_SCORE_DTYPE array, or with p.gzip_level the BedWrite the device made of rows and scores, or with p.bigbed its
        bigbed.BigBedWrite."""
        if self.bigbed:
            return self._bigbed(scores)
        if self.gff3:
            return self._gff(scores)
        if self.rmout:
            return self._rmout(scores)
        if not isinstance(scores, BedWrite):
            if self.gzip:
                raise ValueError(f"{self.filename}: a BGZF BED is written from BedWrite, not from scores on the host")
            if len(rows):
                self.append(0, format_rows(names, by_contig, rows, scores, self.min_score))
            return
        w = scores
        if not self.gzip:
            raise ValueError(f"{self.filename}: BGZF members for a plain BED")
        if self.indexed:                                # (the names count in the order even where the write has no members)
            why = self.name_order(w.names) or w.refused
            if why is None and w.members and w.chunks is None:
                why = "a write came without its index"
            self.no_index(why)
        self.append(0, w.members, w.names, w.chunks, w.linear, w.wpref, w.last_end)


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


def reference_index_parts(names: Sequence, by_contig: bool, rows, scores, min_score: int, rec_end: Sequence[int], depth: int = 5):
    """What dgrp_bed_index_batch states about the text `reference_lines` gives for the same arguments, in Python integers:
    -> (chunks tabix.CHUNK_DTYPE, linear int64 [windows of all records], wpref int64 [records + 1], last_end int64 [records]).
    A chunk is a maximal run of consecutive emitted lines of one record with one bin; linear[wpref[r] + w] is the text offset of
    the first emitted line of record r, in file order, whose end is greater than w << 14 (the running maximum of the ends), or
    -1; last_end[r] the end of the record's last emitted line, 0 without one.  With another depth: what dgrp_bed_csi_batch
    states, the bins those of tabix.csi_reg2bin at that depth."""
    from .tabix import CHUNK_DTYPE, MIN_SHIFT, csi_reg2bin, window_prefix
    nrec = len(rec_end)
    wpref = window_prefix(rec_end, depth)
    linear = np.full(int(wpref[-1]), -1, np.int64)
    filled = [0] * nrec
    last_end = np.zeros(nrec, np.int64)
    chunks, u = [], 0
    for k in range(len(rows)):
        line = reference_lines(names, by_contig, rows[k:k + 1], scores[k:k + 1], min_score)
        if not line:
            continue
        r = int(rows[k]["contig"]) if by_contig else 0
        start, end = int(rows[k]["start"]), int(rows[k]["end"])
        b = csi_reg2bin(start, end, depth)
        if chunks and chunks[-1][2] == r and chunks[-1][3] == b:
            chunks[-1][1] = u + len(line)
        else:
            chunks.append([u, u + len(line), r, b])
        top = ((end - 1) >> MIN_SHIFT) + 1
        if top > filled[r]:
            linear[wpref[r] + filled[r]:wpref[r] + top] = u
            filled[r] = top
        last_end[r] = end
        u += len(line)
    out = np.zeros(len(chunks), CHUNK_DTYPE)
    for i, c in enumerate(chunks):
        out[i] = tuple(c)
    return out, linear, wpref, last_end
