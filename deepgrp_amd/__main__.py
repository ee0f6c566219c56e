#!/usr/bin/env python3
"""deepgrp_amd command line -- drop-in for `deepgrp [flags] predict <model.hdf5> <FASTA>...`
(deepgrp/__main__.py:86-297 of the reference): same flags and defaults, same 5-column TSV.

Differences, all additive:
  * the README's short form `deepgrp <modelfile> <fastafile>` is accepted too;
  * `--xla` and `--threads` are accepted and ignored (there is no TensorFlow here);
  * under torchrun (WORLD_SIZE > 1) the records of all input files are sharded by contig over
    the GPUs and rank 0 writes the rows in input order;
  * `predict --mask_dir DIR [--mask soft|hard] [--mask_classes 1,3]` also writes a masked copy of every input FASTA file
    (deepgrp_amd/masking.py); with --mask_twobit the copy is a UCSC .2bit file instead (soft mask = mask blocks, hard mask = N
    blocks; tables and packed bases built on the GPU, deepgrp_amd/twobit.py);
  * `predict --track_dir DIR [--track_classes 1,3] [--track_digits D] [--track_bin B] [--track_gzip]` also writes the per-base class
    probabilities as one bedGraph file per input and class (deepgrp_amd/tracks.py), with --track_gzip as BGZF deflated on the GPU
    (`--gzip_level {0,1}`: literals only or with matches, for --mask_gzip as well) and with --track_index a tabix index beside
    every BGZF track (deepgrp_amd/tabix.py); with --track_bigwig the tracks are bigWig files instead (`.bw`, deepgrp_amd/bigwig.py:
    binary sections and zoom levels written and deflated on the GPU);
  * `predict --bed_dir DIR [--bed_min_score S]` also writes the predicted repeats of every input as a scored BED file: per row the
    mean and the smallest probability of its class and the share of its bases that carry it, summed on the GPU (deepgrp_amd/bed.py);
    with --bed_gzip the file is BGZF (`.bed.gz`), its lines written and deflated on the GPU, and with --bed_index a tabix index
    (`.bed.gz.tbi`) is built there beside it; with --bed_bigbed the file is a bigBed instead (`.bb`, deepgrp_amd/bigbed.py: binary
    items with 32-bit coordinates, an R-tree and coverage zoom levels, written and deflated on the GPU); with --bed_gff3 the file
    is GFF3 instead (`.gff3`, deepgrp_amd/gff.py: one `repeat_region` feature per row with the BED's figures as attributes, written
    on the GPU; `--bed_names A,B,...` names the labels; `.gff3.gz` and `.gff3.gz.tbi` with --bed_gzip and --bed_index);
    with --bed_rmout the file is a RepeatMasker listing instead (`.out`, `.out.gz` with --bed_gzip; deepgrp_amd/rmout.py: the
    format `evaluate`, `compare`, `train` and `parse_rm` read, written on the GPU; `--rmout_repeats N,N,...` or `--bed_names
    repeat#class/family,...` name the labels, `--rmout_join G` gives the fragments of one element one ID);
  * `predict --seq_dir DIR [--seq_classes 1,3] [--seq_flank N] [--seq_width W]` also writes the sequences of the predicted repeats
    of every input as FASTA, DIR/<basename>.repeats.fa: one record `>NAME:A-B class<label>` per TSV row, gathered on the GPU
    (deepgrp_amd/repeatseq.py); with --seq_gzip as BGZF (`.repeats.fa.gz`), with --seq_fai a `.fai` index beside it;
  * `predict --summary_dir DIR [--summary_bin N] [--bed_names A,B,...]` also writes the repeat content of every input,
    DIR/<basename>.summary.tsv: per record and label the rows, the bases by kind and case, minimum, maximum and N50 of the row
    lengths, the share of the record, GC and the agreement with the input's own soft mask, counted on the GPU
    (deepgrp_amd/summary.py); with --summary_bin also DIR/<basename>.density.tsv, the bases per label in bins of N positions;
  * `evaluate <model> <annotation> <FASTA>...` scores predict's rows against a repeat annotation (deepgrp_amd/evaluation.py);
  * the annotation of `evaluate`, and the bedfile of `train` on sequence files, may be RepeatMasker's own output (`genome.fa.out`,
    `.out.gz`, UCSC `rmsk.txt.gz`; `--annotation_format auto|table|repeatmasker`): it is parsed on the GPU into what the table of
    `parse_rm` holds (deepgrp_amd/annotation.py); `optimize` and `train` on .npz files read the table only;
  * `evaluate --strata PREFIX` also writes recall by divergence bin and element length, PREFIX.strata.tsv and
    PREFIX.strata.bases.tsv, from the listing's divergence column and counts made on the GPU (deepgrp_amd/strata.py);
  * `evaluate --offtarget PREFIX` also writes what the predicted repeats lie on, PREFIX.offtarget.tsv (predicted label by modelled
    class, RepeatMasker class/family or nothing, for all bases and for the unsupported rows) and PREFIX.offtarget.rows.tsv, from
    every row of the listing and counts made on the GPU (deepgrp_amd/offtarget.py);
  * `evaluate --boundaries PREFIX` also writes how well the found elements are delimited, PREFIX.boundaries.tsv (the offset of
    either edge, annotation rows against the predicted labels and predicted rows against the truth) and PREFIX.fragments.tsv (the
    runs under a row), from counts made on the GPU (deepgrp_amd/boundaries.py);
  * `compare <predicted> <annotation> <FASTA>... [--classes C]` gives `evaluate`'s report, and --strata, --offtarget and
    --boundaries, for rows that are already on disk -- a prediction TSV, a table `contig begin end number` or a RepeatMasker
    listing -- without a model: the files are parsed on the GPU and the rows flattened to one label per base first
    (deepgrp_amd/compare.py);
  * PREDICTED of `compare` and the annotation of `evaluate` and `compare` may be GFF3 (`--predicted_format gff3`,
    `--annotation_format gff3`, or a first line `##gff-version 3`), `predict --bed_gff3`'s own file included: parsed on the GPU, the
    label of a feature looked up by name (`--predicted_names`, `--annotation_names`, `--gff_key`, `--gff_by_type`;
    deepgrp_amd/gffin.py); `train` and `optimize` refuse it by name;
  * a FASTA file may be gzip-compressed (recognised by its magic bytes); BGZF files are inflated on the GPU (deepgrp_amd/gz.py);
  * a FASTA file may also be a UCSC .2bit file (recognised by its signature): its packed bases are unpacked on the GPU and every
    command gives what it gives for the FASTA text of the file (deepgrp_amd/twobit.py); one process, or --split_contigs;
  * `train <parameter.toml> <trainfile.npz> <validfile.npz> <bedfile>` trains a GRU model on the GPU (deepgrp_amd/training.py:
    forward, backward through time and the optimizer are HIP kernels) and writes a Keras HDF5 file `predict` loads; `--seed N`
    (an addition) seeds the initial weights, the sampler and the dropout masks.  No TensorBoard output.  Both files may instead be
    sequence files as `predict` takes them (FASTA, gzip, BGZF, .2bit; `--train_contigs a,b` / `--valid_contigs c` pick records by the
    first word of their header): truth and sampler sets are then built on the GPU, and one record trains to the bytes of its .npz;
  * `optimize <space.toml> <parameter.toml> <trainfile.npz> <validfile.npz> <bedfile>` runs the hyper-parameter search of
    deepgrp/optimization.py as seeded random search (deepgrp_amd/optimization.py), `--cohort` trials trained side by side.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from typing import Iterator, List, TextIO, Tuple

import numpy as np

from . import bed, masking, repeatseq, summary, tracks
from .outfiles import class_list

logging.basicConfig()
_LOG = logging.getLogger(__name__)

DEFAULT_COHORT = 8                   # optimize --cohort: the job count with the lowest measured time per job

# The optional outputs of `predict`, each a module with add_options, refuse_on_evaluate, plan and from_plan, in the
# order in which their plans are made (and `evaluate` sends their flags back), in which --help lists them, in which the plans meet
# the model's class count, and in which the files of an input are committed.
_OUTPUTS = (bed, masking, repeatseq, summary, tracks)
_HELP_ORDER = (masking, tracks, bed, repeatseq, summary)
_BIND_ORDER = (tracks, repeatseq, masking, bed, summary)
_COMMIT_ORDER = (tracks, bed, masking, repeatseq, summary)


def _read_multi_fasta(filestream: TextIO) -> Iterator[Tuple[str, str]]:
    """Reads a multi FASTA file (deepgrp/__main__.py:20-43): header = text after '>', sequence
    lines upper-cased and joined; a record without header is dropped; a blank line raises
    IndexError exactly like `line[0]` does in the reference.  (The loop itself: fasta.LineLoop.)"""
    from .fasta import read_multi_fasta_lines
    _LOG.debug("Reading FASTA file.")
    yield from read_multi_fasta_lines(filestream)


def _predict(dnasequence: str, model, options, step_size: int, use_mss: bool) -> Tuple[np.ndarray, int]:
    """Runs a prediction for one sequence (deepgrp/__main__.py:46-83): returns the label per base
    (int64, after MSS or the softmax path) and the number of leading N's."""
    from .pipeline import ContigPipeline, upload_sequence
    _LOG.debug("One hot encoding sequence.")
    start_pos, d_idx = upload_sequence(dnasequence.encode("utf-8"))
    _LOG.debug("Start prediction.")
    pipe = ContigPipeline(model, step_size, options.batch_size, options.min_mss_len, options.xdrop_len, use_mss)
    merged = pipe.merged(d_idx)
    _LOG.debug("Finish prediction.")
    if use_mss:
        _LOG.debug("Applying MSS.")
    labels = pipe.labels(merged)
    return labels.cpu().numpy().astype(np.int64), start_pos


def _records_of(filename):
    """(header, record) pairs of one input as `predict` reads it: a FASTA file (device ingest), '-' or another stream (the
    reference's line loop), or a one-hot `<name>.gz.npz`."""
    import torch
    from .fasta import DeviceRecord, read_multi_fasta_device
    if filename.endswith(".npz") and os.path.isfile(filename):
        # (addition) the one-hot `<fasta>.gz.npz` that `preprocess_sequence` writes for training
        # (deepgrp/_scripts/preprocess_sequence.py:71-78), as an alternative input: ONE record, named after the file
        # (the format keeps no header); same stripping of leading/trailing N as one_hot_encode_dna_sequence
        from .preprocessing import load_onehot_npz
        fwd = load_onehot_npz(filename)
        if fwd.size and not (np.isin(fwd, (0, 1)).all() and (fwd.sum(axis=0) == 1).all()):
            raise ValueError(f"{filename}: `fwd` is not one-hot")
        idx = fwd.argmax(axis=0).astype(np.uint8)
        header = os.path.basename(filename)[:-len(".npz")]
        keep = np.flatnonzero(idx != 4)
        if idx.size == 0:
            return
        if keep.size == 0:
            yield header, DeviceRecord(int(idx.size), None, -int(idx.size))        # all N: the reference raises (sequence.pyx:32)
            return
        st, en = int(keep[0]), int(keep[-1]) + 1
        d_idx = torch.from_numpy(np.ascontiguousarray(idx[st:en])).to(torch.device("cuda", torch.cuda.current_device()))
        yield header, DeviceRecord(st, d_idx, en - st)
        return
    if filename == "-" or not os.path.isfile(filename):
        filestream = sys.stdin if filename == "-" else open(filename, "r")
        try:
            yield from _read_multi_fasta(filestream)
        finally:
            if filename != "-":
                filestream.close()
    else:
        yield from read_multi_fasta_device(filename)


class _RowsByRecord:
    """The rows of one input file in record order, `contig` = the record's ordinal in the file (masking.mask_fasta's input)."""

    def __init__(self):
        self.parts, self.records = [], 0

    def add(self, rows, nrec: int) -> None:
        """`nrec` records' rows: one record (contig ignored) or a batch (contig = index in the batch)."""
        rows = np.array(rows, copy=True)
        if nrec == 1:
            rows["contig"] = self.records
        else:
            rows["contig"] += self.records
        self.parts.append(rows)
        self.records += nrec

    def rows(self):
        from .pipeline import SEGMENT_DTYPE
        return np.concatenate(self.parts) if self.parts else np.zeros(0, SEGMENT_DTYPE)


class _Stages:
    """predict -vv: the stage callback of RecordRunner.run_record for one record -- a device sync and a clock around every stage,
    and the reference's debug lines (deepgrp/__main__.py:69-79), the stage's milliseconds in those of the tracks and the scores."""

    def __init__(self, header: str, use_mss: bool):
        self.header, self.use_mss, self.bases, self.ms, self.t = header, use_mss, 0, {}, 0.0

    def __call__(self, what: str, done: bool, bases: int = 0) -> None:
        import time

        import torch
        if not done:
            self.t = time.perf_counter()
            if what == "encode":
                _LOG.debug("One hot encoding sequence.")
            elif what == "forward":
                _LOG.debug("Start prediction.")
            elif what == "labels" and self.use_mss:
                _LOG.debug("Applying MSS.")
            return
        torch.cuda.synchronize()
        self.ms[what] = (time.perf_counter() - self.t) * 1e3
        if what == "encode":
            self.bases = bases
        elif what == "forward":
            _LOG.debug("Finish prediction.")
        elif what == "tracks":
            _LOG.debug("%s: probability tracks %.2f ms", self.header, self.ms[what])
        elif what == "scores":
            _LOG.debug("%s: row scores %.2f ms", self.header, self.ms[what])

    def close(self, rows) -> int:
        """The record's closing line (none for a record without a base).  -> its bases"""
        ms, n = self.ms, self.bases
        if n:
            _LOG.debug("%s: %d bases; encode %.2f ms, forward + merge %.2f ms (%.1f Mbp/s), %s %.2f ms, segments + read-back %.2f ms, %d rows",
                       self.header, n, ms["encode"], ms["forward"], n / max(ms["forward"], 1e-6) / 1e3,
                       "scores + MSS + vote" if self.use_mss else "softmax", ms["labels"], ms["segments"], len(rows))
        return n


def _gff_options(parser, sides) -> None:
    """The flags of the format `gff3` (deepgrp_amd/gffin.py): the names of the labels per side, and where the label string stands."""
    for side in sides:
        parser.add_argument(f"--{side}_names", type=str, default=None, metavar="NAMES",
                            help=f"with --{side}_format gff3: what the labels 1..C-1 are called in the file, one entry per label "
                                 "separated by commas, an entry one or more alternatives joined by '|' (`LTR|ERV1|ERVK,LINE|L1,Alu,"
                                 "Satellite`); default: class1,class2,... as `predict --bed_gff3` writes without --bed_names")
    parser.add_argument("--gff_key", type=str, default=None, metavar="TAG",
                        help="gff3: the attribute of column 9 whose value is the label's name; without this flag, Name")
    parser.add_argument("--gff_by_type", action="store_true", help="gff3: the label's name is column 3, the type; excludes --gff_key")


def _gff_plan(args, classes: int, sides):
    """gffin.plan with the refusal as an exit: ({names flag: names}, key)."""
    from . import gffin
    try:
        return gffin.plan(args, classes, sides)
    except ValueError as e:
        sys.exit(str(e))


def _gff_resolved(args, flag: str, fmt_flag: str, resolved: str) -> None:
    from . import gffin
    try:
        gffin.refuse_names(flag, getattr(args, flag.lstrip("-")) is not None, fmt_flag, resolved)
    except ValueError as e:
        sys.exit(str(e))


def _refuse_gff3(command: str, path) -> str:
    return (f"{command}: {path} is GFF3, which `evaluate` and `compare` read (--annotation_format gff3); the truth of {command} is the "
            "table of parse_rm or a RepeatMasker listing")


class CommandLineParser:
    """Commandline parser (deepgrp/__main__.py:86-250)."""

    def __init__(self, **kwargs):
        kwargs.setdefault("prog", "deepgrp")
        kwargs.setdefault("formatter_class", argparse.ArgumentDefaultsHelpFormatter)
        kwargs.setdefault("description", "DeepGRP - Prediction of repetitive elements (MI355X / HIP)")
        self.parser = argparse.ArgumentParser(**kwargs)
        self.args = None
        self.threads = 1
        self.xla = False
        self.verbose = 0
        subparsers = self.parser.add_subparsers(help="sub-command help", dest="command")
        self.parser.add_argument("--batch_size", "-b", type=int, default=256,
                                 help="Batch size of the reference's TensorFlow loop; only its placement arithmetic matters here")
        self.parser.add_argument("--step_size", "-s", type=int, default=50, help="Window step size")
        self.parser.add_argument("--xdrop_length", "-x", type=int, default=50,
                                 help="XDrop parameter for MSS algorithm, ignored if --no_use_mss, disabled with values<0")
        self.parser.add_argument("--min_mss_length", "-l", type=int, default=50,
                                 help="Minimal length of maximum scoring segments, ignored if --no_use_mss")
        self.parser.add_argument("--threads", "-t", type=int, default=1, help="Accepted for compatibility (ignored)")
        self.parser.add_argument("--xla", action="store_true", help="Accepted for compatibility (ignored)")
        self.parser.add_argument("-v", "--verbose", action="count", default=0, help="Increase verbosity")
        for output in _HELP_ORDER:
            output.add_options(self.parser)
        train = subparsers.add_parser(name="train", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                      description="Train a deepgrp model (GRU) on the GPU")
        train.add_argument("parameter", type=str)
        train.add_argument("trainfile", type=str)
        train.add_argument("validfile", type=str)
        train.add_argument("bedfile", type=str)
        train.add_argument("--logdir", type=str, default=".")
        train.add_argument("--modelfile", type=str, default="model.hdf5")
        train.add_argument("--seed", type=int, default=None,
                           help="(addition) seed of the initial weights, the sampler and the dropout masks: the same seed "
                                "writes the same model file, byte for byte")
        train.add_argument("--train_contigs", type=str, default=None,
                           help="(addition) with a sequence file (FASTA, gzip, BGZF, .2bit) as trainfile: the records to train on, by "
                                "the first word of their header, comma separated (default: every record, in file order)")
        train.add_argument("--valid_contigs", type=str, default=None, help="(addition) the same for validfile")
        train.add_argument("--annotation_format", choices=("auto", "table", "repeatmasker", "gff3"), default="auto",
                           help="(addition) what bedfile is: `table` = the six columns parse_rm writes, `repeatmasker` = RepeatMasker's "
                                "own listing (`.out`, `.out.gz`) or UCSC's rmsk table, parsed on the GPU (sequence files only); `auto` "
                                "looks at the first lines")
        optimize = subparsers.add_parser(name="optimize", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                         description="(addition) hyper-parameter search (deepgrp/optimization.py): seeded random "
                                                     "search over the [space] table of a TOML file, trials trained side by side on "
                                                     "the GPU, results in <project_root_dir>/results.json")
        optimize.add_argument("space", type=str, help='TOML file with a [space] table: gru_units = ["qnormal", 34, 5, 2]; kinds: '
                                                      "uniform, quniform, normal, qnormal, loguniform, lognormal, choice")
        optimize.add_argument("parameter", type=str)
        optimize.add_argument("trainfile", type=str)
        optimize.add_argument("validfile", type=str)
        optimize.add_argument("bedfile", type=str)
        optimize.add_argument("--annotation_format", choices=("auto", "table", "repeatmasker", "gff3"), default="auto",
                              help="what bedfile is; only `table` (the six columns parse_rm writes) is read here: RepeatMasker "
                                   "output is refused by name")
        optimize.add_argument("--max_evals", type=int, default=20, help="trials to add to results.json")
        optimize.add_argument("--cohort", type=int, default=DEFAULT_COHORT,
                              help="trials trained side by side, 1..64 (more than 8 run in slices of 8 per step)")
        optimize.add_argument("--seed", type=int, default=None, help="seed of the search: trial t of a seed is the same trial "
                                                                     "whatever --cohort is and wherever a run was resumed")
        optimize.add_argument("--project_root_dir", type=str, default=None,
                              help="where results.json and tf_logs/ go (default: project_root_dir of the parameter file)")
        predict = subparsers.add_parser(name="predict", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                        description="predict using a deepgrp model")
        predict.add_argument("model", type=str, help="Keras model in HDF5 format")
        predict.add_argument("FASTA", nargs="+", type=str, help="Fasta input files ('-' = stdin); a `<fasta>.gz.npz` written by "
                                                                "`preprocess_sequence` is accepted too (one record per file)")
        predict.add_argument("--output", type=str, default="-", help="Output filename")
        predict.add_argument("--no_use_mss", "-m", action="store_true", help="Disable maximum scoring segment algorithm")
        verify = subparsers.add_parser(name="verify", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                       description="(addition) measure how far the fp16-operand fused kernel is from a plain "
                                                   "fp32 evaluation of the SAME model on the device, on windows of the given "
                                                   "FASTA files (or a random sequence): the accuracy the 1e-3 bound is about")
        verify.add_argument("model", type=str, help="Keras model in HDF5 format")
        verify.add_argument("FASTA", nargs="*", type=str, help="Fasta input files; none = a random ACGT sequence")
        verify.add_argument("--windows", type=int, default=256, help="windows to compare per record (spread evenly)")
        predict.add_argument("--fast", action="store_true",
                             help="(addition) fp16-operand fused kernels: 2-2.5x the default's speed, class probabilities within 1e-3 of "
                                  "fp32 except on ill-conditioned windows (measure with `verify`); the default is fp32-grade (split "
                                  "operands, 1e-5) for every model")
        predict.add_argument("--precise", action="store_true",
                             help="(addition, kept for compatibility) the default: since every model has an fp32-grade fused kernel "
                                  "this flag selects nothing else")
        predict.add_argument("--split_contigs", action="store_true",
                             help="multi-GPU only: spread the windows of EVERY record over all GPUs (for a few huge "
                                  "records) instead of sharding whole records")
        for output in _HELP_ORDER:
            output.add_options(predict)
        evaluate = subparsers.add_parser(
            name="evaluate", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
            description="(addition) score the rows `predict` writes with the same flags against a repeat annotation: per-class "
                        "confusion matrix, TPR, PPV, F1 and MCC over the bases from the first to the last non-N base of every "
                        "record, and element counts.  Truth of a base: the smallest kept repeat number of the annotation rows that "
                        "cover it (0: none).  Unlike the reference's HPO objective (deepgrp/optimization.py:52-69) the last non-N "
                        "base is evaluated too (its drop_start_end_n drops it) and no extra filter_segments pass runs: the TSV "
                        "users get is what is measured.")
        evaluate.add_argument("model", type=str, help="Keras model in HDF5 format")
        evaluate.add_argument("annotation", type=str, help="table as parse_rm writes it: contig, 0-based begin, exclusive end, "
                                                           "repeat number, further columns ignored; or RepeatMasker's own listing "
                                                           "(`.out`, UCSC rmsk; plain, gzip or BGZF), parsed on the GPU")
        evaluate.add_argument("--annotation_format", choices=("auto", "table", "repeatmasker", "gff3"), default="auto",
                              help="what the annotation is; `auto` looks at its first lines.  A RepeatMasker listing gives what the "
                                   "table parse_rm writes from it gives; it is read after the device is opened, the table before")
        _gff_options(evaluate, ("annotation",))
        evaluate.add_argument("FASTA", nargs="+", type=str, help="inputs as for predict: FASTA files, '-', `<name>.gz.npz`; a "
                                                                 "record is matched to the annotation by the first word of its "
                                                                 "header (.npz: the file name up to the first '.')")
        evaluate.add_argument("--no_use_mss", "-m", action="store_true", help="Disable maximum scoring segment algorithm")
        evaluate.add_argument("--fast", action="store_true", help="fp16-operand fused kernels, as for predict")
        evaluate.add_argument("--repeats", type=class_list, default=None,
                              help="comma-separated repeat numbers to keep from the annotation (default: 1..C-1 of the model)")
        evaluate.add_argument("--min_overlap", type=float, default=0.5,
                              help="an element is found (a predicted row supported) when at least this fraction of its bases "
                                   "carries its class on the other side, in (0, 1]")
        evaluate.add_argument("--output", type=str, default="-", help="TSV report ('-' = standard output)")
        evaluate.add_argument("--json", type=str, default=None, help="also write every figure as JSON here")
        evaluate.add_argument("--curves", type=str, default=None, metavar="PREFIX",
                              help="also write threshold curves: PREFIX.bases.tsv (per class and probability threshold k/bins: TP, FP, "
                                   "FN, TN, TPR, FPR, PPV, F1 of calling a base that class when its probability reaches the threshold) "
                                   "and PREFIX.rows.tsv (per class and --bed_min_score 0..1000: the predicted rows kept, those the "
                                   "annotation supports, their ratio); --json gains the key `curves` (AUROC, average precision, best F1)")
        evaluate.add_argument("--curve_bins", type=int, default=None,
                              help="probability bins of --curves, 2..4096 (default with --curves: 1000)")
        evaluate.add_argument("--curve_elements", action="store_true",
                              help="with --curves: also PREFIX.elements.tsv (per class and --bed_min_score 0..1000: the annotated "
                                   "elements still found by the --min_overlap rule once the rows below that score are gone, recall, "
                                   "the precision of PREFIX.rows.tsv and F1); the JSON's `curves` gains `elements` (recall at 0, the "
                                   "best element-level F1 and the lowest score that reaches it)")
        evaluate.add_argument("--strata", type=str, default=None, metavar="PREFIX",
                              help="also write recall by divergence and element length: PREFIX.strata.tsv (per class and stratum: "
                                   "elements, found, recall, and the bases and hits of the elements) and PREFIX.strata.bases.tsv (per "
                                   "class, stratum and threshold: the bases whose winning element lies in the stratum); the divergence "
                                   "comes from a RepeatMasker listing (a table has none: everything is NA); --json gains the key `strata`")
        evaluate.add_argument("--offtarget", type=str, default=None, metavar="PREFIX",
                              help="also write what the predicted repeats lie on: PREFIX.offtarget.tsv (per predicted label the bases "
                                   "under each modelled class, each other RepeatMasker class/family and nothing, for all bases and "
                                   "for the unsupported predicted rows) and PREFIX.offtarget.rows.tsv (per class its unsupported rows "
                                   "by what most of their bases lie on); needs a RepeatMasker listing as annotation; --json gains the "
                                   "key `offtarget`")
        evaluate.add_argument("--offtarget_by", choices=("family", "class"), default=None,
                              help="names of PREFIX.offtarget.tsv: the class/family token (default with --offtarget) or its part in "
                                   "front of the first '/'")
        evaluate.add_argument("--boundaries", type=str, default=None, metavar="PREFIX",
                              help="also write how well the found elements are delimited: PREFIX.boundaries.tsv (per view, class and "
                                   "side the offset between the row's edge and the other track's run, in bases) and "
                                   "PREFIX.fragments.tsv (per view and class the rows by the runs under them); view `element` takes "
                                   "the annotation rows against the predicted labels, view `row` the predicted rows against the "
                                   "truth; --json gains the key `boundaries`")
        evaluate.add_argument("--boundary_max", type=int, default=None, metavar="W",
                              help="largest offset of --boundaries that is told apart, 1..4096 bases (default with --boundaries: 200)")
        evaluate.add_argument("--boundary_join", type=int, default=None, metavar="G",
                              help="element view of --boundaries: annotation rows of one record and class at most G >= 0 bases apart "
                                   "(abutting and overlapping rows included) count as one element (default: the rows as they are)")
        evaluate.add_argument("--strata_div", type=str, default=None,
                              help="divergence edges of --strata in percent, ascending, 1..15 of them, one decimal allowed "
                                   "(default with --strata: 5,10,15,20,25,30)")
        evaluate.add_argument("--strata_len", type=str, default=None,
                              help="length edges of --strata in bases, ascending, 1..15 of them (default with --strata: 100,300,1000,3000)")
        evaluate.add_argument("--strata_bins", type=int, default=None,
                              help="probability bins of PREFIX.strata.bases.tsv, 2..1000 (default with --strata: 100)")
        compare = subparsers.add_parser(
            name="compare", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
            description="(addition) `evaluate`'s report for rows that are already on disk: the TSV `predict` (or the reference) "
                        "wrote, another tool's calls as a table `contig begin end number`, or a RepeatMasker listing, against a "
                        "repeat annotation.  No model is read and no forward pass runs; the inputs give the records, their names and "
                        "the evaluated span of each.  The predicted rows of a record are flattened first: painted onto its span "
                        "(the smallest label wins) and read back as the runs `predict` would have written.")
        compare.add_argument("predicted", type=str, help="the rows to score: a prediction TSV, a table or a RepeatMasker listing "
                                                         "(plain, gzip or BGZF), parsed on the GPU")
        compare.add_argument("annotation", type=str, help="the annotation, as for evaluate")
        compare.add_argument("FASTA", nargs="+", type=str, help="inputs as for predict and evaluate")
        compare.add_argument("--classes", type=int, default=5, help="classes of the labels, background included, 2..64")
        compare.add_argument("--repeats", type=class_list, default=None,
                             help="comma-separated repeat numbers to keep from the annotation (default: 1..classes-1)")
        compare.add_argument("--predicted_format", choices=("auto", "tsv", "table", "repeatmasker", "gff3"), default="auto",
                             help="what PREDICTED is; `auto` looks at its first lines: tsv, then gff3 (a first line that begins with "
                                  "`##gff-version 3`), then repeatmasker, else table")
        compare.add_argument("--annotation_format", choices=("auto", "table", "repeatmasker", "gff3"), default="auto",
                             help="what the annotation is; `auto` looks at its first lines")
        _gff_options(compare, ("predicted", "annotation"))
        compare.add_argument("--min_overlap", type=float, default=0.5, help="as for evaluate, in (0, 1]")
        compare.add_argument("--output", type=str, default="-", help="TSV report ('-' = standard output)")
        compare.add_argument("--json", type=str, default=None, help="also write every figure as JSON here")
        compare.add_argument("--curves", type=str, default=None, metavar="PREFIX", help="refused: the curves need probabilities and scores")
        compare.add_argument("--curve_bins", type=int, default=None, help="refused, as --curves")
        compare.add_argument("--curve_elements", action="store_true", help="refused, as --curves")
        compare.add_argument("--strata", type=str, default=None, metavar="PREFIX",
                             help="as for evaluate, but PREFIX.strata.tsv alone: PREFIX.strata.bases.tsv needs probabilities")
        compare.add_argument("--strata_div", type=str, default=None, help="as for evaluate")
        compare.add_argument("--strata_len", type=str, default=None, help="as for evaluate")
        compare.add_argument("--strata_bins", type=int, default=None, help="accepted for evaluate's sake; no file of compare reads it")
        compare.add_argument("--offtarget", type=str, default=None, metavar="PREFIX", help="as for evaluate")
        compare.add_argument("--offtarget_by", choices=("family", "class"), default=None, help="as for evaluate")
        compare.add_argument("--boundaries", type=str, default=None, metavar="PREFIX", help="as for evaluate")
        compare.add_argument("--boundary_max", type=int, default=None, metavar="W", help="as for evaluate")
        compare.add_argument("--boundary_join", type=int, default=None, metavar="G", help="as for evaluate")

    def parse_args(self, argv=None) -> "CommandLineParser":
        argv = list(sys.argv[1:] if argv is None else argv)
        # README form `deepgrp <modelfile> <fastafile>`: insert the sub-command before the first positional
        if not any(a in ("predict", "train", "verify", "evaluate", "optimize", "compare") for a in argv):
            takes_value = {"--batch_size", "-b", "--step_size", "-s", "--xdrop_length", "-x", "--min_mss_length", "-l",
                           "--threads", "-t", "--mask_dir", "--mask", "--mask_classes", "--track_dir", "--track_classes",
                           "--track_digits", "--track_bin", "--gzip_level", "--bed_dir", "--bed_min_score", "--bed_names",
                           "--rmout_repeats", "--rmout_join", "--index_format",
                           "--seq_dir", "--seq_classes", "--seq_flank", "--seq_width", "--summary_dir", "--summary_bin"}
            i = 0
            while i < len(argv):
                if argv[i] in takes_value:
                    i += 2
                elif argv[i].startswith("-") and argv[i] != "-":
                    i += 1
                else:
                    break
            if i < len(argv):
                argv.insert(i, "predict")
        args = self.parser.parse_args(argv)
        if args.command is None:
            self.parser.error("a sub-command (predict) is required")
        self.threads, self.verbose, self.xla, self.args = args.threads, args.verbose, args.xla, args
        return self

    def setup_tensorflow(self) -> "CommandLineParser":
        """Kept for call-chain compatibility (deepgrp/__main__.py:221-233); nothing to set up."""
        return self

    def set_logging(self) -> "CommandLineParser":
        levels = [logging.WARNING, logging.INFO, logging.DEBUG]
        _LOG.setLevel(levels[min(len(levels) - 1, self.verbose)])
        return self

    def run(self):
        from . import model as dgmodel
        options = dgmodel.Options(min_mss_len=self.args.min_mss_length, batch_size=self.args.batch_size,
                                  xdrop_len=self.args.xdrop_length)
        getattr(self, self.args.command)(self.args, options)

    @staticmethod
    def predict(args: argparse.Namespace, options) -> None:
        """Predict with deepgrp (deepgrp/__main__.py:252-297)."""
        tracks.check_gzip_flags(args)                           # refusals come before anything runs
        plans = {m: m.plan(args) for m in _OUTPUTS}
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            from .gz import compressed_inputs
            packed = compressed_inputs(args.FASTA)
            if packed:
                sys.exit(f"{packed[0]} is gzip-compressed: compressed input cannot be sharded over ranks (WORLD_SIZE > 1); "
                         "decompress it or run in one process")
            from .twobit import twobit_inputs
            packed = twobit_inputs(args.FASTA)
            if packed and not getattr(args, "split_contigs", False):
                sys.exit(f"{packed[0]} is a 2bit file: the ranks share a file out by byte ranges of FASTA text, and a 2bit file has "
                         "none (WORLD_SIZE > 1); convert it to FASTA, pass --split_contigs or run in one process")
        # host work first: the model file is read once, and every plan meets its class count before the GPU is touched
        from . import model as dgmodel
        _LOG.debug("Loading model %s!", args.model)
        weights = dgmodel.read_keras_hdf5(args.model)
        classes = int(weights["ff_kernel"].shape[-1])
        bound = {m: m.from_plan(plans[m], classes) for m in _BIND_ORDER if plans[m] is not None}
        outputs = [bound[m] for m in _COMMIT_ORDER if m in bound]
        masks = bound.get(masking)                              # the one output several ranks can write
        import torch
        import torch.distributed as dist
        from .pipeline import SEGMENT_DTYPE, record_indices
        from .runner import RecordRunner, rows_text

        world = int(os.environ.get("WORLD_SIZE", "1"))
        rank = int(os.environ.get("RANK", "0"))
        backend = dist.get_backend() if dist.is_initialized() else os.environ.get("DGRP_DIST_BACKEND", "nccl")
        if torch.cuda.is_available():
            local_rank, ndev = int(os.environ.get("LOCAL_RANK", "0")), torch.cuda.device_count()
            if local_rank >= ndev and backend != "gloo":       # (gloo: several ranks may share a GPU -- rehearsals on one card)
                sys.exit(f"rank {rank}: local rank {local_rank} but only {ndev} GPUs visible")
            torch.cuda.set_device(local_rank % max(ndev, 1))
        if world > 1 and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
            else:
                dist.init_process_group(backend)

        if getattr(args, "precise", False) and getattr(args, "fast", False):
            sys.exit("--precise and --fast exclude each other")
        model = dgmodel.device_model(weights)
        options.vecsize = model.input_shape[1]
        _LOG.info("Model loading finished successfully!")
        pipe = CommandLineParser._pipeline(args, options, model)
        outstream = None
        if rank == 0:
            # (headers are carried as bytes through surrogateescape: a Latin-1 header must reach the file as the bytes it was)
            outstream = sys.stdout if args.output == "-" else open(args.output, "w", errors="surrogateescape")

        records_of = _records_of

        runner = RecordRunner(pipe, **{k: v for out in outputs for k, v in out.runner.items()})

        try:
            if world == 1:
                import time
                for filename in args.FASTA:
                    _LOG.info("Processing %s", filename)
                    t_file = time.perf_counter()
                    # the input's rows (contig = record ordinal) are kept once, for the outputs that are written from all of them
                    kept = _RowsByRecord() if any(out.wants_rows for out in outputs) else None
                    # the input's files are renamed into place when all of its records are done, in _COMMIT_ORDER; when anything
                    # raises, what was not committed by then is removed (commit and abort are safe behind each other)
                    handles = []
                    try:
                        for out in outputs:
                            handles.append(out.open(filename))
                        bases = CommandLineParser._predict_file(pipe, runner, filename, records_of(filename), outstream, kept, handles)
                        rows = kept.rows() if kept is not None else None
                        for out, handle in zip(outputs, handles):
                            if out.wants_rows:
                                outstream.flush()
                            handle.commit(rows, _LOG)
                    except BaseException:
                        for handle in handles:
                            handle.abort()
                        raise
                    dt = time.perf_counter() - t_file
                    _LOG.info("%s: %d bases in %.3f s (%.1f Mbp/s; ingest, upload, forward, MSS, segments and TSV text)", filename, bases, dt,
                              bases / max(dt, 1e-9) / 1e6)
            else:
                from .distributed import run_split
                if getattr(args, "split_contigs", False):
                    # every record over all ranks (distributed.run_split): every rank holds every record's class indices and takes
                    # its share of the windows; errors are per record and hit every rank alike
                    records = []
                    for filename in args.FASTA:
                        for header, rec in records_of(filename):
                            records.append((filename, header, rec))
                    parts = []
                    for i, (_f, _h, rec) in enumerate(records):
                        startpos, d_idx = record_indices(rec)
                        parts.append(run_split(pipe, d_idx, startpos, i))
                    allrows = np.concatenate(parts) if parts else np.zeros(0, SEGMENT_DTYPE)
                    if rank == 0:
                        for i, (filename, header, _seq) in enumerate(records):
                            outstream.write(rows_text(filename, header, allrows[allrows["contig"] == i]))
                    if masks is not None:
                        # rank 0 holds every row: it writes the masked copies; the other ranks learn how that went
                        from .distributed import raise_together
                        err = None
                        if rank == 0:
                            try:
                                outstream.flush()
                                for filename in args.FASTA:
                                    ids = [i for i, r in enumerate(records) if r[0] == filename]
                                    i0, i1 = (ids[0], ids[-1] + 1) if ids else (0, 0)
                                    rows = allrows[(allrows["contig"] >= i0) & (allrows["contig"] < i1)].copy()
                                    rows["contig"] -= i0
                                    masking.write_mask(filename, masks.plan.files[filename], rows, masks.plan, _LOG)
                            except Exception as e:          # noqa: BLE001 -- re-raised on every rank together
                                err = e
                        raise_together(err)
                else:
                    CommandLineParser._predict_sharded(args, runner, records_of, outstream, masks)
                dist.barrier()
        finally:
            # rows already produced reach the file even when a later record raises (the reference leaves that to
            # interpreter shutdown)
            if rank == 0 and args.output != "-":
                outstream.close()

    @staticmethod
    def _pipeline(args, options, model):
        """The record pipeline of `predict`'s flags (-s -l -x -b -m --fast --precise)."""
        from .pipeline import ContigPipeline
        pipe = ContigPipeline(model, args.step_size, options.batch_size, options.min_mss_len, options.xdrop_len,
                              use_mss=not args.no_use_mss, precise=getattr(args, "precise", False),
                              fast=getattr(args, "fast", False))
        _LOG.info("Forward kernel: %s", "plain fp32 kernels (more units than the fused kernels take)" if getattr(model, "fp32_only", False)
                  else "fused, split operands (fp32-grade)" if pipe.split else "fused, fp16 operands")
        return pipe

    @staticmethod
    def _predict_file(pipe, runner, filename, records, outstream, kept, handles=()) -> int:
        """predict's loop over one input: the TSV rows of every record to `outstream` and to `kept` (_RowsByRecord, or None), and
        every work item -- names, whether it is a batch, rows, scores, track texts -- to `handles`, the input's files of the outputs
        `runner` was made for (the caller commits or aborts them).  -> bases read"""
        from .evaluation import record_name
        from .fasta import DeviceRecord
        from .runner import rows_text, rows_text_batch
        named = runner.tracks is not None or runner.scores      # the runner's keys are then (header, name of the track and BED lines)
        bases = 0

        def put(headers, names, batch, rows, scores, texts):
            outstream.write(rows_text_batch(filename, headers, rows) if batch else rows_text(filename, headers[0], rows))
            for handle in handles:
                handle.take(names, batch, rows, scores, texts)
            if kept is not None:
                kept.add(rows, len(headers))

        if _LOG.isEnabledFor(logging.DEBUG):
            # -vv: record by record down the runner's own record path, a device sync and a clock around every stage (the reference
            # logs a debug line around each stage of _predict, deepgrp/__main__.py:69-79)
            for chrom, (header, rec) in enumerate(records):
                name = record_name(filename, header) if named else None
                stages = _Stages(header, pipe.use_mss)
                rows, scores, texts = runner.run_record(rec, name, chrom, stage=stages)
                bases += stages.close(rows)
                put([header], [name], False, rows, scores, texts)
        else:
            def keyed():
                nonlocal bases
                for header, rec in records:
                    bases += max(rec.length, 0) + max(rec.startpos, 0) if isinstance(rec, DeviceRecord) else len(rec)
                    yield ((header, record_name(filename, header)) if named else header), rec
            for kind, key, rows, scores, texts in runner.outputs(keyed()):
                keys = key if kind == "batch" else [key]
                put([header for header, _name in keys] if named else keys, [name for _header, name in keys] if named else None,
                    kind == "batch", rows, scores, texts)
        return bases

    @staticmethod
    def _predict_sharded(args, runner, records_of, outstream, masks=None) -> None:
        """Records sharded over the ranks (the reference's record loop, deepgrp/__main__.py:275-292, carries no state from one
        record to the next).  Ingest is rank-local: the chunk table of every FASTA file comes from host scans of 1/world of its
        bytes per rank, the chunks are shared out longest-first by byte length (runs of short records travel together), and a
        rank reads, uploads and encodes ONLY the byte ranges of its share.  Rank 0 gathers the 24-byte segment records (RCCL)
        and writes them in input order.  Inputs that are not regular FASTA files (stdin, .npz) are parsed by every rank and
        shared out as whole records."""
        import torch
        import torch.distributed as dist

        from . import fasta
        from .distributed import file_chunk_tables, gather_records, plan_file_shares, raise_together
        from .fasta import DeviceRecord
        from .pipeline import SEGMENT_DTYPE
        from .runner import rows_text_batch
        world, rank = dist.get_world_size(), dist.get_rank()
        files = list(args.FASTA)
        sharded = [i for i, f in enumerate(files) if f != "-" and os.path.isfile(f) and not f.endswith(".npz")]
        parsed = []                                        # (file index, record number, header, record), the same on every rank
        for i, f in enumerate(files):
            if i not in sharded:
                parsed += [(i, j, header, rec) for j, (header, rec) in enumerate(records_of(f))]
        length = lambda r: max(r.length, 0) if isinstance(r, DeviceRecord) else len(r)
        tables = file_chunk_tables([files[i] for i in sharded])
        sizes = [os.path.getsize(files[i]) for i in sharded]
        ranges, extras = plan_file_shares(tables, sizes, [length(p[3]) for p in parsed], world)
        uploaded0 = fasta.UPLOAD_STATS["bytes"]

        def my_records():
            work = {}
            for f, a, b in ranges[rank]:
                work.setdefault(sharded[f], []).append((a, b))
            for i in extras[rank]:
                work.setdefault(parsed[i][0], []).append(parsed[i])
            for fi in sorted(work):
                if fi in sharded:
                    for key, header, rec in fasta.ingest_ranges(files[fi], work[fi]):
                        yield ((fi, key), header), rec
                else:
                    for _fi, j, header, rec in work[fi]:
                        yield ((fi, (j, 0)), header), rec

        entries, parts, failure = [], [], None           # entries[local id] = (key, header)
        try:
            for kind, key, rows in runner.results(my_records()):
                if kind == "batch":
                    rows["contig"] += len(entries)
                    entries += key
                else:
                    rows["contig"] = len(entries)
                    entries.append(key)
                parts.append(rows)
        except Exception as e:                  # noqa: BLE001 -- re-raised on every rank together, below
            failure = e
        raise_together(failure)                 # a record that raises (all-N ...) must not leave the others in the gather
        every = [None] * world
        dist.all_gather_object(every, entries)
        order = sorted((key, r, lid) for r, ents in enumerate(every) for lid, (key, _h) in enumerate(ents))
        gid = np.zeros(max(len(entries), 1), np.int32)
        for g, (_key, r, lid) in enumerate(order):
            if r == rank:
                gid[lid] = g
        local = np.concatenate(parts) if parts else np.zeros(0, SEGMENT_DTYPE)
        local_ids = local["contig"].copy()
        local["contig"] = gid[local["contig"]]
        allrows = gather_records(local, torch.device("cuda", torch.cuda.current_device()))
        CommandLineParser.last_sharded = {"uploaded_bytes": fasta.UPLOAD_STATS["bytes"] - uploaded0, "records": len(entries),
                                          "file_bytes": int(sum(sizes))}
        _LOG.info("rank %d: %d records, %d of %d file bytes uploaded", rank, len(entries),
                  CommandLineParser.last_sharded["uploaded_bytes"], int(sum(sizes)))
        if rank == 0:
            g = 0
            while g < len(order):                          # one formatter call per input file
                fi, g0 = order[g][0][0], g
                while g < len(order) and order[g][0][0] == fi:
                    g += 1
                lo, hi = np.searchsorted(allrows["contig"], [g0, g])
                rows = allrows[lo:hi].copy()
                rows["contig"] -= g0
                outstream.write(rows_text_batch(files[fi], [every[r][lid][1] for _k, r, lid in order[g0:g]], rows))
        if masks is not None:
            if rank == 0:
                outstream.flush()
            # each rank masks its own byte ranges of every file with its own rows (contig = ordinal of the record among the records
            # of that file this rank ingested, in file order: the local ids of one file are consecutive), into one temporary file
            # per input that rank 0 creates at full size and renames once every rank has written
            file_of = np.array([key[0] for key, _h in entries], np.int64)
            for f, fi in enumerate(sharded):
                sel = file_of[local_ids] == fi
                mine = local[sel].copy()
                mine["contig"] = local_ids[sel] - int(np.searchsorted(file_of, fi))
                spans = [(a, b) for ff, a, b in ranges[rank] if ff == f]
                masking.write_mask_sharded(files[fi], masks.plan.files[files[fi]], mine, spans, masks.plan)

    last_sharded: dict = {}

    @staticmethod
    def evaluate(args: argparse.Namespace, options) -> None:
        """Score `predict`'s rows against an annotation (deepgrp_amd/evaluation.py): TSV report, optionally JSON."""
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("evaluate runs in one process on one GPU; it cannot be sharded (WORLD_SIZE > 1)")
        for output in _OUTPUTS:
            output.refuse_on_evaluate(args)
        if not 0.0 < args.min_overlap <= 1.0:
            sys.exit(f"--min_overlap must lie in (0, 1], not {args.min_overlap}")
        from . import boundaries as dgboundaries, curves as dgcurves, offtarget as dgofftarget, strata as dgstrata
        # the reports that were asked for, in the order of their JSON keys; every plan refuses what it must before the model is read
        plans = [(m, p) for m in (dgcurves, dgstrata, dgofftarget, dgboundaries) for p in [m.plan(args)] if p is not None]
        gff_sides = (("--annotation_names", "--annotation_format", args.annotation_format),)
        _gff_plan(args, None, gff_sides)                         # (the number of entries waits for the model's class count)
        from . import annotation as dgann
        ann_format = None
        if args.annotation_names is not None:                    # (only this refusal needs the file's first lines this early)
            ann_format = dgann.resolve_format(args.annotation, args.annotation_format)
            _gff_resolved(args, "--annotation_names", "--annotation_format", ann_format)
        import json

        from . import model as dgmodel
        from .evaluation import AnnotationError, NoMatchError, evaluate, tsv_report, read_annotation
        # host work first: the model's class count, the repeat numbers and the annotation are checked before the GPU is touched
        weights = dgmodel.read_keras_hdf5(args.model)
        classes = int(weights["ff_kernel"].shape[-1])
        repeats = sorted(set(args.repeats)) if args.repeats is not None else list(range(1, classes))
        bad = [r for r in repeats if not 0 < r < classes]
        if bad:
            sys.exit(f"--repeats: {bad[0]} is not a repeat class of this model (1..{classes - 1})")
        if ann_format is None:
            ann_format = dgann.resolve_format(args.annotation, args.annotation_format)
        listed = ann_format == "repeatmasker"
        gff_names, gff_key = _gff_plan(args, classes, gff_sides)
        try:
            # a table is read here, before the device is touched; a RepeatMasker listing and a GFF3 file are parsed ON the device
            # (the model's class check above still comes first)
            if ann_format == "gff3":
                from . import gffin
                annotation = gffin.read_annotation(args.annotation, gff_names["--annotation_names"], gff_key, repeats)
            elif any(m is dgofftarget for m, _p in plans):
                annotation = dgann.evaluation_rows(args.annotation, repeats, offtarget=True)
            else:
                annotation = dgann.evaluation_rows(args.annotation, repeats) if listed else read_annotation(args.annotation, repeats)
        except AnnotationError as e:
            sys.exit(str(e))
        model = dgmodel.device_model(weights)
        options.vecsize = model.input_shape[1]
        pipe = CommandLineParser._pipeline(args, options, model)
        info = dict(model=args.model, annotation=args.annotation, inputs=list(args.FASTA), repeats=repeats,
                    options=dict(step_size=args.step_size, min_mss_length=args.min_mss_length, xdrop_length=args.xdrop_length,
                                 batch_size=args.batch_size, use_mss=not args.no_use_mss, fast=bool(args.fast),
                                 min_overlap=args.min_overlap))
        reports = [m.from_plan(p, classes, annotation) for m, p in plans]
        try:
            rep = evaluate(model, annotation, ((f, _records_of(f)) for f in args.FASTA), pipe, repeats, args.min_overlap, info, reports)
        except NoMatchError as e:
            sys.exit(str(e))
        for r, (_m, p) in zip(reports, plans):
            r.write(p, _LOG)
        text = tsv_report(rep)
        if args.output == "-":
            sys.stdout.write(text)
            sys.stdout.flush()
        else:
            with open(args.output, "w") as fh:
                fh.write(text)
        if args.json is not None:
            with open(args.json, "w") as fh:
                json.dump(rep, fh, indent=1, allow_nan=False)
                fh.write("\n")

    @staticmethod
    def compare(args: argparse.Namespace, options) -> None:
        """Score rows that are already on disk against an annotation (deepgrp_amd/compare.py): `evaluate`'s report without a model."""
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("compare runs in one process on one GPU; it cannot be sharded (WORLD_SIZE > 1)")
        for output in _OUTPUTS:
            output.refuse_on_evaluate(args)
        # what needs probabilities or scores is refused by name before anything is read
        for flag, given in (("--curves", args.curves is not None), ("--curve_elements", args.curve_elements),
                            ("--curve_bins", args.curve_bins is not None)):
            if given:
                sys.exit(f"{flag} needs the probabilities and row scores of a forward pass, which compare does not run: the curves "
                         "belong to evaluate")
        if not 0.0 < args.min_overlap <= 1.0:
            sys.exit(f"--min_overlap must lie in (0, 1], not {args.min_overlap}")
        from . import compare as dgcompare
        classes = args.classes
        if not dgcompare.MIN_CLASSES <= classes <= dgcompare.MAX_CLASSES:
            sys.exit(f"--classes must lie in {dgcompare.MIN_CLASSES}..{dgcompare.MAX_CLASSES}, not {classes}")
        repeats = sorted(set(args.repeats)) if args.repeats is not None else list(range(1, classes))
        bad = [r for r in repeats if not 0 < r < classes]
        if bad:
            sys.exit(f"--repeats: {bad[0]} is not a repeat class of --classes {classes} (1..{classes - 1})")
        gff_names, gff_key = _gff_plan(args, classes, (("--predicted_names", "--predicted_format", args.predicted_format),
                                                       ("--annotation_names", "--annotation_format", args.annotation_format)))
        from . import boundaries as dgboundaries, offtarget as dgofftarget, strata as dgstrata
        plans = [(m, p) for m in (dgstrata, dgofftarget, dgboundaries) for p in [m.plan(args)] if p is not None]
        for _m, p in plans:
            for out in (v for k, v in p._asdict().items() if k.endswith("_path")):
                if os.path.exists(args.predicted) and os.path.realpath(out) == os.path.realpath(args.predicted):
                    sys.exit(f"the file {out} would overwrite the input {args.predicted}")
        import json

        from . import annotation as dgann
        from .evaluation import AnnotationError, NoMatchError, tsv_report
        ann_format = dgann.resolve_format(args.annotation, args.annotation_format)
        listed = ann_format == "repeatmasker"
        _gff_resolved(args, "--annotation_names", "--annotation_format", ann_format)
        _gff_resolved(args, "--predicted_names", "--predicted_format", dgcompare.resolve_predicted_format(args.predicted, args.predicted_format))
        try:
            predicted = dgcompare.read_predicted(args.predicted, args.predicted_format, classes, gff_names=gff_names["--predicted_names"],
                                                 gff_key=gff_key)
            if ann_format == "gff3":
                from . import gffin
                annotation = gffin.read_annotation(args.annotation, gff_names["--annotation_names"], gff_key, repeats)
            elif any(m is dgofftarget for m, _p in plans):
                annotation = dgann.evaluation_rows(args.annotation, repeats, offtarget=True)
            else:
                annotation = dgann.evaluation_rows(args.annotation, repeats) if listed else dgcompare.read_table(args.annotation, repeats)
        except AnnotationError as e:
            sys.exit(str(e))
        info = dict(predicted=args.predicted, predicted_format=predicted.format, annotation=args.annotation, inputs=list(args.FASTA),
                    repeats=repeats, options=dict(min_overlap=args.min_overlap),
                    predicted_rows=dict(read=predicted.rows_read, dropped=predicted.rows_dropped))
        reports = [m.from_plan(p, classes, annotation) for m, p in plans]
        try:
            rep = dgcompare.compare(predicted, annotation, ((f, _records_of(f)) for f in args.FASTA), classes, repeats, args.min_overlap,
                                    info, reports)
        except (NoMatchError, dgcompare.NoPredictedError) as e:
            sys.exit(str(e))
        for r, (m, p) in zip(reports, plans):
            if m is dgstrata:
                dgcompare.write_strata(r, p, _LOG)
            else:
                r.write(p, _LOG)
        text = tsv_report(rep)
        if args.output == "-":
            sys.stdout.write(text)
            sys.stdout.flush()
        else:
            with open(args.output, "w") as fh:
                fh.write(text)
        if args.json is not None:
            with open(args.json, "w") as fh:
                json.dump(rep, fh, indent=1, allow_nan=False)
                fh.write("\n")

    @staticmethod
    def verify(args: argparse.Namespace, options) -> None:
        """One line per record and fused kernel ("split" = the default where it exists, "fp16" = --fast): largest
        |p_fused - p_fp32| over the compared windows, and how many per-base argmax calls differ.  Exit status 1 if the
        default kernel exceeds 1e-3 on any record."""
        from . import model as dgmodel
        from .fasta import DeviceRecord, read_multi_fasta_device
        from .pipeline import upload_sequence
        model = dgmodel.load_model(args.model, custom_objects={"ReverseComplement": dgmodel.ReverseComplement})
        levels = ([("split", 1)] if model.supports_split else []) + [("fp16", 0)]
        results = []

        def measure(filename, header, d_idx):
            for name, level in levels:
                results.append((filename, header, name, model.check_accuracy(d_idx, args.step_size, args.windows, level=level)))

        if not args.FASTA:
            measure("<random>", "ACGT", None)
        for filename in args.FASTA:
            if filename == "-" or not os.path.isfile(filename):
                stream = sys.stdin if filename == "-" else open(filename, "r")
                records = list(_read_multi_fasta(stream))
            else:
                records = list(read_multi_fasta_device(filename))
            for header, rec in records:
                d_idx = rec.d_idx if isinstance(rec, DeviceRecord) else upload_sequence(rec.encode("utf-8"))[1]
                if d_idx.numel() <= model.input_shape[1]:
                    continue                                                # no window (prediction.py:31)
                measure(filename, header, d_idx)
        bad = False
        for filename, header, kernel, r in results:
            sys.stdout.write(f"{filename}\t{header}\t{kernel}\t{r['max_abs_diff']:.3e}\t{r['windows_checked']}\t{r['argmax_flips']}\t"
                             f"{'ok' if r['within_1e-3'] else 'ABOVE 1e-3'}\n")
            # the verdict is about the kernel `predict` uses by default for this model
            bad = bad or (kernel == levels[0][0] and not r["within_1e-3"])
        if bad:
            sys.exit(1)

    @staticmethod
    def train(args: argparse.Namespace, options) -> None:
        """Train deepgrp (deepgrp/__main__.py:299-351): options from the TOML file, truth from the BED table for the contigs the
        two file names start with, a freshly initialised model trained on the GPU, saved as Keras HDF5."""
        from . import model as dgmodel
        from . import preprocessing as dgpreprocess
        from . import training as dgtrain
        for path in (args.parameter, args.trainfile, args.validfile, args.bedfile):
            if not os.path.isfile(path):
                sys.exit(f"train: {path}: no such file")
        with open(args.parameter, "r") as file:
            parameter = dgmodel.Options.from_toml(file)
        # the reference goes on with parameter.fromdict(options.todict()), which puts every default back over the file's values
        # (units, vecsize, batch_size, ...): the parameter file would be ignored.  Here the file holds.
        try:
            dgtrain.check_options(parameter)                     # refusals come before anything is read or run
        except dgtrain.TrainingRefused as exc:
            sys.exit(f"train: {exc}")
        logdir = args.logdir
        sides = (("trainfile", args.trainfile, "--train_contigs", args.train_contigs),
                 ("validfile", args.validfile, "--valid_contigs", args.valid_contigs))
        npz = [dgtrain.is_npz(path) for _role, path, _flag, _contigs in sides]
        from . import annotation as dgann
        bed_format = dgann.resolve_format(args.bedfile, args.annotation_format)
        if bed_format == "gff3":
            sys.exit(_refuse_gff3("train", args.bedfile))
        listed = bed_format == "repeatmasker"
        if npz[0] != npz[1]:
            kinds = ["a .npz of preprocess_sequence" if z else "a sequence file" for z in npz]
            sys.exit(f"train: {sides[0][0]} {sides[0][1]} is {kinds[0]} and {sides[1][0]} {sides[1][1]} is {kinds[1]}: "
                     "give both sides in one form")
        if npz[0]:
            if listed:
                sys.exit(dgann.refuse_npz("train", args.bedfile))
            for _role, path, flag, contigs in sides:
                if contigs is not None:
                    sys.exit(f"train: {flag} selects records of a sequence file; {path} is a .npz of preprocess_sequence, one "
                             "record named by the file")
            train_chr = os.path.basename(args.trainfile).split(".")[0]
            val_chr = os.path.basename(args.validfile).split(".")[0]
            if not os.path.isdir(logdir):
                os.mkdir(logdir)
            _LOG.info("Loading in all data necessary from %s, %s, %s", args.trainfile, args.validfile, args.bedfile)
            train_fwd = dgpreprocess.load_onehot_npz(args.trainfile)
            val_fwd = dgpreprocess.load_onehot_npz(args.validfile)
            y_train = dgpreprocess.preprocess_y(args.bedfile, train_chr, train_fwd.shape[1], parameter.repeats_to_search)
            y_val = dgpreprocess.preprocess_y(args.bedfile, val_chr, val_fwd.shape[1], parameter.repeats_to_search)
            train_data = dgpreprocess.Data(*dgpreprocess.drop_start_end_n(train_fwd, y_train))
            val_data = dgpreprocess.Data(*dgpreprocess.drop_start_end_n(val_fwd, y_val))
        else:
            # sequence files: the record names are read and checked on the host, then ingest, truth and sampler sets are the GPU's
            picked = []
            for _role, path, flag, contigs in sides:
                contigs = None if contigs is None else [c for c in contigs.split(",") if c]
                try:
                    dgtrain.select_contigs(dgtrain.sequence_names(path), contigs, f"train: {flag}: {path}" if contigs is not None
                                           else f"train: {path}")
                except ValueError as exc:
                    sys.exit(str(exc))
                picked.append(contigs)
            if not os.path.isdir(logdir):
                os.mkdir(logdir)
            _LOG.info("Loading in all data necessary from %s, %s, %s", args.trainfile, args.validfile, args.bedfile)
            try:
                # a RepeatMasker listing is parsed once, on the device, for both sides
                bed = dgann.read_listing(args.bedfile) if listed else args.bedfile
                train_data, val_data = (dgtrain.DeviceData.from_sequence_file(path, bed, parameter.repeats_to_search,
                                                                             contigs, vecsize=int(parameter.vecsize))
                                        for (_role, path, _flag, _c), contigs in zip(sides, picked))
            except ValueError as exc:
                sys.exit(f"train: {exc}")
        _LOG.info("Creating model for training")
        dgmodel.reset_layer_names()
        config = {"class_name": "Functional", "config": dgmodel.model_config(parameter)}
        weights = dgmodel.initial_weights(parameter, args.seed)
        _LOG.info("Training Model")
        best = dgtrain.training((train_data, val_data), parameter, weights, logdir, seed=args.seed)
        _LOG.info("Saving model as %s", args.modelfile)
        dgmodel.save_keras_hdf5(args.modelfile, best["kernel"], best["recurrent_kernel"], best["bias"], best["ff_kernel"],
                                best["ff_bias"], best["scale"], vecsize=int(parameter.vecsize), config=config)

    @staticmethod
    def optimize(args: argparse.Namespace, options) -> None:
        """Hyper-parameter search (deepgrp/optimization.py, driven by the reference's notebook): data as `train` loads it, the
        space from the [space] table, `--max_evals` trials in cohorts of `--cohort`, one line per finished trial."""
        import functools
        import json
        import tomli
        from . import model as dgmodel
        from . import optimization as dgopt
        from . import preprocessing as dgpreprocess
        for path in (args.space, args.parameter, args.trainfile, args.validfile, args.bedfile):
            if not os.path.isfile(path):
                sys.exit(f"optimize: {path}: no such file")
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world > 1:
            sys.exit(f"optimize: WORLD_SIZE = {world}: the search runs in one process on one GPU")
        if not 1 <= args.cohort <= 64:
            sys.exit(f"optimize: --cohort {args.cohort}: 1..64 trials can be trained side by side")
        if args.max_evals < 1:
            sys.exit(f"optimize: --max_evals {args.max_evals}: at least one trial")
        from . import annotation as dgann
        bed_format = dgann.resolve_format(args.bedfile, args.annotation_format)
        if bed_format == "gff3":
            sys.exit(_refuse_gff3("optimize", args.bedfile))
        if bed_format == "repeatmasker":
            sys.exit(dgann.refuse_npz("optimize", args.bedfile))
        with open(args.space, "rb") as file:
            try:
                space = tomli.load(file).get("space")
            except tomli.TOMLDecodeError as exc:
                sys.exit(f"optimize: {args.space}: {exc}")
        if not isinstance(space, dict) or not space:
            sys.exit(f"optimize: {args.space}: no [space] table")
        try:
            dgopt.check_space(space)
        except ValueError as exc:
            sys.exit(f"optimize: {args.space}: {exc}")
        with open(args.parameter, "r") as file:
            parameter = dgmodel.Options.from_toml(file)
        if args.project_root_dir is not None:
            parameter.project_root_dir = args.project_root_dir
        train_chr = os.path.basename(args.trainfile).split(".")[0]
        val_chr = os.path.basename(args.validfile).split(".")[0]
        _LOG.info("Loading in all data necessary from %s, %s, %s", args.trainfile, args.validfile, args.bedfile)
        train_fwd = dgpreprocess.load_onehot_npz(args.trainfile)
        val_fwd = dgpreprocess.load_onehot_npz(args.validfile)
        y_train = dgpreprocess.preprocess_y(args.bedfile, train_chr, train_fwd.shape[1], parameter.repeats_to_search)
        y_val = dgpreprocess.preprocess_y(args.bedfile, val_chr, val_fwd.shape[1], parameter.repeats_to_search)
        train_data = dgpreprocess.Data(*dgpreprocess.drop_start_end_n(train_fwd, y_train))
        val_data = dgpreprocess.Data(*dgpreprocess.drop_start_end_n(val_fwd, y_val))
        run = functools.partial(dgopt.build_and_optimize if args.cohort == 1 else dgopt.build_and_optimize_cohort,
                                train_data, val_data, args.step_size, parameter)

        def objective(draws):
            got = run(draws)
            for draw, res in zip([draws] if args.cohort == 1 else draws, [got] if args.cohort == 1 else got):
                values = " ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in draw.items())
                print(f"trial {draw.tid}\t{res['status']}\tloss {res['loss']:.6g}\t{values}"
                      + (f"\t{res['error']}" if res["error"] else ""), flush=True)
            return got

        count = dgopt.run_a_trial(space, objective, parameter.project_root_dir, args.max_evals, seed=args.seed, cohort=args.cohort)
        with open(os.path.join(parameter.project_root_dir, "results.json"), "r") as file:
            done = [t for t in json.load(file) if t["status"] == dgopt.STATUS_OK]
        if not done:
            print(f"no trial of {count} gave a finite MCC")
            return
        best = min(done, key=lambda t: t["loss"])
        values = " ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in best["params"].items())
        print(f"best of {count}: trial {best['tid']}\tloss {best['loss']:.6g}\t{values}\t{best['logdir']}")


def main(argv=None):
    CommandLineParser().parse_args(argv).set_logging().setup_tensorflow().run()


if __name__ == "__main__":
    main()
