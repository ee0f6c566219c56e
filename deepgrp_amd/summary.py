"""Repeat content table (`predict --summary_dir`): how much of every record of an input is repeat, per class -- the figure of
RepeatMasker's `.tbl` -- with the base composition under each class and the agreement of the predicted repeats with the soft mask
the input already carries (UCSC genomes are soft-masked by RepeatMasker + TRF), from one pass over the bytes on the GPU.

Definitions.  A record's sequence position p is masking.py's: the p-th byte of its body that is neither CR nor LF.  The kind of a
byte is dgrp_encode's class: A/a 0, C/c 1, G/g 2, T/t 3, every other byte 4.  A byte is lower case when it lies in 'a'..'z'.  The
label of a position is the label of the row that covers it, 0 where no row does; a record's rows are ascending and disjoint.  The
counts of a record are `counts[C][5][2]` (int64, C = the model's classes): its positions per (label, kind, case); every base-level
figure below derives from that table.  The row-level figures (rows, minimum, maximum and N50 of the row lengths per label) come
from the rows in numpy: with the lengths sorted longest first, N50 is the length at which twice the running sum first reaches the
total.

`DIR/<basename>.summary.tsv`: one header line; per record, in file order, one line per label 0..C-1 and one line `all` (the labels
> 0 together); behind the last record the same block for the record `*`, the file's totals.  Tab-separated columns:

    record          first word of the header (twobit.record_name)
    label           class<c>, or for c > 0 the c-th name of --bed_names; `all`
    rows            rows of the label (label 0 has none)
    bases           positions under the label
    A C G T other   of these by kind, both cases together
    lower           of these in lower case
    min max N50     of the row lengths; `.` where there is no row
    frac_record     bases / positions of the record
    frac_acgt       ACGT positions under the label / ACGT positions of the record
    gc              (C + G) / (A + C + G + T) under the label
    mask_recall     on `all` lines, else `.`: lower-case positions under a label > 0 / lower-case positions
    mask_precision  on `all` lines, else `.`: lower-case positions under a label > 0 / positions under a label > 0

Every ratio is printed `%.6f` from the two integers, `.` when the denominator is 0: no float comes from the device.  A record with a
sequence line that is not ASCII has no bytes to count: `.` in every base-level column; its rows still count in the row-level
columns, and the totals hold the base-level figures of the other records.

`--summary_bin N` adds `DIR/<basename>.density.tsv`, the table behind a repeat-landscape plot: one header line, then per record
and bin of N positions (the last one short) record, start, end, ACGT positions of the bin, and per label 1..C-1 the positions of
the bin under that label.

Plain records (LF / CRLF line ends only) are counted on the GPU (dgrp_repeat_summary_batch: all plain records of an ingest group
in one call); the others through masking.sequence_byte_offsets and `count_host` / `bins_host`, which state the same integers."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from .outfiles import RowsOutput

KINDS, CASES = 5, 2
MIN_CLASSES, MAX_CLASSES = 2, 64                      # dgrp_repeat_summary_batch's envelope
_KIND = np.full(256, 4, np.int64)
for _k, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _KIND[list(_pair)] = _k
_LOWER = np.zeros(256, np.int64)
_LOWER[97:123] = 1
HEADER = (b"#record\tlabel\trows\tbases\tA\tC\tG\tT\tother\tlower\tmin\tmax\tN50\tfrac_record\tfrac_acgt\tgc\tmask_recall\t"
          b"mask_precision\n")


def bad_row(rows: np.ndarray, n: int, C: int) -> int:
    """The index of the first row dgrp_repeat_summary_batch calls bad in a record of `n` positions, or -1: a label outside 0..C-1,
    start < 0, end <= start, end > n, or the next row starting below its end."""
    if not len(rows):
        return -1
    st, en, lab = rows["start"].astype(np.int64), rows["end"].astype(np.int64), rows["label"].astype(np.int64)
    bad = (lab < 0) | (lab >= C) | (st < 0) | (en <= st) | (en > n)
    bad[:-1] |= st[1:] < en[:-1]
    hit = np.flatnonzero(bad)
    return int(hit[0]) if hit.size else -1


def _labels(rows: np.ndarray, n: int, C: int, what: str) -> np.ndarray:
    """The label of every position of a record of n positions."""
    k = bad_row(rows, n, C)
    if k >= 0:
        raise ValueError(f"{what}: row {k} [{int(rows['start'][k])}, {int(rows['end'][k])}) label {int(rows['label'][k])} is empty, "
                         f"out of order, beyond its sequence of {n} characters or not one of the {C} classes")
    label = np.zeros(n, np.int64)
    for s, e, lab in zip(rows["start"].tolist(), rows["end"].tolist(), rows["label"].tolist()):
        label[s:e] = lab
    return label


def count_host(buf, offs: np.ndarray, rows: np.ndarray, C: int, what: str = "record") -> np.ndarray:
    """counts[C][5][2] of one record in numpy: `buf[offs]` are its sequence bytes (masking.sequence_byte_offsets), `rows` its rows
    in ascending order.  A bad row raises ValueError."""
    buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    seq = buf[offs]
    label = _labels(rows, int(seq.size), C, what)
    cell = (label * KINDS + _KIND[seq]) * CASES + _LOWER[seq]
    return np.bincount(cell, minlength=C * KINDS * CASES).astype(np.int64).reshape(C, KINDS, CASES)


def bins_host(buf, offs: np.ndarray, rows: np.ndarray, C: int, bin: int, what: str = "record") -> np.ndarray:
    """The density table [ceil(n / bin)][C] of one record of n positions in numpy: column 0 the ACGT positions of the bin, column
    l >= 1 its positions under label l."""
    if bin < 1:
        raise ValueError(f"bin must be at least 1, not {bin}")
    buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    seq = buf[offs]
    n = int(seq.size)
    label = _labels(rows, n, C, what)
    nb = (n + bin - 1) // bin
    b = np.arange(n, dtype=np.int64) // bin
    out = np.zeros((nb, C), np.int64)
    np.add.at(out, (b[_KIND[seq] < 4], 0), 1)
    under = label > 0
    np.add.at(out, (b[under], label[under]), 1)
    return out


def n50(lengths) -> int:
    """With the lengths sorted longest first: the length at which twice the running sum first reaches the total (-1: no length)."""
    v = np.sort(np.asarray(lengths, np.int64))[::-1]
    if not v.size:
        return -1
    return int(v[np.argmax(2 * np.cumsum(v) >= v.sum())])


def row_stats(rows: np.ndarray, C: int) -> np.ndarray:
    """[C + 1][5] int64: rows, sum of lengths, minimum, maximum and N50 of the rows of every label 0..C-1, and in line C of the
    labels > 0 together; -1 for minimum, maximum and N50 where there is no row."""
    out = np.zeros((C + 1, 5), np.int64)
    out[:, 2:] = -1
    ln = (rows["end"].astype(np.int64) - rows["start"].astype(np.int64)) if len(rows) else np.zeros(0, np.int64)
    lab = rows["label"].astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    for c in range(C + 1):
        v = ln[lab == c] if c < C else ln[lab > 0]
        if v.size:
            out[c] = (v.size, int(v.sum()), int(v.min()), int(v.max()), n50(v))
    return out


def _ratio(num: int, den: int) -> bytes:
    return b"." if den == 0 else b"%.6f" % (num / den)


def _dot(v: int) -> bytes:
    return b"." if v < 0 else b"%d" % v


def _raw_name(nm) -> bytes:
    return nm if isinstance(nm, bytes) else str(nm).encode("utf-8", "surrogateescape")


def names_refusal(names: Sequence) -> Optional[str]:
    """Why these names cannot stand in the label column, or None: the names are written as they are (GFF3's are %-escaped, a
    TSV has no escape), so an empty name or one with a tab, a line end or another control byte would break the columns."""
    for i, nm in enumerate(names):
        raw = _raw_name(nm)
        if not raw:
            return f"--bed_names: the name of label {i + 1} is empty"
        if any(b < 0x20 or b == 0x7F for b in raw):
            return (f"--bed_names: the name of label {i + 1} holds a tab, a line end or another control character, which the "
                    "tab-separated files of --summary_dir cannot hold")
    return None


def label_names(C: int, names: Optional[Sequence] = None) -> List[bytes]:
    """class<c> for c = 0..C-1, or for c > 0 the names given (C - 1 of them: --bed_names), then `all`."""
    if names is not None and len(names) != C - 1:
        raise ValueError(f"{len(names)} names for {C - 1} repeat classes (labels 1..{C - 1})")
    if names is not None and names_refusal(names) is not None:
        raise ValueError(names_refusal(names))
    out = [b"class%d" % c for c in range(C)]
    if names is not None:
        out[1:] = [_raw_name(nm) for nm in names]
    return out + [b"all"]


def _block(name: bytes, counts: Optional[np.ndarray], stats: np.ndarray, labels: List[bytes]) -> List[bytes]:
    C = len(labels) - 1
    lines = []
    if counts is not None:
        total = int(counts.sum())
        acgt_all = int(counts[:, :4].sum())
        lower_all = int(counts[:, :, 1].sum())
    for c in range(C + 1):
        row_cols = [b"%d" % stats[c, 0]]
        tail = [_dot(int(stats[c, 2])), _dot(int(stats[c, 3])), _dot(int(stats[c, 4]))]
        if counts is None:
            lines.append(b"\t".join([name, labels[c]] + row_cols + [b"."] * 7 + tail + [b"."] * 5) + b"\n")
            continue
        t = counts[c] if c < C else counts[1:].sum(axis=0)
        kind = t.sum(axis=1)
        bases, lower, acgt = int(t.sum()), int(t[:, 1].sum()), int(kind[:4].sum())
        cols = [b"%d" % bases] + [b"%d" % int(k) for k in kind] + [b"%d" % lower]
        ratios = [_ratio(bases, total), _ratio(acgt, acgt_all), _ratio(int(kind[1] + kind[2]), acgt)]
        ratios += [_ratio(lower, lower_all), _ratio(lower, bases)] if c == C else [b".", b"."]
        lines.append(b"\t".join([name, labels[c]] + row_cols + cols + tail + ratios) + b"\n")
    return lines


def format_summary(records, C: int, names: Optional[Sequence] = None) -> bytes:
    """The `.summary.tsv` of a file.  `records`: per record, in file order, (name as bytes, counts [C][5][2] or None for a record
    whose bytes cannot be counted, its rows); `names`: the names of the labels 1..C-1 (--bed_names)."""
    labels = label_names(C, names)
    lines = [HEADER]
    total = np.zeros((C, KINDS, CASES), np.int64)
    every = []
    for name, counts, rows in records:
        lines += _block(name, counts, row_stats(rows, C), labels)
        if counts is not None:
            total += counts
        every.append(rows)
    allrows = np.concatenate(every) if every else np.zeros(0, [("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
    lines += _block(b"*", total, row_stats(allrows, C), labels)
    return b"".join(lines)


def density_header(C: int, names: Optional[Sequence] = None) -> bytes:
    return b"\t".join([b"#record", b"start", b"end", b"acgt"] + label_names(C, names)[1:C]) + b"\n"


def format_density(name: bytes, bins: np.ndarray, n: int, bin: int) -> bytes:
    """The `.density.tsv` lines of one record of n positions: `bins` [>= ceil(n / bin)][C], the lines of the first ceil(n / bin)."""
    nb = (n + bin - 1) // bin
    start = np.arange(nb, dtype=np.int64) * bin
    end = np.minimum(start + bin, n)
    table = np.concatenate([start[:, None], end[:, None], np.asarray(bins[:nb], np.int64)], axis=1)
    return b"".join(name + b"\t" + b"\t".join(b"%d" % v for v in row) + b"\n" for row in table.tolist())


def _count_device(g, per, C: int, bin: int, what: str):
    """dgrp_repeat_summary_batch over the plain records of one walk group (`per`: their rows) -> (counts [nrec][C][5][2], bins
    [sum of reserved bins][C] or None, the bin offsets)."""
    import torch

    from ._lib import check
    from .pipeline import stream_ptr
    L, dev = g.L, g.dev
    nrec = len(g.dev_recs)
    h_row_off = np.zeros(nrec + 1, np.int64)
    np.cumsum([len(p) for p in per], out=h_row_off[1:])
    nrows = int(h_row_off[-1])
    sel = np.ascontiguousarray(np.concatenate(per)) if nrows else None
    d_rows = torch.from_numpy(sel.view(np.uint8)).to(dev) if nrows else None
    h_bin_off = np.zeros(nrec + 1, np.int64)
    if bin:
        np.cumsum((g.h_len + bin - 1) // bin, out=h_bin_off[1:])
    nbins = int(h_bin_off[-1])
    d_counts = torch.empty(nrec * C * KINDS * CASES, dtype=torch.int64, device=dev)
    d_bins = torch.empty(nbins * C, dtype=torch.int64, device=dev) if nbins else None
    d_bad = torch.empty(1, dtype=torch.int64, device=dev)
    wb = int(L.dgrp_repeat_summary_workspace_bytes(nrec, int(g.h_len.sum()), nrows))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    check(L.dgrp_repeat_summary_batch(g.ptr, nrec, g.h_off.ctypes.data, g.h_len.ctypes.data, d_rows.data_ptr() if nrows else None,
                                      h_row_off.ctypes.data, C, bin, h_bin_off.ctypes.data if bin else None, d_counts.data_ptr(),
                                      d_bins.data_ptr() if nbins else None, d_bad.data_ptr(), work.data_ptr(), wb, stream_ptr()),
          f"dgrp_repeat_summary_batch ({what})")
    counts = d_counts.cpu().numpy().reshape(nrec, C, KINDS, CASES)              # (the copy waits for the stream)
    bad = int(d_bad.cpu().numpy()[0])
    if bad >= 0:
        j = int(np.searchsorted(h_row_off, bad, side="right") - 1)
        q = sel[bad]
        raise ValueError(f"{what}: record {g.dev_names[j].decode('utf-8', 'replace')!r}: row {bad - int(h_row_off[j])} "
                         f"[{int(q['start'])}, {int(q['end'])}) label {int(q['label'])} is empty, out of order, beyond its sequence of "
                         f"{int(counts[j].sum())} characters or not one of the {C} classes")
    bins = d_bins.cpu().numpy().reshape(nbins, C) if nbins else (np.zeros((0, C), np.int64) if bin else None)
    return counts, bins, h_bin_off


def write_summary(fasta_path, out_path, rows, classes: int, bin: Optional[int] = None, bin_path=None, names: Optional[Sequence] = None,
                  group_bytes: int = 256 << 20, group_records: int = 4096) -> dict:
    """Write the `.summary.tsv` of `fasta_path` to `out_path` and, with `bin` (>= 1), its `.density.tsv` to `bin_path`.  `rows`
    (pipeline.SEGMENT_DTYPE): the TSV rows, `contig` = the record's ordinal in the file (masking.mask_fasta's input); `classes`: the
    model's classes C; `names`: the names of the labels 1..C-1.  The input may be plain FASTA, gzip or a UCSC .2bit file
    (repeatseq.walk_groups).  Both files are staged (outfiles.StagedFile): renamed into place on success, removed on failure.
    Returns dict(records, device_records, host_records, uncounted_records, positions, repeat_positions, rows)."""
    import contextlib

    from .outfiles import StagedFile
    from .pipeline import SEGMENT_DTYPE
    from .repeatseq import walk_groups

    C = int(classes)
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        raise ValueError(f"the summary takes {MIN_CLASSES}..{MAX_CLASSES} classes, not {C}")
    bin = int(bin) if bin else 0
    if bin < 0:
        raise ValueError(f"bin must be at least 1, not {bin}")
    if bool(bin) != (bin_path is not None):
        raise ValueError("the density table needs both a bin and a file name")
    label_names(C, names)
    rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
    rows = rows[np.lexsort((rows["start"], rows["contig"]))] if rows.size else rows
    contig = rows["contig"]

    def rows_of(k):
        lo, hi = np.searchsorted(contig, [k, k + 1])
        return rows[lo:hi]

    report = dict(records=0, device_records=0, host_records=0, uncounted_records=0, positions=0, repeat_positions=0, rows=int(rows.size))
    staged = []
    records = []                                                # (name, counts or None, rows) in file order
    ordinal = 0
    try:
        out = StagedFile(str(out_path))
        staged.append(out)
        dens = None
        if bin:
            dens = StagedFile(str(bin_path))
            staged.append(dens)
            dens.fh.write(density_header(C, names))
        with contextlib.closing(walk_groups(fasta_path, group_bytes, group_records, "its bases are not counted")) as groups:
            for g in groups:
                ordinal = g.records
                found = {}                                      # ordinal -> (name, counts or None, bins or None)
                if g.dev_recs:
                    per = [rows_of(k) for _i, k in g.dev_recs]
                    counts, bins, bin_off = _count_device(g, per, C, bin, str(fasta_path))
                    for j, (_i, k) in enumerate(g.dev_recs):
                        found[k] = (g.dev_names[j], counts[j], bins[bin_off[j]:bin_off[j + 1]] if bin else None)
                    report["device_records"] += len(g.dev_recs)
                for k, name, chunk, offs in g.host_recs:
                    if offs is None:
                        found[k] = (name, None, None)
                        report["uncounted_records"] += 1
                        continue
                    what = f"{fasta_path}: record {name.decode('utf-8', 'replace')!r}"
                    found[k] = (name, count_host(chunk, offs, rows_of(k), C, what),
                                bins_host(chunk, offs, rows_of(k), C, bin, what) if bin else None)
                    report["host_records"] += 1
                for k in sorted(found):
                    name, counts, bins = found[k]
                    records.append((name, counts, rows_of(k)))
                    if dens is not None and counts is not None:
                        dens.fh.write(format_density(name, bins, int(counts.sum()), bin))
                del g
        if contig.size and int(contig[-1]) >= ordinal:
            raise ValueError(f"{fasta_path}: rows name record {int(contig[-1])}, but only {ordinal} records were read")
        out.fh.write(format_summary(records, C, names))
        for f in staged:
            f.finish()
        for f in staged:
            f.commit()
    except BaseException:
        for f in staged:
            f.abort()
        raise
    report["records"] = len(records)
    report["positions"] = int(sum(int(c.sum()) for _n, c, _r in records if c is not None))
    report["repeat_positions"] = int(sum(int(c[1:].sum()) for _n, c, _r in records if c is not None))
    return report


# ------------------------------------------------------------------------- the output of `predict`
class SummaryPlan(NamedTuple):
    files: dict                                     # input file -> (its summary, its density table or None)
    bin: Optional[int]                              # --summary_bin
    names: Optional[tuple]                          # --bed_names: the name of label 1..C-1


def add_options(parser) -> None:
    """The repeat-content flags, like the repeat-sequence flags on `predict` and on the main parser, set only where given."""
    s = argparse.SUPPRESS
    parser.add_argument("--summary_dir", type=str, default=s,
                        help="(addition) also write the repeat content of every input as DIR/<basename of the input>.summary.tsv: per "
                             "record and label (and for all labels > 0 together, and for the whole file) rows, bases, A, C, G, T, "
                             "other, lower case, min, max and N50 of the row lengths, share of the record, of its ACGT bases, GC, and "
                             "recall and precision against the input's own soft mask, counted on the GPU; --bed_names names the "
                             "labels; one process only")
    parser.add_argument("--summary_bin", type=int, default=s,
                        help="(addition) with --summary_dir: also DIR/<basename>.density.tsv, per record and bin of N sequence "
                             "positions the ACGT bases and the positions under every label > 0 (N >= 1)")


def refuse_on_evaluate(args) -> None:
    if getattr(args, "summary_dir", None) is not None or getattr(args, "summary_bin", None) is not None:
        sys.exit("--summary_dir belongs to predict, not evaluate")


def plan(args) -> Optional[SummaryPlan]:
    """--summary_dir and its options, or None without the flag.  Everything that can be refused without the model is refused here
    (sys.exit), before any prediction."""
    sdir, nbin = getattr(args, "summary_dir", None), getattr(args, "summary_bin", None)
    if sdir is None:
        if nbin is not None:
            sys.exit("--summary_bin needs --summary_dir")
        return None
    if nbin is not None and nbin < 1:
        sys.exit(f"--summary_bin must be at least 1, not {nbin}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or getattr(args, "split_contigs", False):
        sys.exit("--summary_dir: the repeat content of an input is counted by one process, from all of its rows; it cannot be "
                 "counted by several ranks (WORLD_SIZE > 1, --split_contigs); run in one process")
    names = getattr(args, "bed_names", None)
    if names is not None:
        from . import gff
        names = tuple(nm.encode("utf-8", "surrogateescape") for nm in names.split(","))
        if gff.names_refusal(names) is not None:
            sys.exit(gff.names_refusal(names))
        if names_refusal(names) is not None:
            sys.exit(names_refusal(names))
    from .outfiles import plan_inputs
    from .tracks import input_basename

    def outputs_of(f):
        base = os.path.join(sdir, input_basename(f))
        return (base + ".summary.tsv", base + ".density.tsv" if nbin is not None else None)

    files = plan_inputs("--summary_dir", args.FASTA, outputs_of, "summaries", stdin="read a second time for the counts",
                        npz="holds no sequence bytes to count", every_input=True, directory=sdir)
    return SummaryPlan(files, nbin, names)


def from_plan(p: SummaryPlan, classes: int) -> "Summary":
    """The model's class count against the kernel's envelope and against the number of names (sys.exit)."""
    if not MIN_CLASSES <= classes <= MAX_CLASSES:
        sys.exit(f"--summary_dir: the model has {classes} classes; the summary takes {MIN_CLASSES}..{MAX_CLASSES}")
    if p.names is not None and len(p.names) != classes - 1:
        sys.exit(f"--bed_names gives {len(p.names)} names, but the model has {classes - 1} repeat classes (labels 1..{classes - 1})")
    return Summary(p, classes)


class Summary(RowsOutput):
    """--summary_dir as an output of `predict`: the repeat content of an input is counted when the input is done, from all of its
    rows (write_summary stages its files: renamed on success, removed on failure)."""

    def __init__(self, p: SummaryPlan, classes: int):
        self.plan, self.classes = p, classes

    def write(self, filename: str, rows, log) -> None:
        p, t0 = self.plan, time.perf_counter()
        final, density = p.files[filename]
        rep = write_summary(filename, final, rows, self.classes, bin=p.bin, bin_path=density, names=p.names)
        log.info("%s: repeat content of %d records (%d counted on the device, %d on the host), %d of %d positions under %d rows, to "
                 "%s in %.2f ms", filename, rep["records"], rep["device_records"], rep["host_records"], rep["repeat_positions"],
                 rep["positions"], rep["rows"], final, (time.perf_counter() - t0) * 1e3)
