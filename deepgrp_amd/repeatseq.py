"""FASTA of the predicted repeats (`predict --seq_dir`): one FASTA record per TSV row of an input, in TSV order -- what `bedtools
getfasta` would give for the rows, without a second tool, a second pass or an indexed uncompressed FASTA.

For a row (start, end, label) of a record named NAME (the first word of its header) with `len` sequence positions:

    A = start - min(flank, start)        B = end + min(flank, len - end)         (0-based, half-open)
    >NAME:A-B class<label>LF                       (flank == 0)
    >NAME:A-B class<label> core=<start>-<end>LF    (flank > 0)
    the bytes of the sequence positions [A, B) as the input has them, `width` per line, every line LF-terminated

A record's sequence position p is masking.py's: the p-th character of the sequence the reference's line loop builds.  Plain records
(LF / CRLF line ends only) are gathered on the GPU (dgrp_fasta_extract_batch: all plain records of an ingest group in one call);
the others through masking.sequence_byte_offsets and `extract_host`, which gives the same bytes."""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import mmap
import os
import sys
import time
from typing import Iterable, List, NamedTuple, Optional, Tuple

import numpy as np

from .masking import class_bits, sequence_byte_offsets
from .outfiles import RowsOutput, class_list

_LOG = logging.getLogger(__name__)

SEQ_PIECE = 256 << 20                # bytes of text one device call is given room for; a group with more goes in several calls
MAX_WIDTH = 1 << 30
ENTRY_DTYPE = np.dtype([("text_off", "<i8"), ("base_off", "<i8"), ("bases", "<i8")])       # struct dgrp_extract_entry


def _digits(v: np.ndarray) -> np.ndarray:
    """Decimal digits of non-negative integers."""
    v = np.asarray(v, np.int64)
    d = np.ones(v.shape, np.int64)
    for k in range(1, 19):
        d += v >= 10 ** k
    return d


def kept_rows(rows: np.ndarray, bits: int) -> np.ndarray:
    """Per row: its label is in the class mask (dgrp_fasta_extract_batch's rule)."""
    lab = rows["label"].astype(np.int64)
    ok = (lab >= 0) & (lab < 64)
    return ok & ((np.uint64(bits) >> np.where(ok, lab, 0).astype(np.uint64)) & np.uint64(1)).astype(bool)


def row_bounds(rows: np.ndarray, name_lens, flank: int, width: int) -> np.ndarray:
    """Per row an upper bound of its text bytes, stated without the sequence lengths: B <= end + flank.  Exact at flank 0."""
    st, en = rows["start"].astype(np.int64), rows["end"].astype(np.int64)
    a = st - np.minimum(flank, st)
    b = en + flank
    bases = b - a
    hdr = 1 + np.asarray(name_lens, np.int64) + 1 + _digits(a) + 1 + _digits(b) + 6 + _digits(np.maximum(rows["label"], 0)) + 1
    if flank > 0:
        hdr = hdr + 6 + _digits(st) + 1 + _digits(en)
    return hdr + bases + (bases + width - 1) // width


def text_bound(rows: np.ndarray, name_lens, flank: int, width: int) -> int:
    """An upper bound of the text bytes of `rows` (all taken as kept; `name_lens`: the name length of every row's record, an array
    or one number): the sum of row_bounds.  Exact at flank 0."""
    return int(row_bounds(rows, name_lens, flank, width).sum()) if len(rows) else 0


def _wrapped(seq: np.ndarray, width: int) -> bytes:
    n = seq.size
    out = np.full(n + (n + width - 1) // width, 10, np.uint8)
    i = np.arange(n, dtype=np.int64)
    out[i + i // width] = seq
    return out.tobytes()


def extract_host(buf, offs: np.ndarray, name: bytes, rows: np.ndarray, bits: int, flank: int = 0, width: int = 60,
                 what: str = "record") -> Tuple[bytes, np.ndarray]:
    """The text of one record's rows as dgrp_fasta_extract_batch writes it, in numpy: `buf[offs]` are the record's sequence bytes
    (masking.sequence_byte_offsets), `rows` its rows in ascending order.  -> (text, entries of the kept rows: ENTRY_DTYPE, offsets
    in the text)."""
    buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    n = int(offs.size)
    st, en = rows["start"].astype(np.int64), rows["end"].astype(np.int64)
    if (st < 0).any() or (en <= st).any() or (en > n).any() or (st[1:] < en[:-1]).any():
        raise ValueError(f"{what}: a row is empty, out of order or beyond its sequence of {n} characters")
    keep = kept_rows(rows, bits)
    parts: List[bytes] = []
    entries = np.zeros(int(keep.sum()), ENTRY_DTYPE)
    at = k = 0
    for s, e, lab in zip(st[keep].tolist(), en[keep].tolist(), rows["label"][keep].tolist()):
        a, b = s - min(flank, s), e + min(flank, n - e)
        head = b">" + name + b":%d-%d class%d" % (a, b, lab) + (b" core=%d-%d" % (s, e) if flank > 0 else b"") + b"\n"
        body = _wrapped(buf[offs[a:b]], width)
        entries[k] = (at, at + len(head), b - a)
        parts += [head, body]
        at += len(head) + len(body)
        k += 1
    return b"".join(parts), entries


def fai_lines(name: bytes, starts: np.ndarray, entries: np.ndarray, flank: int, width: int, shift: int) -> bytes:
    """The `.fai` lines of the kept rows of one record (`starts`: their row starts): name = NAME:A-B, bases, offset of the first base
    (`shift` = the bytes of the file in front of the entries' text), W' = min(width, bases), W' + 1 -- as `samtools faidx` writes."""
    out = []
    for s, e in zip(starts.tolist(), entries.tolist()):
        a = s - min(flank, s)
        w = min(width, e[2])
        out.append(name + b":%d-%d\t%d\t%d\t%d\t%d\n" % (a, a + e[2], e[2], shift + e[1], w, w + 1))
    return b"".join(out)


def _extract_device(L, dev, ptr, h_off, h_len, sel, h_row_off, names: List[bytes], bits, flank, width, want_entries, what):
    """dgrp_fasta_extract_batch over the rows `sel` of the records (h_off, h_len) of the buffer at `ptr`, in pieces of at most
    SEQ_PIECE bytes of text by text_bound (a row whose own text is larger goes alone, in a buffer of its exact size).  Yields
    (d_text, entries or None, lo, hi) per piece: the text of the rows sel[lo:hi]."""
    import torch

    from ._lib import check, name_blob
    from .pipeline import stream_ptr
    nrec = len(names)
    _raw, blob, h_name_off = name_blob(names)
    d_names = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev) if blob else None
    nrows = int(sel.size)
    rec_of = np.searchsorted(h_row_off, np.arange(nrows), side="right") - 1
    name_len = np.diff(h_name_off)[rec_of]
    keep = kept_rows(sel, bits)
    # per-row bounds (a row outside the class mask has no text), cut into pieces at SEQ_PIECE
    per = np.where(keep, row_bounds(sel, name_len, flank, width), 0)
    cuts, acc = [0], 0
    for i, b in enumerate(per.tolist()):
        if acc and acc + b > SEQ_PIECE:
            cuts.append(i)
            acc = 0
        acc += b
    cuts.append(nrows)
    d_rows = torch.from_numpy(sel.view(np.uint8)).to(dev)
    wb = int(L.dgrp_fasta_extract_workspace_bytes(nrec, int(h_len.sum()), nrows))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi == lo:
            continue
        piece_off = np.clip(h_row_off, lo, hi).astype(np.int64)
        cap = min(int(per[lo:hi].sum()), SEQ_PIECE)
        size, kept = C.c_int64(0), C.c_int64(0)
        d_entries = torch.empty((hi - lo) * ENTRY_DTYPE.itemsize, dtype=torch.uint8, device=dev) if want_entries else None
        for attempt in (0, 1):
            d_text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            rc = L.dgrp_fasta_extract_batch(ptr, nrec, h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(), piece_off.ctypes.data,
                                            d_names.data_ptr() if d_names is not None else None, h_name_off.ctypes.data, flank, width,
                                            bits, d_text.data_ptr(), cap, C.byref(size), d_entries.data_ptr() if want_entries else None,
                                            C.byref(kept), work.data_ptr(), wb, stream_ptr())
            if rc == -3 and attempt == 0 and size.value > cap:      # DGRP_ENOMEM: one row larger than a piece, in a buffer of its size
                cap = size.value
                del d_text
                continue
            check(rc, f"dgrp_fasta_extract_batch ({what})")
            break
        entries = None
        if want_entries:
            entries = d_entries[:kept.value * ENTRY_DTYPE.itemsize].cpu().numpy().view(ENTRY_DTYPE)
        yield d_text[:size.value], entries, lo, hi
        del d_text, d_entries


class WalkGroup:
    """One ingest group of `walk_groups`.  `dev_recs`: (index in the group, ordinal) of its plain records, `dev_names` their names;
    their bodies are bytes [h_off[j], h_off[j] + h_len[j]) of the 16-byte aligned device address `ptr` (the group's bytes stay in
    HBM while the group lives).  `host_recs`: (ordinal, name, chunk bytes, offsets of the sequence bytes in the chunk or None for a
    record with a non-ASCII sequence line) of the others.  `records`: the records of the file up to and including this group."""

    __slots__ = ("L", "dev", "dev_recs", "dev_names", "host_recs", "ptr", "h_off", "h_len", "records", "_grp")


def walk_groups(fasta_path, group_bytes: int, group_records: int, skipped: str):
    """The second walk over an input that `predict` has read, with its bytes resident: plain FASTA, gzip (gz.open_inflated: the
    inflated text) or a UCSC .2bit file (twobit.open_text: the text of the file, soft-masked bases lower case), in the ingest's
    groups.  Yields one WalkGroup per group; a record's ordinal is its place among the records the reference loop yields, in file
    order.  A record with a non-ASCII sequence line gets one warning that ends in `skipped`.  Close the generator (or exhaust it)
    to release the file."""
    import contextlib

    from . import gz
    from . import twobit as tbit
    from ._lib import lib
    from .fasta import RESIDENT_BYTES, _chunk_groups, _upload_file
    from .masking import _text_encoding
    from .pipeline import require_gpu

    text = d_text = None
    if gz.is_gzip(fasta_path):
        text, d_text, size = gz.open_inflated(fasta_path, RESIDENT_BYTES, require_gpu, _upload_file)
    elif tbit.is_twobit(fasta_path):
        text, d_text, size = tbit.open_text(fasta_path, RESIDENT_BYTES, require_gpu, _upload_file)
    else:
        size = os.path.getsize(fasta_path)
    if not size:
        return
    L = lib()
    dev = require_gpu()
    ordinal = 0
    with contextlib.ExitStack() as stack:
        if d_text is not None:
            mm = text
        else:
            fh = stack.enter_context(open(fasta_path, "rb"))
            mm = stack.enter_context(mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ))
        for grp in _chunk_groups(L, dev, fasta_path, mm, 0, size, group_bytes, group_records, keep_raw=True, d_file=d_text):
            g0 = grp.starts[grp.c0]
            g = WalkGroup()
            g.L, g.dev, g._grp = L, dev, grp
            g.dev_recs, g.dev_names, g.host_recs = [], [], []
            for i, c in enumerate(range(grp.c0, grp.c1)):
                a, b = grp.starts[c], grp.starts[c + 1]
                if grp.plain(i):
                    header = mm[a:grp.head_ends[c]].decode("ascii").strip()[1:]
                    if header:
                        g.dev_recs.append((i, ordinal))
                        g.dev_names.append(tbit.record_name(header))
                        ordinal += 1
                    continue
                chunk = mm[a:b]
                for header, offs in sequence_byte_offsets(chunk):
                    if offs is None:
                        _LOG.warning("%s: record %r has sequence lines that are not ASCII; %s", fasta_path, header, skipped)
                    g.host_recs.append((ordinal, tbit.record_name(header, _text_encoding()), chunk, offs))
                    ordinal += 1
            g.ptr, g.h_off, g.h_len = 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
            if g.dev_recs:
                # d_raw may be a view of the resident range at any offset: the kernels take the 16-byte aligned address below it
                # (inside the same allocation) and offsets that include the difference
                ptr = grp.d_raw.data_ptr()
                shift = ptr & 15
                g.ptr = ptr - shift
                g.h_off = np.array([grp.body0s[i] - g0 + shift for i, _k in g.dev_recs], np.int64)
                g.h_len = np.array([grp.starts[grp.c0 + i + 1] - grp.body0s[i] for i, _k in g.dev_recs], np.int64)
            g.records = ordinal
            del grp
            yield g
            del g


def write_repeat_fasta(fasta_path, out_path, rows, classes: Optional[Iterable[int]] = None, flank: int = 0, width: int = 60,
                       compress: bool = False, level: int = 1, fai_path=None, group_bytes: int = 256 << 20,
                       group_records: int = 4096) -> int:
    """Write the FASTA of the rows of `fasta_path` to `out_path`.  `rows` (pipeline.SEGMENT_DTYPE): the TSV rows, `contig` = the
    record's ordinal among the records the reference loop yields, in file order (masking.mask_fasta's input).  `classes`: the labels
    to write (None: every label > 0).  The input may be plain FASTA, gzip (gz.open_inflated: the inflated text) or a UCSC .2bit file
    (twobit.open_text: the text of the file, soft-masked bases lower case).  Works in the ingest's groups: the plain records of a
    group go through dgrp_fasta_extract_batch in one call (several when text_bound exceeds SEQ_PIECE), the others through
    `extract_host`; a record with a non-ASCII sequence line gets one warning and contributes nothing.  `compress=True`: `out_path`
    is the BGZF file of the same bytes, deflated on the device where the text is (gz.bgzf_members_device at `level`), the EOF member
    behind the last.  `fai_path`: also the `.fai` of the (uncompressed) file, from the entries the device returns.  Both files are
    staged (outfiles.StagedFile): renamed into place on success, removed on failure.  Returns the bytes of FASTA text written."""
    import contextlib

    import torch

    from . import gz
    from .outfiles import StagedFile
    from .pipeline import SEGMENT_DTYPE

    if not 1 <= int(width) <= MAX_WIDTH:
        raise ValueError(f"line width must lie in 1..2^30, not {width}")
    if flank < 0:
        raise ValueError(f"flank must not be negative, got {flank}")
    if level not in gz.LEVELS:
        raise ValueError(f"compression level must be one of {gz.LEVELS}, not {level!r}")
    if compress and fai_path is not None:
        raise ValueError("a .fai states offsets of the uncompressed file; a BGZF FASTA would also need a .gzi")
    flank, width, bits = int(flank), int(width), class_bits(classes)
    rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
    rows = rows[np.lexsort((rows["start"], rows["contig"]))] if rows.size else rows
    contig = rows["contig"]

    def rows_of(k):
        lo, hi = np.searchsorted(contig, [k, k + 1])
        return rows[lo:hi]

    staged = []
    written = 0                                                 # bytes of FASTA text so far
    ordinal = 0
    try:
        out = StagedFile(str(out_path))
        staged.append(out)
        fai = None
        if fai_path is not None:
            fai = StagedFile(str(fai_path))
            staged.append(fai)

        def emit(data, dev=None):
            """One piece of text: host bytes or a device tensor."""
            nonlocal written
            if isinstance(data, torch.Tensor):
                n = int(data.numel())
                out.fh.write(gz.bgzf_members_device(data, level) if compress else data.cpu().numpy().tobytes())
            else:
                n = len(data)
                if compress and n:
                    data = gz.bgzf_members_device(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev), level)
                out.fh.write(data)
            written += n

        with contextlib.closing(walk_groups(fasta_path, group_bytes, group_records, "none of its repeats is written")) as groups:
            for g in groups:
                ordinal = g.records
                L, dev, dev_recs, dev_names, host_recs = g.L, g.dev, g.dev_recs, g.dev_names, g.host_recs
                pieces = iter(())
                mixed = bool(host_recs)
                if dev_recs:
                    per = [rows_of(k) for _i, k in dev_recs]
                    h_row_off = np.zeros(len(dev_recs) + 1, np.int64)
                    np.cumsum([len(p) for p in per], out=h_row_off[1:])
                    if h_row_off[-1]:
                        sel = np.concatenate(per)
                        pieces = _extract_device(L, dev, g.ptr, g.h_off, g.h_len, sel, h_row_off, dev_names, bits, flank, width,
                                                 mixed or fai is not None, str(fasta_path))
                        rec_of = np.searchsorted(h_row_off, np.arange(sel.size), side="right") - 1
                if not mixed:
                    for d_piece, entries, lo, hi in pieces:
                        if fai is not None:
                            keep = np.flatnonzero(kept_rows(sel[lo:hi], bits)) + lo
                            for j in np.unique(rec_of[keep]).tolist():
                                m = rec_of[keep] == j
                                fai.fh.write(fai_lines(dev_names[j], sel["start"][keep[m]], entries[m], flank, width, written))
                        emit(d_piece)
                        del d_piece
                else:
                    # (rare) records of both paths in one group: the device text comes down and is cut by record
                    texts = {}                                  # ordinal -> [(text, entries, row starts)]
                    for d_piece, entries, lo, hi in pieces:
                        h_piece = d_piece.cpu().numpy().tobytes()
                        keep = np.flatnonzero(kept_rows(sel[lo:hi], bits)) + lo
                        ends = np.append(entries["text_off"][1:], len(h_piece))
                        for j in np.unique(rec_of[keep]).tolist():
                            m = np.flatnonzero(rec_of[keep] == j)
                            t0, t1 = int(entries["text_off"][m[0]]), int(ends[m[-1]])
                            e = entries[m].copy()
                            e["text_off"] -= t0
                            e["base_off"] -= t0
                            texts.setdefault(dev_recs[j][1], []).append((h_piece[t0:t1], e, sel["start"][keep[m]], dev_names[j]))
                        del d_piece
                    for k, name, chunk, offs in host_recs:
                        if offs is None:
                            continue
                        rk = rows_of(k)
                        t, e = extract_host(chunk, offs, name, rk, bits, flank, width, f"{fasta_path}: record {name!r}")
                        texts[k] = [(t, e, rk["start"][kept_rows(rk, bits)], name)]
                    for k in sorted(texts):
                        for t, e, starts, name in texts[k]:
                            if fai is not None:
                                fai.fh.write(fai_lines(name, starts, e, flank, width, written))
                            emit(t, dev)
                del g
        if contig.size and int(contig[-1]) >= ordinal:
            raise ValueError(f"{fasta_path}: rows name record {int(contig[-1])}, but only {ordinal} records were read")
        if compress:
            out.fh.write(gz.BGZF_EOF)
        for f in staged:
            f.finish()
        for f in staged:
            f.commit()
    except BaseException:
        for f in staged:
            f.abort()
        raise
    return written


# ------------------------------------------------------------------------- the output of `predict`
class SeqPlan(NamedTuple):
    files: dict                                     # input file -> the FASTA of its repeats
    classes: Optional[Tuple[int, ...]]              # --seq_classes (None: every label > 0)
    flank: int
    width: int
    gzip: bool                                      # --seq_gzip
    fai: bool                                       # --seq_fai: <file>.fai beside every file
    level: int                                      # --gzip_level of --seq_gzip


def add_options(parser) -> None:
    """The repeat-sequence flags, like the track flags on `predict` and on the main parser, set only where given."""
    s = argparse.SUPPRESS
    parser.add_argument("--seq_dir", type=str, default=s,
                        help="(addition) also write the sequences of the predicted repeats of every input as FASTA, DIR/<basename of "
                             "the input>.repeats.fa: per TSV row one record '>NAME:A-B class<label>' (0-based, half-open, as bedtools "
                             "getfasta names it) with the bases of the row exactly as the input has them, gathered on the GPU; one "
                             "process only")
    parser.add_argument("--seq_classes", type=class_list, default=s,
                        help="(addition) with --seq_dir: comma-separated labels to write, e.g. 1,3 (default: every label > 0)")
    parser.add_argument("--seq_flank", type=int, default=s,
                        help="(addition) with --seq_dir: also take up to N bases on either side of every row, clamped to the record; "
                             "the header then ends in ' core=<start>-<end>' (default: 0)")
    parser.add_argument("--seq_width", type=int, default=s,
                        help="(addition) with --seq_dir: bases per line, 1..2^30 (default: 60)")
    parser.add_argument("--seq_gzip", action="store_true", default=s,
                        help="(addition) with --seq_dir: write the FASTA as BGZF (bgzip's format) to DIR/<basename>.repeats.fa.gz, "
                             "deflated on the GPU (--gzip_level, 1 unless given)")
    parser.add_argument("--seq_fai", action="store_true", default=s,
                        help="(addition) with --seq_dir: also write the samtools faidx index DIR/<basename>.repeats.fa.fai; not with "
                             "--seq_gzip")


def refuse_on_evaluate(args) -> None:
    if any(getattr(args, k, None) not in (None, False) for k in ("seq_dir", "seq_classes", "seq_flank", "seq_width", "seq_gzip", "seq_fai")):
        sys.exit("--seq_dir belongs to predict, not evaluate")


def plan(args) -> Optional[SeqPlan]:
    """--seq_dir and its options, or None without the flag.  Everything that can be refused without the model is refused here
    (sys.exit), before any prediction."""
    sdir = getattr(args, "seq_dir", None)
    packed_out, fai = bool(getattr(args, "seq_gzip", False)), bool(getattr(args, "seq_fai", False))
    classes, flank, width = getattr(args, "seq_classes", None), getattr(args, "seq_flank", None), getattr(args, "seq_width", None)
    if sdir is None:
        if packed_out or fai or classes is not None or flank is not None or width is not None:
            sys.exit("--seq_classes, --seq_flank, --seq_width, --seq_gzip and --seq_fai need --seq_dir")
        return None
    if fai and packed_out:
        sys.exit("--seq_fai and --seq_gzip exclude each other: a .fai states offsets of the uncompressed file, a BGZF FASTA would "
                 "also need a .gzi index, which is not written")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or getattr(args, "split_contigs", False):
        sys.exit("--seq_dir: the repeat sequences of an input are written by one process, in TSV order; they cannot be written by "
                 "several ranks (WORLD_SIZE > 1, --split_contigs); run in one process")
    flank, width = (0 if flank is None else flank), (60 if width is None else width)
    if not 1 <= width <= MAX_WIDTH:
        sys.exit(f"--seq_width must lie in 1..2^30, not {width}")
    if flank < 0:
        sys.exit(f"--seq_flank must not be negative, got {flank}")
    from .outfiles import plan_inputs
    from .tracks import gzip_level, input_basename
    level = gzip_level(args, 1)

    def outputs_of(f):
        out = os.path.join(sdir, input_basename(f) + ".repeats.fa" + (".gz" if packed_out else ""))
        return (out, out + ".fai" if fai else None)

    files = plan_inputs("--seq_dir", args.FASTA, outputs_of, "repeat sequences", stdin="read a second time for the sequences",
                        npz="holds no sequence bytes to write", every_input=True, directory=sdir)
    return SeqPlan({f: outs[0] for f, outs in files.items()}, classes, flank, width, packed_out, fai, level)


def from_plan(p: SeqPlan, classes: int) -> "RepeatSeq":
    """The labels checked against the model's class count (sys.exit on one it lacks)."""
    bad = [c for c in (p.classes or ()) if not 0 < c < classes]
    if bad:
        sys.exit(f"--seq_classes: label {bad[0]} is not a repeat class of this model (labels 1..{classes - 1})")
    return RepeatSeq(p)


class RepeatSeq(RowsOutput):
    """--seq_dir as an output of `predict`: the FASTA of an input's repeats is written when the input is done, from all of its rows
    (write_repeat_fasta stages its files: renamed on success, removed on failure)."""

    def write(self, filename: str, rows, log) -> None:
        p, t0 = self.plan, time.perf_counter()
        final = p.files[filename]
        nbytes = write_repeat_fasta(filename, final, rows, classes=p.classes, flank=p.flank, width=p.width, compress=p.gzip,
                                    level=p.level, fai_path=final + ".fai" if p.fai else None)
        log.info("%s: %d bytes of FASTA, %d of %d rows, to %s in %.2f ms", filename, nbytes,
                 int(kept_rows(rows, class_bits(p.classes)).sum()), len(rows), final, (time.perf_counter() - t0) * 1e3)
