"""Masked FASTA output (`predict --mask_dir`): a copy of the input file whose sequence bytes state the prediction -- soft (inside a
masked TSV row lower case, every other letter upper case, as RepeatMasker -xsmall) or hard (inside a row 'N').  The copy has the
input's length; headers, line ends, text before the first header and records without a header are copied byte for byte.

A record's sequence position p is the p-th character of the sequence the reference's line loop builds (deepgrp/__main__.py:20-43),
the coordinate of the TSV rows.  Plain records (fasta.py's device path: LF / CRLF line ends only) are rewritten on the GPU
(dgrp_fasta_mask_batch, in place on the uploaded bytes); the others through `sequence_byte_offsets`, the byte-level mirror of
fasta.LineLoop."""
from __future__ import annotations

import argparse
import logging
import mmap
import os
import re
import sys
import tempfile
import time
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .outfiles import RowsOutput, class_list

_LOG = logging.getLogger(__name__)

MODES = {"soft": 0, "hard": 1}
_STRIP = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"            # what str.strip() removes from an ASCII line
_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)?")          # one line of text mode's universal newlines, terminator included
_IS_LETTER = np.zeros(256, bool)
_IS_LETTER[65:91] = _IS_LETTER[97:123] = True


def class_bits(classes: Optional[Iterable[int]]) -> int:
    """The class mask of dgrp_fasta_mask_batch: bit c set for every label c to mask; None = every label > 0."""
    if classes is None:
        return ((1 << 64) - 1) & ~1
    bits = 0
    for c in classes:
        c = int(c)
        if not 0 < c < 64:
            raise ValueError(f"class {c} cannot be masked (labels 1..63)")
        bits |= 1 << c
    return bits


def _text_encoding() -> str:
    """The encoding `open(path, "r")` reads with (fasta._text_lines)."""
    from .fasta import _text_lines
    return _text_lines(b"").encoding


def sequence_byte_offsets(chunk: bytes) -> List[Tuple[str, Optional[np.ndarray]]]:
    """The records fasta.LineLoop yields from this piece of a file (a chunk: it starts at the file start or with a '>' line), in
    order, as (header, offsets): `offsets` are the positions in `chunk` of the record's sequence characters in the reference's order,
    so that bytes(chunk[offsets]).upper() is the sequence the loop builds -- or None when a sequence line of the record is not ASCII
    (its characters are not bytes).  Lines as text mode splits them (LF, CRLF, lone CR), each stripped as str.strip() strips; a blank
    line raises IndexError as the loop does."""
    enc = None
    out: List[Tuple[str, Optional[np.ndarray]]] = []
    header, parts, ascii_ok = "", [], True

    def close():
        if header:
            out.append((header, (np.concatenate(parts) if parts else np.zeros(0, np.int64)) if ascii_ok else None))

    pos, n = 0, len(chunk)
    while pos < n:
        m = _LINE.match(chunk, pos)
        line_end = m.end()
        content = chunk[pos:line_end].rstrip(b"\r\n")
        start = pos
        pos = line_end
        if content.isascii():
            body = content.strip(_STRIP)
            if not body:
                raise IndexError("string index out of range")          # the reference loop's blank line
            lead = len(content) - len(content.lstrip(_STRIP))
            if body[0] == 62:
                close()
                header, parts, ascii_ok = body[1:].decode("ascii"), [], True
            else:
                parts.append(np.arange(start + lead, start + lead + len(body), dtype=np.int64))
        else:
            enc = enc or _text_encoding()
            text = content.decode(enc, "surrogateescape").strip()
            if not text:
                raise IndexError("string index out of range")
            if text[0] == ">":
                close()
                header, parts, ascii_ok = text[1:], [], True
            else:
                ascii_ok = False
    close()
    return out


def _paint(n: int, rows: np.ndarray, bits: int, what: str) -> np.ndarray:
    """Per sequence position of a record of n characters: inside a row whose label is in the mask."""
    edge = np.zeros(n + 1, np.int32)
    if rows.size:
        st, en = rows["start"].astype(np.int64), rows["end"].astype(np.int64)
        if (st < 0).any() or (en <= st).any() or (en > n).any():
            raise ValueError(f"{what}: a row lies outside its sequence of {n} characters")
        lab = rows["label"].astype(np.int64)
        ok = (lab >= 0) & (lab < 64)
        sel = ok & ((np.uint64(bits) >> np.where(ok, lab, 0).astype(np.uint64)) & np.uint64(1)).astype(bool)
        np.add.at(edge, st[sel], 1)
        np.add.at(edge, en[sel], -1)
    return np.cumsum(edge[:n]) > 0


def _apply_host(buf: np.ndarray, pos: np.ndarray, inside: np.ndarray, mode: int) -> None:
    """Mask the bytes buf[pos] (inside[i] for buf[pos[i]]) as dgrp_fasta_mask_batch does."""
    b = buf[pos]
    if mode == 1:
        b = np.where(inside, np.uint8(78), b)
    else:
        letter = _IS_LETTER[b]
        b = np.where(letter, np.where(inside, b | 0x20, b & 0xDF), b).astype(np.uint8)
    buf[pos] = b


def _pwrite_all(fd: int, data, offset: int) -> None:
    view = memoryview(data).cast("B")
    done = 0
    while done < len(view):
        done += os.pwrite(fd, view[done:], offset + done)


def mask_fasta(fasta_path, out_path, rows, mode: str = "soft", classes: Optional[Iterable[int]] = None,
               ranges: Optional[Sequence[Tuple[int, int]]] = None, group_bytes: int = 256 << 20, group_records: int = 4096,
               compress: bool = False, level: int = 0, twobit: bool = False) -> int:
    """Write the masked copy of `fasta_path`.  `rows` (pipeline.SEGMENT_DTYPE): the TSV rows, `contig` = the record's ordinal among
    the records the reference loop yields from the processed bytes, in file order.  `classes`: the labels to mask (None: every label
    > 0).  `ranges=None`: the whole file goes to `out_path` (created or truncated to the input's size); else only those byte ranges
    (whole chunks, as fasta.ingest_ranges takes them) are processed and written into the existing `out_path`, which must already
    have the input's size -- ranks of a sharded run each write their own share.  Works in groups as the ingest does: one upload,
    dgrp_fasta_encode_batch (which tells the plain records), dgrp_fasta_mask_batch in place, one read-back, one write.
    A gzip-compressed `fasta_path` (no `ranges`) is masked as its inflated text (gz.open_inflated: BGZF members inflated on the
    device, other gzip through zlib), resident on the device.  `compress=True` (no `ranges`): `out_path` becomes a BGZF file of the
    masked text -- every group is deflated on the device where it was masked (gz.bgzf_compress_device at `level`: 0 literals only,
    1 with matches) and its members are appended, the EOF member behind the last; a group boundary is just a short member.  A UCSC
    .2bit `fasta_path` (no `ranges`) is masked as the text of the file (twobit.open_text: built on the device by
    dgrp_twobit_text_batch), which takes the place inflated gzip text takes.  `twobit=True` (no `ranges`, no `compress`):
    `out_path` becomes the 2bit file of the masked text (twobit.py states it) -- every group stays on the device where it was masked,
    its plain records are packed there (dgrp_twobit_pack_batch) and only their blobs are read back and spooled; records of the host
    path are packed by twobit.pack_record from the host-masked bytes; header and index are written when the input is done.
    twobit.Refused where the input has no 2bit file.  Returns the number of records seen."""
    import torch

    import contextlib

    from . import gz
    from . import twobit as tbit
    from ._lib import check, lib
    from .fasta import RESIDENT_BYTES, _chunk_groups, _upload_file
    from .pipeline import SEGMENT_DTYPE, require_gpu, stream_ptr

    if mode not in MODES:
        raise ValueError(f"mask mode must be one of {sorted(MODES)}, not {mode!r}")
    if level not in gz.LEVELS:
        raise ValueError(f"compression level must be one of {gz.LEVELS}, not {level!r}")
    mcode, bits = MODES[mode], class_bits(classes)
    rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
    rows = rows[np.lexsort((rows["start"], rows["contig"]))] if rows.size else rows
    contig = rows["contig"]
    packed = gz.is_gzip(fasta_path)
    if ranges is not None and (packed or compress):
        raise ValueError(f"{fasta_path}: a compressed input or output has no byte ranges to share out; it is masked whole")
    if twobit and (ranges is not None or compress):
        raise ValueError(f"{fasta_path}: a 2bit masked copy is written whole by one process and is not compressed")
    text = d_text = None
    if packed:
        text, d_text, size = gz.open_inflated(fasta_path, RESIDENT_BYTES, require_gpu, _upload_file)
    elif tbit.is_twobit(fasta_path):
        if ranges is not None:
            raise ValueError(f"{fasta_path}: a 2bit input has no byte ranges of FASTA text to share out; it is masked whole")
        # the masked copy is the text of the file (twobit.py), built on the device: from here on as inflated gzip text
        packed = True
        text, d_text, size = tbit.open_text(fasta_path, RESIDENT_BYTES, require_gpu, _upload_file)
    else:
        size = os.path.getsize(fasta_path)
    if twobit:
        if size == 0:
            tbit.write_file([], [], out_path, what=str(fasta_path))
        ranges = [(0, size)] if size else []
    elif ranges is None:
        with open(out_path, "wb") as fh:
            if compress and size == 0:
                fh.write(gz.BGZF_EOF)
            elif not compress:
                fh.truncate(size)
        ranges = [(0, size)] if size else []
    elif os.path.getsize(out_path) != size:
        raise ValueError(f"{out_path}: {os.path.getsize(out_path)} bytes, the input has {size}")
    if size == 0:
        return 0
    L = lib()
    dev = require_gpu()
    written = 0                                                 # compress: bytes of out_path so far

    def rows_of(k):
        lo, hi = np.searchsorted(contig, [k, k + 1])
        return lo, hi

    ordinal = 0
    fd = None if twobit else os.open(out_path, os.O_WRONLY)
    names, sizes = [], []                                       # twobit: the records so far, their blobs in `spool`
    try:
        with contextlib.ExitStack() as stack:
            if twobit:
                import tempfile
                spool = stack.enter_context(tempfile.TemporaryFile(dir=os.path.dirname(os.path.abspath(out_path))))
            if packed:
                mm = text
            else:
                fh = stack.enter_context(open(fasta_path, "rb"))
                mm = stack.enter_context(mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_COPY))
            for r0, r1 in ranges:
                if not (0 <= r0 < r1 <= size) or (r0 and not (mm[r0] == 62 and mm[r0 - 1] == 10)):
                    raise ValueError(f"{fasta_path}: [{r0}, {r1}) is not a range of whole chunks")
                for grp in _chunk_groups(L, dev, fasta_path, mm, r0, r1, group_bytes, group_records, keep_raw=True, d_file=d_text):
                    g0, g1 = grp.starts[grp.c0], grp.starts[grp.c1]
                    dev_recs, host_chunks = [], []              # (i, ordinal); (chunk start, chunk end, [(header, offsets, ordinal)])
                    dev_names = []                              # twobit: the names of dev_recs
                    for i, c in enumerate(range(grp.c0, grp.c1)):
                        a, b = grp.starts[c], grp.starts[c + 1]
                        if grp.plain(i):
                            header = mm[r0 + a:r0 + grp.head_ends[c]].decode("ascii").strip()[1:]
                            if header:
                                dev_recs.append((i, ordinal))
                                if twobit:
                                    dev_names.append(tbit.record_name(header))
                                ordinal += 1
                            continue
                        recs = []
                        for header, offs in sequence_byte_offsets(mm[r0 + a:r0 + b]):
                            recs.append((header, offs, ordinal))
                            ordinal += 1
                        if recs:
                            host_chunks.append((a, recs))
                    d_raw = grp.d_raw
                    if dev_recs:
                        # d_raw may be a view of the resident range at any offset: the kernel takes the 16-byte aligned address below
                        # it (inside the same allocation) and offsets that include the difference
                        ptr = d_raw.data_ptr()
                        shift = ptr & 15
                        h_off = np.array([grp.body0s[i] - g0 + shift for i, _k in dev_recs], np.int64)
                        h_len = np.array([grp.starts[grp.c0 + i + 1] - grp.body0s[i] for i, _k in dev_recs], np.int64)
                        spans = [rows_of(k) for _i, k in dev_recs]
                        h_row_off = np.zeros(len(dev_recs) + 1, np.int64)
                        np.cumsum([hi - lo for lo, hi in spans], out=h_row_off[1:])
                        sel = np.concatenate([rows[lo:hi] for lo, hi in spans]) if h_row_off[-1] else np.zeros(0, SEGMENT_DTYPE)
                        d_rows = torch.from_numpy(sel.view(np.uint8)).to(dev) if sel.size else None
                        wb = L.dgrp_fasta_mask_workspace_bytes(len(dev_recs), int(h_len.sum()), int(h_row_off[-1]))
                        work = torch.empty(wb, dtype=torch.uint8, device=dev)
                        check(L.dgrp_fasta_mask_batch(ptr - shift, len(dev_recs), h_off.ctypes.data, h_len.ctypes.data,
                                                      d_rows.data_ptr() if d_rows is not None else None, h_row_off.ctypes.data,
                                                      mcode, bits, ptr - shift, work.data_ptr(), wb, stream_ptr()),
                              f"dgrp_fasta_mask_batch ({fasta_path})")
                        del work, d_rows
                    if twobit:
                        blobs = {}                              # ordinal -> (name, blob)
                        if dev_recs:
                            if int(h_len.sum()) > 0xFFFFFFFF:
                                raise tbit.Refused(f"{fasta_path}: record {dev_recs[0][1]} ({dev_names[0]!r}) has more than 2^32 - 1 "
                                                   "bases; a 2bit record cannot hold it")
                            d_blobs, _counts, blob_off = tbit.pack_device(ptr - shift, h_off, h_len, dev,
                                                                          f"dgrp_twobit_pack_batch ({fasta_path})")
                            h_blobs = d_blobs[:int(blob_off[-1])].cpu().numpy()
                            for j, (_i, k) in enumerate(dev_recs):
                                blobs[k] = (dev_names[j], h_blobs[blob_off[j]:blob_off[j + 1]])
                            del d_blobs
                        if host_chunks:                         # these records only go through the host
                            host = (d_raw.cpu().numpy() if packed else
                                    np.frombuffer(mm, dtype=np.uint8, count=g1 - g0, offset=r0 + g0).copy())
                            for a, recs in host_chunks:
                                for header, offs, k in recs:
                                    if offs is None:
                                        raise tbit.Refused(f"{fasta_path}: record {header!r} has sequence lines that are not ASCII; "
                                                           "it has no 2bit form")
                                    lo, hi = rows_of(k)
                                    inside = _paint(offs.size, rows[lo:hi], bits, f"{fasta_path}: record {header!r}")
                                    _apply_host(host, offs + (a - g0), inside, mcode)
                                    blobs[k] = (tbit.record_name(header, _text_encoding()), tbit.pack_record(host[offs + (a - g0)]))
                            del host
                        del grp, d_raw
                        for k in sorted(blobs):
                            name, blob = blobs[k]
                            names.append(name)
                            sizes.append(len(blob))
                            spool.write(memoryview(blob))
                        continue
                    host = None
                    if compress and not host_chunks:
                        pass                                    # the group stays on the device
                    elif dev_recs or packed:
                        host = d_raw.cpu().numpy()
                    else:
                        host = np.frombuffer(mm, dtype=np.uint8, count=g1 - g0, offset=r0 + g0).copy()
                    if not compress:
                        d_raw = None
                    del grp
                    for a, recs in host_chunks:
                        for header, offs, k in recs:
                            lo, hi = rows_of(k)
                            if offs is None:
                                _LOG.warning("%s: record %r has sequence lines that are not ASCII; copied unmasked", fasta_path, header)
                                continue
                            inside = _paint(offs.size, rows[lo:hi], bits, f"{fasta_path}: record {header!r}")
                            _apply_host(host, offs + (a - g0), inside, mcode)
                    if compress:
                        # (a group with host-masked records went down, was patched and goes up again: rare)
                        d_comp = gz.bgzf_compress_device(d_raw if host is None else torch.from_numpy(host).to(dev), eof=False,
                                                         level=level)
                        comp = d_comp.cpu().numpy()
                        _pwrite_all(fd, comp, written)
                        written += comp.size
                        del d_comp, comp
                    else:
                        _pwrite_all(fd, host, r0 + g0)
                    del host, d_raw
            if twobit and size:
                def pieces():
                    spool.seek(0)
                    while True:
                        piece = spool.read(64 << 20)
                        if not piece:
                            return
                        yield piece
                tbit.write_file(names, pieces(), out_path, sizes=sizes, what=str(fasta_path))
        if compress:
            _pwrite_all(fd, gz.BGZF_EOF, written)
    finally:
        if fd is not None:
            os.close(fd)
    if contig.size and int(contig[-1]) >= ordinal:
        raise ValueError(f"{fasta_path}: rows name record {int(contig[-1])}, but only {ordinal} records were read")
    return ordinal


# ------------------------------------------------------------------------- the output of `predict`
class MaskPlan(NamedTuple):
    files: dict                                     # input file -> its masked copy
    mode: str                                       # --mask: soft or hard
    classes: Optional[Tuple[int, ...]]              # --mask_classes (None: every label > 0)
    gzip: bool = False                              # --mask_gzip
    twobit: bool = False                            # --mask_twobit
    level: int = 0                                  # --gzip_level of --mask_gzip


def add_options(parser) -> None:
    """The masking flags: on `predict` and, for the README form with the flags in front, on the main parser as well (the values
    are only set where given, so neither parser's default hides the other's)."""
    s = argparse.SUPPRESS
    parser.add_argument("--mask_dir", type=str, default=s,
                        help="(addition) also write a masked copy of every input FASTA file as DIR/<basename of the input>")
    parser.add_argument("--mask", choices=("soft", "hard"), default=s,
                        help="(addition) soft: predicted repeats lower case, the rest upper case; hard: predicted repeats 'N'")
    parser.add_argument("--mask_classes", type=class_list, default=s,
                        help="(addition) comma-separated labels to mask, e.g. 1,3 (default: every label > 0)")
    parser.add_argument("--mask_gzip", action="store_true", default=s,
                        help="(addition) with --mask_dir: write every masked copy as BGZF (bgzip's format, deflated on the GPU) to "
                             "DIR/<basename>.gz, and accept gzip-compressed inputs; one process only")
    parser.add_argument("--mask_twobit", action="store_true", default=s,
                        help="(addition) with --mask_dir: write every masked copy as a UCSC .2bit file (soft mask = mask blocks, hard "
                             "mask = N blocks; packed on the GPU) to DIR/<basename>.2bit instead of FASTA text, and accept "
                             "gzip-compressed inputs; one process only")
    parser.add_argument("--gzip_level", type=int, default=s,
                        help="(addition) level of the GPU deflate of --mask_gzip, --track_gzip, --track_bigwig, --bed_gzip and --bed_bigbed: 0 "
                             "literals "
                             "only, 1 with matches (default: 0 for masked copies, 1 for tracks and the BED)")


def refuse_on_evaluate(args) -> None:
    if getattr(args, "mask_twobit", False):
        sys.exit("--mask_twobit belongs to predict, not evaluate")
    if getattr(args, "mask_dir", None) is not None or getattr(args, "mask_gzip", False):
        sys.exit("--mask_dir belongs to predict, not evaluate")
    if getattr(args, "gzip_level", None) is not None:
        sys.exit("--gzip_level belongs to predict, not evaluate")


def plan(args) -> Optional[MaskPlan]:
    """--mask_dir and its options, or None without the flag.  Everything that can be refused without the model is refused here
    (sys.exit), before any prediction."""
    mdir = getattr(args, "mask_dir", None)
    packed_out = bool(getattr(args, "mask_gzip", False))
    twobit_out = bool(getattr(args, "mask_twobit", False))
    if mdir is None:
        if twobit_out:
            sys.exit("--mask_twobit needs --mask_dir")
        if getattr(args, "mask", None) is not None or getattr(args, "mask_classes", None) is not None or packed_out:
            sys.exit("--mask, --mask_classes and --mask_gzip need --mask_dir")
        return None
    if twobit_out and packed_out:
        sys.exit("--mask_twobit and --mask_gzip exclude each other: a 2bit file is a binary format of its own and is not compressed")
    if packed_out and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or getattr(args, "split_contigs", False)):
        sys.exit("--mask_gzip: a compressed masked copy cannot be written by several ranks (WORLD_SIZE > 1, --split_contigs): "
                 "they share a file out by byte ranges, and a compressed file has none; run in one process")
    if twobit_out and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or getattr(args, "split_contigs", False)):
        sys.exit("--mask_twobit: a 2bit masked copy cannot be written by several ranks (WORLD_SIZE > 1, --split_contigs): "
                 "they share a file out by byte ranges, and a 2bit file has none of the input's; run in one process")
    from .gz import compressed_inputs
    from .outfiles import plan_inputs
    from .twobit import is_twobit

    def copy_of(f):
        if not packed_out and not twobit_out and compressed_inputs([f]):
            sys.exit(f"--mask_dir: {f} is gzip-compressed; the masked copy is written by byte offsets of the input, so give the "
                     "uncompressed FASTA or pass --mask_gzip")
        base = os.path.basename(f)
        if twobit_out:
            # chr.fa -> chr.fa.2bit, hg38.fa.gz -> hg38.fa.2bit, hg38.2bit -> hg38.2bit
            if base.endswith(".gz") and compressed_inputs([f]):
                base = base[:-3]
            if not base.endswith(".2bit"):
                base += ".2bit"
        elif is_twobit(f):
            base += ".fa"                                     # the masked copy of a 2bit file is its FASTA text
        if packed_out and not base.endswith(".gz"):
            base += ".gz"
        return os.path.join(mdir, base)

    files = plan_inputs("--mask_dir", args.FASTA, copy_of, "masked copies", "masked copy", stdin="masked", npz="cannot be masked",
                        directory=mdir)
    return MaskPlan(files, getattr(args, "mask", None) or "soft", getattr(args, "mask_classes", None), packed_out, twobit_out,
                    getattr(args, "gzip_level", None) or 0)


def from_plan(p: MaskPlan, classes: int) -> "Mask":
    """The labels checked against the model's class count (sys.exit on one it lacks)."""
    bad = [c for c in (p.classes or ()) if not 0 < c < classes]
    if bad:
        sys.exit(f"--mask_classes: label {bad[0]} is not a repeat class of this model (labels 1..{classes - 1})")
    return Mask(p)


class Mask(RowsOutput):
    """--mask_dir as an output of `predict`: the masked copy of an input is written when the input is done, from all of its rows."""

    def write(self, filename: str, rows, log) -> None:
        t0 = time.perf_counter()
        write_mask(filename, self.plan.files[filename], rows, self.plan, log)
        log.debug("%s: masked copy %s in %.2f ms", filename, self.plan.files[filename], (time.perf_counter() - t0) * 1e3)


def write_mask(filename: str, final: str, rows, p: MaskPlan, log=_LOG) -> None:
    """The masked copy of one file: written to a temporary file next to `final`, renamed on success, removed on failure.
    --mask_twobit: an input that has no 2bit file (twobit.Refused) gets one warning and no file; the command goes on."""
    from .twobit import Refused
    fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(final) + ".", suffix=".tmp", dir=os.path.dirname(final) or ".")
    os.close(fd)
    try:
        if p.twobit:
            mask_fasta(filename, tmp, rows, mode=p.mode, classes=p.classes, twobit=True)
        else:
            mask_fasta(filename, tmp, rows, mode=p.mode, classes=p.classes, compress=p.gzip, level=p.level)
        os.replace(tmp, final)
    except Refused as e:
        os.remove(tmp)
        log.warning("--mask_twobit: %s; no %s is written", e, final)
    except BaseException:
        os.remove(tmp)
        raise


def write_mask_sharded(filename: str, final: str, rows, spans, p: MaskPlan) -> None:
    """write_mask over the ranks: rank 0 creates the temporary file at the input's size, every rank writes its byte ranges,
    rank 0 renames it (or removes it when any rank failed)."""
    import torch.distributed as dist

    from .distributed import raise_together
    rank = dist.get_rank()
    name = [None]
    err = None
    if rank == 0:
        try:
            fd, tmp = tempfile.mkstemp(prefix="." + os.path.basename(final) + ".", suffix=".tmp", dir=os.path.dirname(final) or ".")
            os.ftruncate(fd, os.path.getsize(filename))
            os.close(fd)
            name = [tmp]
        except Exception as e:              # noqa: BLE001 -- re-raised on every rank together
            err = e
    raise_together(err)
    dist.broadcast_object_list(name, src=0)          # (after rank 0 made the file: the barrier in front of the writes)
    tmp = name[0]
    try:
        if spans:
            mask_fasta(filename, tmp, rows, mode=p.mode, classes=p.classes, ranges=spans)
    except Exception as e:                  # noqa: BLE001
        err = e
    try:
        raise_together(err)                 # every rank has written (or failed): the barrier behind the writes
    except BaseException:
        if rank == 0:
            os.remove(tmp)
        raise
    if rank == 0:
        os.replace(tmp, final)
