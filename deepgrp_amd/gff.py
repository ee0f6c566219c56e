"""GFF3 of the scored repeats (`predict --bed_dir DIR --bed_gff3`): for every input file one `DIR/<basename>.gff3` in the place of the
`.bed`, the same rows and the same four figures as the BED line (bed.py), as GFF3 feature lines.

The file.  Its first 16 bytes are `##gff-version 3\\n` (HEADER), also when the input has no row; no other pragma or comment line is
written anywhere.  Then one line per emitted row, in TSV order:

    seqid<TAB>deepgrp<TAB>repeat_region<TAB>start+1<TAB>end<TAB>mean<TAB>.<TAB>.<TAB>ID=r<j>;Name=<cname>;label=<L>;score=<score>;min=<min>;agree=<agree><LF>

start and end are the TSV's (GFF3 is 1-based and closed, hence start+1); score (0..1000), mean, min and agree (`d.dddd`) are the
BED line's figures, R(num, den, k) of bed.py; j is the 1-based ordinal of the line in the whole file, counted across records, batches
and writes (filtered rows do not count); seqid is the record's name (evaluation.record_name) with every byte outside
`[a-zA-Z0-9.:^*$@!+_?-|]` written %XX (`escape_seqid`); cname is `class<L>` or, with --bed_names, the entry of label L with the
bytes below 0x20, 0x7f and `%;=&,` written %XX (`escape_value`).  Both escapes are made here, on the host, once per write; the
device (dgrp_gff_text_batch) copies name bytes verbatim.  There is one formatter, on the device: the plain `.gff3` is its text read
back, `.gff3.gz` (--bed_gzip) the same text deflated there.

The tabix index (`.gff3.gz.tbi`, --bed_index) has the fields of htslib's `gff` preset (PRESET: format 0, sequence in column 1, begin
in column 4, end in column 5, meta `#`, skip 0): `reference_index` is tabix.reference_index under that preset -- lines that start
with `#` are skipped, a line's interval is [column 4 - 1, column 5), and the chunk and linear-index rules are unchanged.  The header
is a BGZF member of its own, so the first chunk begins at text offset 16, the first byte of the second member.

`reference_lines`, `reference_index_parts` and `reference_index` are the statements the device entries and `BedFiles` are tested
against, in Python integers and bytes only."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import tabix

HEADER = b"##gff-version 3\n"
PRESET = tabix.PRESET_GFF
MAX_NAME = 255                                      # bytes of a --bed_names entry

_SEQID_OK = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789.:^*$@!+_?-|")
_VALUE_BAD = frozenset(list(range(0x20)) + [0x7f] + list(b"%;=&,"))


def _raw(name) -> bytes:
    return name if isinstance(name, bytes) else name.encode("utf-8", "surrogateescape")


def escape_seqid(name) -> bytes:
    """Column 1: every byte outside [a-zA-Z0-9.:^*$@!+_?-|] as %XX, upper-case hex."""
    return b"".join(bytes([b]) if b in _SEQID_OK else b"%%%02X" % b for b in _raw(name))


def escape_value(value) -> bytes:
    """An attribute's value: the bytes below 0x20, 0x7f and `%;=&,` as %XX, upper-case hex."""
    return b"".join(b"%%%02X" % b if b in _VALUE_BAD else bytes([b]) for b in _raw(value))


def names_refusal(names: Sequence) -> Optional[str]:
    """Why --bed_names cannot be these names (an empty one, one above MAX_NAME bytes), or None."""
    for i, nm in enumerate(names):
        if not _raw(nm):
            return f"--bed_names: the name of label {i + 1} is empty"
        if len(_raw(nm)) > MAX_NAME:
            return f"--bed_names: the name of label {i + 1} has {len(_raw(nm))} bytes, above {MAX_NAME}"
    return None


class GffText(NamedTuple):
    """What one write adds to the file once its first ordinal is known: `data` (the text of a plain `.gff3`, the BGZF members without
    EOF member of a `.gff3.gz`), the lines in it and, with --bed_index, the arrays of ContigPipeline.gff_index_batch."""
    data: bytes
    lines: int
    chunks: Optional[np.ndarray] = None
    linear: Optional[np.ndarray] = None
    wpref: Optional[np.ndarray] = None
    last_end: Optional[np.ndarray] = None


class GffWrite(NamedTuple):
    """One write (a record, or a batch) of a GFF3 file: the records' names as they come (not escaped), why this input cannot have
    an index, and `render(id0) -> GffText`, called by `BedFiles.write` with the lines the file holds so far -- the ordinals run
    through the file, so a write's text exists only when the writes in front of it are counted.  render None: no row."""
    names: List[bytes]
    refused: Optional[str] = None
    render: Optional[Callable[[int], GffText]] = None


# ---- the statements ------------------------------------------------------------------------------------------------------------------
def reference_lines(names: Sequence, by_contig: bool, rows, scores, min_score: int = 0, class_names: Optional[Sequence] = None,
                    id0: int = 0) -> Tuple[bytes, int]:
    """The feature lines (no header) in Python integers -> (text, lines): names and class_names as they come, escaped here."""
    from .bed import ONE, _half_up
    if id0 < 0:
        raise ValueError("id0 below 0")
    seqids = [escape_seqid(nm) for nm in names]
    cnames = None if class_names is None else [escape_value(nm) for nm in class_names]
    out = []
    for row, sc in zip(rows, scores):
        total, bases, agree, qmin = int(sc["sum"]), int(sc["bases"]), int(sc["agree"]), int(sc["qmin"])
        if bases <= 0:
            raise ValueError("a row without a scored base")
        score = _half_up(total, bases << 24, 1000)
        if score < min_score:
            continue
        mean, low, agr = (b"%d.%04d" % divmod(f, 10000) for f in
                          (_half_up(total, bases << 24, 10000), _half_up(qmin, ONE, 10000), _half_up(agree, bases, 10000)))
        label = int(row["label"])
        if cnames is None:
            cname = b"class%d" % label
        elif 1 <= label <= len(cnames):
            cname = cnames[label - 1]
        else:
            raise ValueError(f"label {label} outside the {len(cnames)} class names")
        out.append(b"%s\tdeepgrp\trepeat_region\t%d\t%d\t%s\t.\t.\tID=r%d;Name=%s;label=%d;score=%d;min=%s;agree=%s\n"
                   % (seqids[int(row["contig"]) if by_contig else 0], int(row["start"]) + 1, int(row["end"]), mean, id0 + len(out) + 1,
                      cname, label, score, low, agr))
    return b"".join(out), len(out)


def reference_index_parts(names: Sequence, by_contig: bool, rows, scores, min_score: int, rec_end: Sequence[int],
                          class_names: Optional[Sequence] = None, id0: int = 0, depth: int = 5):
    """bed.reference_index_parts for the text `reference_lines` gives for the same arguments: what dgrp_gff_index_batch states
    (with another depth: dgrp_gff_csi_batch).
    The intervals are the rows' [start, end); only the line lengths differ from the BED's."""
    from .tabix import CHUNK_DTYPE, MIN_SHIFT, csi_reg2bin, window_prefix
    nrec = len(rec_end)
    wpref = window_prefix(rec_end, depth)
    linear = np.full(int(wpref[-1]), -1, np.int64)
    filled = [0] * nrec
    last_end = np.zeros(nrec, np.int64)
    chunks, u, done = [], 0, 0
    for k in range(len(rows)):
        line, n = reference_lines(names, by_contig, rows[k:k + 1], scores[k:k + 1], min_score, class_names, id0 + done)
        if not n:
            continue
        done += 1
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


def reference_index(gz_bytes: bytes) -> bytes:
    """The `.tbi` payload of a finished `.gff3.gz`, from the file alone (tabix.reference_index under the `gff` preset)."""
    return tabix.reference_index(gz_bytes, PRESET)


def read_index(pl: bytes) -> dict:
    """tabix.read_index of a payload of the `gff` preset."""
    return tabix.read_index(pl, PRESET)


def query(index: dict, gz_bytes: bytes, seqid: bytes, beg: int, end: int) -> List[bytes]:
    """The feature lines of `seqid` that overlap the zero-based half-open [beg, end), found through the index (tabix.query)."""
    return tabix.query(index, gz_bytes, seqid, beg, end, PRESET)


def header_member(level: int) -> bytes:
    """HEADER as the BGZF member a `.gff3.gz` begins with (the library's host encoder, as the device writes the members behind it)."""
    from .gz import bgzf_compress_host
    return bgzf_compress_host(HEADER, eof=False, level=level)
