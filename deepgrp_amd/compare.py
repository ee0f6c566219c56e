"""`compare`: the reports of `evaluate` for rows that are already on disk -- the TSV `predict` (or the reference) wrote, the calls of
another tool as a table `contig begin end number`, or a RepeatMasker listing -- against an annotation.  No model is loaded and no
forward pass runs: the inputs are read only for their records, their names and the evaluated span of each.

PREDICTED, four forms (sniffed on the first 64 KiB: `tsv`, then `gff3` where the first line begins with `##gff-version 3`, then
`repeatmasker`, else `table`):
    tsv           fields between tabs: the first is the file, the last three are start, end and label, what lies between is the
                  header and may hold tabs.  The record a row belongs to is evaluation.record_name's rule on (file, header) without
                  the `isfile` test (`tsv_name`).  An empty line is skipped; fewer than five fields are an AnnotationError.  A label
                  outside 1..C-1 is an AnnotationError naming file and line; one name under two file fields is refused.
    table         evaluation.read_annotation's grammar; a row whose number is outside 1..C-1 is dropped and counted.
    repeatmasker  annotation.read_listing; likewise.
    gff3          gffin.py: feature lines, the label looked up by name (--predicted_names, --gff_key, --gff_by_type); likewise.
`tsv` and `table` are parsed on the device (dgrp_rows_parse, csrc/rows_parse_kernels.hip).  What the device does not
decide -- a byte outside 0x20..0x7e other than tab and line feed, a carriage return that no line feed follows, a number that is not
1..18 plain digits -- goes to the host whole: `read_annotation` itself for a table, `tsv_flat_host` below for a TSV, which is also
the statement the device path is tested against.  A malformed line or an end below its begin is reported by the host path too, in
its own words.

FLATTENING makes foreign rows safe for every report: the predicted rows of a record are painted onto its evaluated span
(dgrp_paint_rows_batch: the smallest label wins, clipped to the span) and the rows that are scored are the runs of that track as
dgrp_segments extracts them -- the rows `predict` would have written for that label track, the last base a row of its own.  The rows
of a `predict` TSV come back unchanged; overlapping, nested, unsorted or abutting rows become ascending and disjoint.
`flatten_reference` is the numpy statement."""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import annotation as dgann

PREDICTED_FORMATS = ("auto", "tsv", "table", "repeatmasker", "gff3")
ANNOTATION_FORMATS = dgann.FORMATS
MIN_CLASSES, MAX_CLASSES, DEFAULT_CLASSES = 2, 64, 5
MIN_ROW_BYTES = 8                        # the shortest line dgrp_rows_parse keeps: n // 8 + 1 rows always suffice
REASONS = {1: "expected contig, begin, end and repeat number", 2: "expected file, header, start, end and label between tabs"}
GROUP_RECORDS = 4096                     # records of one work item
GROUP_BASES = 1 << 26                    # bases of one work item of several records


class NoPredictedError(ValueError):
    """Not one predicted row names a record of the inputs."""


class Flat(NamedTuple):
    """Rows in file order: begin, end, number, line (int64); run r is rows run_first[r] .. run_first[r + 1], named run_names[r] and,
    for a TSV, under the file field run_files[r] (else None); lines: the lines of the file; route: "device" or "host"."""
    begin: np.ndarray
    end: np.ndarray
    number: np.ndarray
    line: np.ndarray
    run_first: np.ndarray
    run_names: List[str]
    run_files: Optional[List[str]]
    lines: int
    route: str


class Predicted(dict):
    """{record name: SEGMENT_DTYPE rows} in file order; `lines[name]`: the line of every row (None: a table read on the host);
    `format`, `route` ("device", "host"); `rows_read`: the rows of the file, `rows_dropped`: those with a number outside 1..C-1."""
    lines: Optional[Dict[str, np.ndarray]] = None
    format: str = "tsv"
    route: str = "host"
    rows_read: int = 0
    rows_dropped: int = 0


# ---------------------------------------------------------------- sniffing
def _is_tsv_line(line: str) -> bool:
    f = line.split("\t")
    if not (len(f) >= 5 and all(x.isascii() and x.isdigit() for x in f[-3:])):
        return False
    return len(f) < 13 or dgann.parse_rm.parse_line(line).ctg is None    # (a row of a UCSC rmsk table may end in three digit fields)


def sniff_predicted(path) -> str:
    """"tsv" when every one of the first 16 non-empty lines has at least five tab fields whose last three are digits (and is no row
    of a UCSC rmsk table, whose repEnd, repLeft and id may all be digits); else annotation.sniff's answer, "repeatmasker" or
    "table".  Decided on the first 64 KiB (inflated when the magic bytes say gzip)."""
    head = dgann._head(path)
    lines = head.decode("utf-8", "replace").replace("\r\n", "\n").split("\n")
    if len(head) >= dgann.SNIFF_BYTES and lines:
        lines.pop()                                                  # (cut somewhere)
    seen = [ln for ln in lines if ln][:dgann.SNIFF_LINES]
    if seen and all(_is_tsv_line(ln) for ln in seen):
        return "tsv"
    return dgann.sniff(path)


def resolve_predicted_format(path, fmt: str) -> str:
    if fmt not in PREDICTED_FORMATS:
        raise ValueError(f"predicted format {fmt!r}: one of {', '.join(PREDICTED_FORMATS)}")
    return sniff_predicted(path) if fmt == "auto" else fmt


# ---------------------------------------------------------------- the host statement of the TSV
def tsv_name(file: str, header: str) -> str:
    """evaluation.record_name without the `isfile` test: the rows were written elsewhere, the file need not be here."""
    if file.endswith(".npz"):
        return os.path.basename(file).split(".")[0]
    words = header.split()
    return words[0] if words else ""


def _host_bytes(path) -> bytes:
    from . import gz
    with open(path, "rb") as fh:
        data = fh.read()
    return bytes(gz.inflate_host(data, path, 1 << 62)) if data[:2] == gz.MAGIC else data


def _host_lines(path) -> List[str]:
    """The lines as `open(path, "r", errors="surrogateescape")` reads them (universal newlines), split at line feeds alone."""
    import io
    text = io.StringIO(_host_bytes(path).decode("utf-8", "surrogateescape"), newline=None).read()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def tsv_flat_host(path) -> Flat:
    """The TSV rule of the module docstring, line by line: the host path, and the statement dgrp_rows_parse's format 1 is tested against."""
    from .evaluation import _bad
    lines = _host_lines(path)
    keys, vals = [], []
    for k, line in enumerate(lines, 1):
        if line == "":
            continue
        f = line.split("\t")
        if len(f) < 5:
            raise _bad(path, k, line, REASONS[2])
        row = []
        for what, tok in zip(("start", "end", "label"), f[-3:]):
            try:
                row.append(int(np.int64(int(tok))))
            except (ValueError, OverflowError):
                raise _bad(path, k, line, f"{what} {tok!r} is not an integer") from None
        keys.append((tsv_name(f[0], "\t".join(f[1:-3])), f[0]))
        vals.append(row + [k])
    a = np.asarray(vals, np.int64).reshape(-1, 4)
    first = [i for i in range(len(keys)) if i == 0 or keys[i] != keys[i - 1]]
    return Flat(a[:, 0], a[:, 1], a[:, 2], a[:, 3], np.asarray(first + [len(keys)], np.int64), [keys[i][0] for i in first],
                [keys[i][1] for i in first], len(lines), "host")


# ---------------------------------------------------------------- the device parser
def rows_parse_device(d_text, n: Optional[int] = None, tsv: bool = False, cap: Optional[int] = None, out=None):
    """dgrp_rows_parse on the uint8 device tensor `d_text` (its first `n` bytes): -> (counts = [lines, rows, runs, not-decided flag,
    first malformed line, its reason], the device arrays begin, end, number, name_pos, name_len, file_pos, file_len, line, run_first
    of `cap` rows -- default n // 8 + 1; `out`: use these instead --, the return code).  Nothing is raised for DGRP_ENOMEM (-3: more
    rows than `cap`; counts[1] tells the need)."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    n = int(d_text.numel()) if n is None else int(n)
    dev = d_text.device
    cap = n // MIN_ROW_BYTES + 1 if cap is None else int(cap)
    if out is None:
        i64 = lambda: torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        i32 = lambda: torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out = dict(begin=i64(), end=i64(), number=i64(), name_pos=i64(), name_len=i32(), file_pos=i64(), file_len=i32(), line=i64(),
                   run_first=i64())
    wb = int(L.dgrp_rows_parse_workspace_bytes(n))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    counts = (C.c_int64 * 6)()
    rc = L.dgrp_rows_parse(d_text.data_ptr() if n else None, n, 1 if tsv else 0,
                           *(out[k].data_ptr() for k in ("begin", "end", "number", "name_pos", "name_len", "file_pos", "file_len", "line",
                                                         "run_first")), cap, counts, work.data_ptr(), wb, stream_ptr())
    if rc not in (0, -3):
        check(rc, "dgrp_rows_parse")
    return [int(c) for c in counts], out, rc


def _span_texts(d_text, pos, ln) -> List[str]:
    """The spans (device arrays of positions and lengths) of the text as strings: their bytes in one gather and one copy."""
    import torch
    k = int(pos.numel())
    if k == 0:
        return []
    ln = ln.to(torch.int64)
    total = int(ln.sum())
    offs = torch.cumsum(ln, 0) - ln
    blob = b""
    if total:
        shift = torch.repeat_interleave(pos - offs, ln, output_size=total)
        blob = d_text[torch.arange(total, device=d_text.device) + shift].cpu().numpy().tobytes()
    cut = np.concatenate([offs.cpu().numpy(), [total]])
    return [blob[cut[r]:cut[r + 1]].decode("ascii") for r in range(k)]


def flat_of_device_text(d_text, n: int, tsv: bool):
    """-> (the Flat of the text in device memory, or None where the device does not decide the file; (line, reason) of the first
    malformed line, or None)."""
    counts, out, rc = rows_parse_device(d_text, n, tsv)
    if counts[3]:
        return None, None
    if counts[4]:
        return None, (counts[4], counts[5])
    if rc != 0:
        from ._lib import check
        check(rc, "dgrp_rows_parse")
    lines, kept, runs = counts[:3]
    host = lambda k: out[k][:kept].cpu().numpy()
    first = out["run_first"][:runs]
    names = _span_texts(d_text, out["name_pos"][first], out["name_len"][first])
    files = _span_texts(d_text, out["file_pos"][first], out["file_len"][first]) if tsv else None
    run_first = np.concatenate([first.cpu().numpy(), [kept]]).astype(np.int64)
    return Flat(host("begin"), host("end"), host("number"), host("line"), run_first, names, files, lines, "device"), None


def _device_text(path):
    """(the text of `path` in device memory or None for an empty file, its size) -- uploaded, or inflated there --, or None where it
    is above the resident-bytes limit of the ingest: the rule of annotation.read_listing."""
    from . import gz
    from .fasta import RESIDENT_BYTES, _upload_file
    from .pipeline import require_gpu
    if gz.is_gzip(path):
        try:
            _text, d_text, size = gz.open_inflated(path, RESIDENT_BYTES, require_gpu, _upload_file)
        except gz.GzipError:
            raise
        except ValueError:                                           # inflates to more than the limit
            return None
        return d_text, size
    size = os.path.getsize(path)
    if size > RESIDENT_BYTES:
        return None
    return (_upload_file(path, size, require_gpu()) if size else None), size


def _flat_device(path, tsv: bool) -> Optional[Flat]:
    """The Flat of the file parsed on the device; None where the host path has to read it (not decided, malformed -- the host words
    the error --, above the resident limit)."""
    got = _device_text(path)
    if got is None:
        return None
    d_text, size = got
    if size == 0:
        return Flat(*(np.zeros(0, np.int64) for _ in range(4)), np.zeros(1, np.int64), [], [] if tsv else None, 0, "device")
    flat, _malformed = flat_of_device_text(d_text, size, tsv)
    return flat


def _segment_dtype():
    from .pipeline import SEGMENT_DTYPE
    return SEGMENT_DTYPE


def _grouped(path, flat: Flat, keep: np.ndarray):
    """({name: rows}, {name: lines}) of the rows `keep` marks, as annotation.Listing groups them."""
    number = np.where((flat.number >= 0) & (flat.number < (1 << 31)), flat.number, -1)
    listing = dgann.Listing(path, flat.begin, flat.end, number, flat.line, flat.run_first, flat.run_names, flat.lines, flat.route)
    return listing.grouped(keep)


def _table_on_host(path, repeats):
    """read_annotation on a table that may be gzip: the inflated text goes through a temporary file, an error names `path`."""
    from . import gz
    from .evaluation import AnnotationError, read_annotation
    if not gz.is_gzip(path):
        return read_annotation(path, repeats)
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".table") as tmp:
        tmp.write(_host_bytes(path))
        tmp.flush()
        try:
            return read_annotation(tmp.name, repeats)
        except AnnotationError as e:
            raise AnnotationError(str(e).replace(tmp.name, str(path), 1)) from None


def read_table(path, repeats: Optional[Iterable[int]] = None, device: bool = True) -> dgann.Rows:
    """evaluation.read_annotation(path, repeats) with the lines found and the numbers read on the device: the same rows in the same
    order; whatever it raises, the host path raises."""
    flat = _flat_device(path, False) if device else None
    if flat is None or bool(((flat.begin < 0) | (flat.end < flat.begin)).any()):
        return dgann.Rows(_table_on_host(path, repeats))
    keep = np.ones(flat.begin.size, bool) if repeats is None else np.isin(flat.number, np.array(sorted(set(int(r) for r in repeats)), np.int64))
    rows_of, lines_of = _grouped(path, flat, keep)
    out = dgann.Rows(rows_of)
    out.lines, out.route = lines_of, "device"
    return out


# ---------------------------------------------------------------- the predicted rows
def _check_classes(classes: int) -> int:
    if not MIN_CLASSES <= int(classes) <= MAX_CLASSES:
        raise ValueError(f"classes must lie in {MIN_CLASSES}..{MAX_CLASSES}, not {classes}")
    return int(classes)


def _tsv_rows(path, flat: Flat, classes: int):
    """The checks of a TSV on its rows, the first offender in file order named with its line: a label outside 1..C-1, an end below
    its begin; then one name under two file fields.  -> ({name: rows}, {name: lines})"""
    from .annotation import line_text
    from .evaluation import AnnotationError, _bad
    wrong = (flat.number < 1) | (flat.number >= classes)
    bad = np.flatnonzero(wrong | (flat.begin < 0) | (flat.end < flat.begin))
    if bad.size:
        k = int(bad[0])
        ln = int(flat.line[k])
        why = (f"label {int(flat.number[k])} is not a class of 1..{classes - 1}" if wrong[k] else
               "negative begin" if flat.begin[k] < 0 else "end below begin")
        raise _bad(path, ln, line_text(path, ln), why)
    under: Dict[str, str] = {}
    for name, file in zip(flat.run_names, flat.run_files):
        if under.setdefault(name, file) != file:
            raise AnnotationError(f"{path}: the record name {name!r} stands under two files, {under[name]!r} and {file!r}: their rows "
                                  "cannot be told apart")
    return _grouped(path, flat, np.ones(flat.begin.size, bool))


def read_predicted(path, fmt: str = "auto", classes: int = DEFAULT_CLASSES, device: bool = True, gff_names=None,
                   gff_key: Optional[bytes] = b"Name") -> Predicted:
    """The predicted rows of `path` as {record name: SEGMENT_DTYPE rows}, label = class, file order within a name (module
    docstring).  device False: the host paths.  gff_names (gffin.parse_names; None: class1..), gff_key (None: the type column):
    how the rows of a `gff3` file get their numbers."""
    from .evaluation import read_annotation
    classes = _check_classes(classes)
    fmt = resolve_predicted_format(path, fmt)
    if fmt == "gff3":
        from . import gffin
        return gffin.read_predicted(path, gffin.default_names(classes) if gff_names is None else gff_names, gff_key, classes, device)
    if fmt == "repeatmasker":
        listing = dgann.read_listing(path, device)
        read = listing.table_mask()
        bad = np.flatnonzero(read & ((listing.begin < 0) | (listing.end < listing.begin)))
        if bad.size:
            k = int(bad[0])
            raise listing._bad(k, "negative begin" if listing.begin[k] < 0 else "end below begin")
        keep = read & (listing.number >= 1) & (listing.number < classes)
        rows_of, lines_of = listing.grouped(keep)
        out = Predicted(rows_of)
        out.lines, out.route, out.rows_read, out.rows_dropped = lines_of, listing.route, int(read.sum()), int(read.sum() - keep.sum())
    elif fmt == "table":
        flat = _flat_device(path, False) if device else None
        if flat is not None and not bool(((flat.begin < 0) | (flat.end < flat.begin)).any()):
            keep = (flat.number >= 1) & (flat.number < classes)
            rows_of, lines_of = _grouped(path, flat, keep)
            out = Predicted(rows_of)
            out.lines, out.route, out.rows_read, out.rows_dropped = lines_of, "device", int(keep.size), int(keep.size - keep.sum())
        else:
            out = Predicted()
            for name, rows in _table_on_host(path, None).items():
                keep = (rows["label"] >= 1) & (rows["label"] < classes)
                out.rows_read += int(keep.size)
                out.rows_dropped += int(keep.size - keep.sum())
                if keep.any():
                    out[name] = rows[keep]
    else:
        flat = _flat_device(path, True) if device else None
        if flat is None:
            flat = tsv_flat_host(path)
        rows_of, lines_of = _tsv_rows(path, flat, classes)
        out = Predicted(rows_of)
        out.lines, out.route, out.rows_read = lines_of, flat.route, int(flat.begin.size)
    out.format = fmt
    return out


# ---------------------------------------------------------------- flattening
def flatten_reference(origin: int, length: int, rows: np.ndarray) -> np.ndarray:
    """The flattening rule in numpy for one record of `length` evaluated bases from the coordinate `origin`: the rows painted onto
    a zero track, the smallest label winning a base, clipped to the span; then every run of one label > 0 among the bases but the
    last as a row, and the last base as a row of its own where it carries a label (deepgrp/sequence.pyx:79-85)."""
    n, o = int(length), int(origin)
    SEG = _segment_dtype()
    if n <= 0:
        return np.zeros(0, SEG)
    track = np.zeros(n, np.int64)
    for row in rows:
        a, e = min(max(int(row["start"]) - o, 0), n), min(max(int(row["end"]) - o, 0), n)
        if e > a:
            part = track[a:e]
            track[a:e] = np.where(part == 0, int(row["label"]), np.minimum(part, int(row["label"])))
    body = track[:n - 1]
    edge = np.flatnonzero(np.diff(body, prepend=0, append=0))        # where the label changes, the two ends included
    runs = [(int(a), int(e), int(body[a])) for a, e in zip(edge[:-1], edge[1:]) if body[a]]
    if track[n - 1]:
        runs.append((n - 1, n, int(track[n - 1])))
    out = np.zeros(len(runs), SEG)
    if runs:
        a = np.asarray(runs, np.int64)
        out["start"], out["end"], out["label"] = a[:, 0] + o, a[:, 1] + o, a[:, 2]
    return out


def flatten(origins: Sequence[int], lengths: Sequence[int], rows: Sequence[np.ndarray]) -> List[np.ndarray]:
    """`flatten_reference` of every record of a work item, on the device and on the current stream: one dgrp_paint_rows_batch for
    the item, one dgrp_segments per record that has a row, one copy back for all of them.  -> the rows record by record
    (`contig` = the record's index in the item)."""
    import torch

    from ._lib import check, lib
    from .evaluation import paint, tables, upload
    from .pipeline import require_gpu, stream_ptr
    SEG = _segment_dtype()
    nrec = len(lengths)
    out = [np.zeros(0, SEG) for _ in range(nrec)]
    rows = [np.ascontiguousarray(r, SEG) for r in rows]
    ln, org, off = tables(origins, [max(int(x), 0) for x in lengths])
    todo = [r for r in range(nrec) if len(rows[r]) and ln[r] > 0]
    if not todo:
        return out
    L, dev = lib(), require_gpu()
    ro, _flat, d_rows = upload(rows, dev)
    work = torch.empty(max(int(L.dgrp_eval_workspace_bytes(nrec, int(ro[-1]))), int(L.dgrp_segments_workspace_bytes(int(ln.max()))), 1),
                       dtype=torch.uint8, device=dev)
    d_labels = paint(ln, org, off, ro, d_rows, work, dev)
    # k rows leave at most 2 k + 1 runs on the track, and the last base may be cut off the run it ends
    caps = np.array([2 * len(rows[r]) + 2 for r in todo], np.int64)
    at = np.zeros(len(todo) + 1, np.int64)
    np.cumsum(caps, out=at[1:])
    d_rec = torch.empty(int(at[-1]) * SEG.itemsize, dtype=torch.uint8, device=dev)
    d_count = torch.zeros(len(todo), dtype=torch.int64, device=dev)
    s = stream_ptr()
    for k, r in enumerate(todo):
        check(L.dgrp_segments(d_labels.data_ptr() + int(off[r]), int(ln[r]), int(org[r]), r, d_rec.data_ptr() + int(at[k]) * SEG.itemsize,
                              int(caps[k]), d_count.data_ptr() + 8 * k, work.data_ptr(), work.numel(), s), "dgrp_segments")
    count = d_count.cpu().numpy()
    rec = d_rec.cpu().numpy().view(SEG)
    for k, r in enumerate(todo):
        if count[k] > caps[k]:
            raise RuntimeError(f"{int(count[k])} runs from {len(rows[r])} rows: more than 2 k + 2")
        out[r] = rec[at[k]:at[k] + count[k]].copy()
    return out


# ---------------------------------------------------------------- the command
def compare(predicted: Dict[str, np.ndarray], annotation: Dict[str, np.ndarray],
            inputs: Iterable[Tuple[str, Iterable[Tuple[str, object]]]], classes: int, repeats: Sequence[int], min_overlap: float = 0.5,
            info: Optional[Dict[str, object]] = None, reports=()) -> Dict[str, object]:
    """Score the rows `predicted` (read_predicted's dict) against `annotation` (read_annotation's dict) over the records of `inputs`
    -- (filename, (header, record) pairs) as `predict` reads them -- and return the JSON content of evaluation.report.  The records
    are walked as evaluation.evaluate walks them; consecutive short records form one work item (one Accumulator.add), a long one is
    an item of its own.  The predicted rows of an item are flattened (module docstring) before they are scored; no scores and no
    probabilities exist, so the reports get `scores=None`, `probed=None`.  Raises NoMatchError when no annotation row names a
    record, NoPredictedError when no predicted row does."""
    from .evaluation import Accumulator, NoMatchError, record_name, report, strip_n
    from .runner import SMALL_RECORD
    SEG = _segment_dtype()
    classes = _check_classes(classes)
    reports = list(reports)
    for r in reports:
        if hasattr(r, "probe") and r.key != "strata":
            raise ValueError(f"the report {r.key!r} needs probabilities or scores: compare has none")
        r.bind(annotation, classes)
    acc = Accumulator(classes, min_overlap, reports)
    empty = np.zeros(0, SEG)
    seen_names: List[str] = []
    tally = dict(matched=0, flattened=0)

    def run(group):
        names = [g[0] for g in group]
        org, ln = [g[1] for g in group], [g[2] for g in group]
        pred = flatten(org, ln, [predicted.get(nm, empty) for nm in names])
        tally["flattened"] += sum(len(p) for p in pred)
        acc.add(org, ln, pred, [annotation.get(nm, empty) for nm in names], None, None, names)

    group, bases = [], 0
    for filename, records in inputs:
        for header, rec in records:
            if isinstance(rec, str):
                startpos, length = strip_n(rec.encode("utf-8"))
            else:
                startpos, length = int(rec.startpos), int(rec.length)
            name = record_name(filename, header)
            if length < 0:
                raise ValueError(f"{filename}: the record {name!r} holds no base other than N")
            if len(seen_names) < 5 and name not in seen_names:
                seen_names.append(name)
            tally["matched"] += name in predicted
            small = length <= SMALL_RECORD
            if group and (not small or len(group) >= GROUP_RECORDS or bases + length > GROUP_BASES):
                run(group)
                group, bases = [], 0
            group.append((name, startpos, length))
            bases += length
            if not small:
                run(group)
                group, bases = [], 0
    if group:
        run(group)
    some = lambda d, none: ", ".join(repr(x) for x in sorted(d)[:5]) or none
    if acc.rows_used == 0:
        raise NoMatchError("no annotation row names a record of the inputs (records: {}; annotation: {})".format(
            ", ".join(repr(x) for x in seen_names) or "none", some(annotation, "no kept rows")))
    if tally["matched"] == 0:
        raise NoPredictedError("no predicted row names a record of the inputs: nothing to compare (records: {}; predicted: {})".format(
            ", ".join(repr(x) for x in seen_names) or "none", some(predicted, "no rows")))
    info = dict(info or {})
    info.setdefault("repeats", [int(r) for r in repeats])
    rows = dict(info.get("predicted_rows") or {})
    rows.setdefault("read", int(getattr(predicted, "rows_read", sum(len(v) for v in predicted.values()))))
    rows.setdefault("dropped", int(getattr(predicted, "rows_dropped", 0)))
    rows["flattened"] = int(tally["flattened"])
    info["predicted_rows"] = rows
    return report(acc, info)


def write_strata(report, plan, log) -> None:
    """`--strata` without probabilities: PREFIX.strata.tsv alone (the element counts); PREFIX.strata.bases.tsv is not written."""
    from .outfiles import write_texts
    from .strata import strata_tsv
    log.warning("--strata: %s needs probabilities, which compare does not have: only %s is written", plan.bases_path, plan.strata_path)
    write_texts(log, plan.prefix, "--strata", (plan.strata_path,), [strata_tsv(report.counts, report.div_edges, report.len_edges)])
