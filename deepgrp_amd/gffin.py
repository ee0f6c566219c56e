"""GFF3 as PREDICTED of `compare` and as ANNOTATION of `evaluate` and `compare` (format `gff3`): the feature lines of the file -- what
`predict --bed_dir D --bed_gff3` writes, and what repeat finders and genome portals ship -- read into the rows a table gives, the
label of a row looked up by NAME.

THE GRAMMAR is stated once, in include/deepgrp_hip.h (dgrp_gff_parse): lines, the end of the features E (`##FASTA`, or a line that
opens with '>'), nine fields between single tabs, 1-based closed coordinates, the label string (column 3, or the value of one
attribute key of column 9), its %XX decoding and the exact match against a table of alternatives.  `features_host` below is that
grammar on the lines of the file in Python: the host path, and the statement the device entry (csrc/gff_parse_kernels.hip,
DESIGN 5zb) is tested against.

NAMES.  One entry per label 1..C-1, separated by commas; an entry is one or more alternatives joined by '|':
`LTR|ERV1|ERVK,LINE|L1,Alu,Satellite`.  The default is `class1,...,class<C-1>`, what --bed_gff3 writes without --bed_names.  A row
whose label string equals no alternative (or that has no piece with the key) has the number 0.

ROUTES.  The text goes to the device whole (uploaded, or inflated there).  What the device does not decide -- a byte outside
0x20..0x7e other than tab and line feed, a carriage return that no line feed follows, a start or end that is not 1..18 plain digits
-- goes to the host whole, as does a file above the resident-bytes limit and `device=False`.  Both routes raise a malformed line, a
negative begin (start 0) and an end below its begin as evaluation.AnnotationError naming file, line and the line's text.  The seqid
of a run is decoded (`decode`) on the host before the rows are grouped: two spellings of one name are one record."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MIN_LINE_BYTES = 11                      # the shortest feature line dgrp_gff_parse keeps: n // 11 + 1 rows always suffice
MAX_ALTERNATIVES = 4096
MAX_NAME = 255                           # bytes of an alternative, and of the key
DEFAULT_KEY = "Name"
REASON = "expected nine fields between tabs"        # reason 3 of the device entry
_HEX = b"0123456789abcdefABCDEF"

Names = List[List[bytes]]


def _raw(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


def _text(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")


def decode(raw: bytes) -> bytes:
    """The %XX rule: '%' followed by two hex digits of either case is that byte, any other '%' is itself."""
    out = bytearray()
    p, n = 0, len(raw)
    while p < n:
        if raw[p] == 0x25 and n - p >= 3 and raw[p + 1] in _HEX and raw[p + 2] in _HEX:
            out.append(int(raw[p + 1:p + 3], 16))
            p += 3
        else:
            out.append(raw[p])
            p += 1
    return bytes(out)


# ---------------------------------------------------------------- names
def default_names(classes: int) -> Names:
    return [[b"class%d" % k] for k in range(1, int(classes))]


def parse_names(spec: Optional[str], classes: Optional[int], flag: str = "names") -> Names:
    """The entries of a names flag for `classes` classes (None: the default).  ValueError: an empty alternative, one above MAX_NAME
    bytes, the wrong number of entries, one alternative under two labels, more than MAX_ALTERNATIVES alternatives.  classes None
    (`evaluate` before its model is read): every check but the number of entries."""
    if spec is None:
        return default_names(2 if classes is None else classes)
    names = [[_raw(a) for a in entry.split("|")] for entry in spec.split(",")]
    under: Dict[bytes, int] = {}
    for label, entry in enumerate(names, 1):
        for alt in entry:
            if not alt:
                raise ValueError(f"{flag}: an empty alternative in the entry of label {label}")
            if len(alt) > MAX_NAME:
                raise ValueError(f"{flag}: an alternative of label {label} has {len(alt)} bytes, above {MAX_NAME}")
            if under.setdefault(alt, label) != label:
                raise ValueError(f"{flag}: the alternative {_text(alt)!r} stands under two labels, {under[alt]} and {label}")
    if len(under) > MAX_ALTERNATIVES:
        raise ValueError(f"{flag}: {len(under)} alternatives, above {MAX_ALTERNATIVES}")
    if classes is not None and len(names) != classes - 1:
        raise ValueError(f"{flag}: {len(names)} entries for the labels 1..{classes - 1}: one entry per label, separated by commas")
    return names


def check_key(key: Optional[str], by_type: bool) -> Optional[bytes]:
    """--gff_key and --gff_by_type as the key of the readers: None for the type column.  ValueError: both, an empty key, one above
    MAX_NAME bytes or with a byte that ends a tag."""
    if by_type:
        if key is not None:
            raise ValueError("--gff_by_type takes the label from column 3: it excludes --gff_key")
        return None
    raw = _raw(DEFAULT_KEY if key is None else key)
    if not raw or len(raw) > MAX_NAME:
        raise ValueError(f"--gff_key: a tag of 1..{MAX_NAME} bytes, not {len(raw)}")
    if any(c in raw for c in b"=;\t\n\r"):
        raise ValueError(f"--gff_key: {_text(raw)!r} holds a byte that ends a tag")
    return raw


def names_table(names: Names):
    """What the device looks a label string up in: (the alternatives back to back, uint8; int64 offsets [count + 1]; int32 numbers
    [count]; count), the alternatives in ascending byte order -- the order dgrp_gff_parse's binary search needs."""
    pairs = sorted({alt: label for label, entry in enumerate(names, 1) for alt in entry}.items())
    if len(pairs) > MAX_ALTERNATIVES:
        raise ValueError(f"{len(pairs)} alternatives, above {MAX_ALTERNATIVES}")
    off = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum([len(a) for a, _l in pairs], out=off[1:])
    blob = np.frombuffer(b"".join(a for a, _l in pairs), np.uint8).copy()
    return blob, off, np.array([l for _a, l in pairs], np.int32), len(pairs)


# ---------------------------------------------------------------- the host statement
def _split_lines(data: bytes) -> List[bytes]:
    """The lines of the text: cut at line feeds, a carriage return directly before the cut (or the end) taken off."""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def _host_bytes(path) -> bytes:
    from .compare import _host_bytes as read
    return read(path)


def line_text(path, lineno: int) -> str:
    """Line `lineno` (from 1) of the file, for an error message."""
    lines = _split_lines(_host_bytes(path))
    return _text(lines[lineno - 1]) if 0 < lineno <= len(lines) else ""


def features_of_bytes(path, data: bytes, names: Names, key: Optional[bytes]):
    """The grammar on the bytes of a file: -> (compare.Flat with route "host", E)."""
    from .compare import Flat
    from .evaluation import _bad
    number_of = {alt: label for label, entry in enumerate(names, 1) for alt in entry}
    seqids, vals = [], []
    at, lines, end_at = 0, 0, len(data)
    for raw_line in data.split(b"\n") if data else []:
        if at >= len(data):
            break                                                    # (the empty piece behind a final line feed)
        line = raw_line[:-1] if raw_line.endswith(b"\r") else raw_line
        if line == b"##FASTA" or line.startswith(b">"):
            end_at = at
            break
        at += len(raw_line) + 1
        lines += 1
        if line == b"" or line.startswith(b"#"):
            continue
        f = line.split(b"\t", 8)
        if len(f) < 9:
            raise _bad(path, lines, _text(line), REASON)
        row = []
        for what, tok in zip(("start", "end"), f[3:5]):
            try:
                row.append(int(np.int64(int(_text(tok)))))
            except (ValueError, OverflowError):
                raise _bad(path, lines, _text(line), f"{what} {_text(tok)!r} is not an integer") from None
        label: Optional[bytes] = f[2]
        if key is not None:
            label = None
            for piece in f[8].split(b";"):
                tag, eq, value = piece.partition(b"=")
                if eq and tag == key:
                    label = value
                    break
        seqids.append(f[0])
        vals.append((row[0] - 1, row[1], number_of.get(decode(label), 0) if label is not None else 0, lines))
    a = np.asarray(vals, np.int64).reshape(-1, 4)
    first = [i for i in range(len(seqids)) if i == 0 or seqids[i] != seqids[i - 1]]
    flat = Flat(a[:, 0], a[:, 1], a[:, 2], a[:, 3], np.asarray(first + [len(seqids)], np.int64), [_text(decode(seqids[i])) for i in first],
                None, lines, "host")
    return flat, end_at


def features_host(path, names: Names, key: Optional[bytes]):
    """The feature lines of `path` (plain, gzip or BGZF) by the grammar, on the host -> compare.Flat: rows in file order, begin =
    start - 1, the runs of byte-equal seqids with their DECODED names.  A malformed line is an AnnotationError."""
    return features_of_bytes(path, _host_bytes(path), names, key)[0]


# ---------------------------------------------------------------- the device entry
_TABLES: Dict[object, tuple] = {}


def _device_table(names: Names, key: Optional[bytes], dev):
    import torch
    ident = (tuple(tuple(e) for e in names), key, str(dev))
    if ident not in _TABLES:
        if len(_TABLES) >= 8:
            _TABLES.clear()
        blob, off, number, count = names_table(names)
        up = lambda a: torch.from_numpy(a).to(dev)                   # (an empty table is passed as NULL)
        d_key = torch.from_numpy(np.frombuffer(key, np.uint8).copy()).to(dev) if key else None
        _TABLES[ident] = (up(blob), up(off), up(number), count, d_key)
    return _TABLES[ident]


def gff_parse_device(d_text, n: Optional[int], names: Names, key: Optional[bytes], cap: Optional[int] = None, out=None):
    """dgrp_gff_parse on the uint8 device tensor `d_text` (its first `n` bytes): -> (counts = [lines in front of E, rows, runs,
    not-decided flag, first malformed line, its reason, E], the device arrays begin, end, number, name_pos, name_len, line, run_first
    of `cap` rows -- default n // 11 + 1; `out`: use these instead --, the return code).  Nothing is raised for DGRP_ENOMEM (-3: more
    rows than `cap`; counts[1] tells the need)."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    n = int(d_text.numel()) if n is None else int(n)
    dev = d_text.device
    d_names, d_off, d_number, count, d_key = _device_table(names, key, dev)
    cap = n // MIN_LINE_BYTES + 1 if cap is None else int(cap)
    if out is None:
        i64 = lambda: torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        out = dict(begin=i64(), end=i64(), number=i64(), name_pos=i64(), name_len=torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
                   line=i64(), run_first=i64())
    wb = int(L.dgrp_gff_parse_workspace_bytes(n))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    counts = (C.c_int64 * 7)()
    rc = L.dgrp_gff_parse(d_text.data_ptr() if n else None, n, d_names.data_ptr() if count else None, d_off.data_ptr() if count else None,
                          d_number.data_ptr() if count else None, count, d_key.data_ptr() if key else None, len(key) if key else 0,
                          *(out[k].data_ptr() for k in ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")), cap, counts,
                          work.data_ptr(), wb, stream_ptr())
    if rc not in (0, -3):
        check(rc, "dgrp_gff_parse")
    return [int(c) for c in counts], out, rc


def features_device(d_text, n: int, names: Names, key: Optional[bytes]):
    """-> (the compare.Flat of the text in device memory, or None where the device does not decide the file or finds a malformed
    line; the line of the first malformed line, or None; E)."""
    from .compare import Flat, _span_texts
    counts, out, rc = gff_parse_device(d_text, n, names, key)
    if counts[3]:
        return None, None, counts[6]
    if counts[4]:
        return None, counts[4], counts[6]
    if rc != 0:
        from ._lib import check
        check(rc, "dgrp_gff_parse")
    lines, kept, runs = counts[:3]
    host = lambda k: out[k][:kept].cpu().numpy()
    first = out["run_first"][:runs]
    run_names = [_text(decode(s.encode("ascii"))) for s in _span_texts(d_text, out["name_pos"][first], out["name_len"][first])]
    run_first = np.concatenate([first.cpu().numpy(), [kept]]).astype(np.int64)
    return Flat(host("begin"), host("end"), host("number"), host("line"), run_first, run_names, None, lines, "device"), None, counts[6]


# ---------------------------------------------------------------- the readers
def read_features(path, names: Names, key: Optional[bytes], device: bool = True):
    """The rows of the GFF3 file `path` as a compare.Flat, checked: a malformed line, a negative begin and an end below its begin
    raise evaluation.AnnotationError with `<file>:<line>:` and the line's text, on either route."""
    from .compare import Flat, _device_text
    from .evaluation import _bad
    flat = None
    got = _device_text(path) if device else None
    if got is not None:
        d_text, size = got
        if size == 0:
            flat = Flat(*(np.zeros(0, np.int64) for _ in range(4)), np.zeros(1, np.int64), [], None, 0, "device")
        else:
            flat, malformed, _end = features_device(d_text, size, names, key)
            if malformed is not None:
                raise _bad(path, malformed, line_text(path, malformed), REASON)
    if flat is None:
        flat = features_host(path, names, key)
    bad = np.flatnonzero((flat.begin < 0) | (flat.end < flat.begin))
    if bad.size:
        k = int(bad[0])
        ln = int(flat.line[k])
        raise _bad(path, ln, line_text(path, ln), "negative begin" if flat.begin[k] < 0 else "end below begin")
    return flat


def read_predicted(path, names: Names, key: Optional[bytes], classes: int, device: bool = True):
    """PREDICTED of `compare`: the rows with a number of 1..classes-1 as a compare.Predicted; the others are dropped and counted."""
    from .compare import Predicted, _grouped
    flat = read_features(path, names, key, device)
    keep = (flat.number >= 1) & (flat.number < classes)
    rows_of, lines_of = _grouped(path, flat, keep)
    out = Predicted(rows_of)
    out.lines, out.route, out.rows_read, out.rows_dropped = lines_of, flat.route, int(keep.size), int(keep.size - keep.sum())
    out.format = "gff3"
    return out


def read_annotation(path, names: Names, key: Optional[bytes], repeats: Optional[Iterable[int]] = None, device: bool = True):
    """ANNOTATION of `evaluate` and `compare`: an annotation.Rows like the table's, `repeats` filtering the numbers exactly as it
    filters a table's fourth column (None keeps every row, the number 0 of an unnamed row included)."""
    from .annotation import Rows
    from .compare import _grouped
    flat = read_features(path, names, key, device)
    keep = np.ones(flat.begin.size, bool) if repeats is None else np.isin(flat.number, np.array(sorted(set(int(r) for r in repeats)), np.int64))
    rows_of, lines_of = _grouped(path, flat, keep)
    out = Rows(rows_of)
    out.lines, out.route = lines_of, flat.route
    return out


# ---------------------------------------------------------------- the command line
def plan(args, classes: Optional[int], sides: Sequence[Tuple[str, str, str]]):
    """The GFF3 flags of a command, checked before anything is read: `sides` = (names flag, format flag, its value) per side.  ->
    ({names flag: Names}, key).  ValueError states the refusal.  classes None: as parse_names."""
    key = check_key(getattr(args, "gff_key", None), bool(getattr(args, "gff_by_type", False)))
    names = {}
    for flag, fmt_flag, fmt in sides:
        spec = getattr(args, flag.lstrip("-"), None)
        if spec is not None and fmt not in ("auto", "gff3"):
            raise ValueError(f"{flag} names the labels of a GFF3 file: {fmt_flag} {fmt} has numbers")
        names[flag] = parse_names(spec, classes, flag)
    return names, key


def refuse_names(flag: str, given: bool, fmt_flag: str, resolved: str) -> None:
    """The same refusal once `auto` has looked at the file."""
    if given and resolved != "gff3":
        raise ValueError(f"{flag} names the labels of a GFF3 file: {fmt_flag} auto found {resolved}")
