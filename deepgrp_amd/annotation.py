"""RepeatMasker output as the annotation of `evaluate` and `train`, parsed on the GPU: a `genome.fa.out` listing or a UCSC `rmsk`
table, plain, gzip or BGZF, gives what the six-column table of ``python -m deepgrp_amd._scripts.parse_rm`` gives -- the same rows in
the same order with the same numbers -- without that table being written and read again.

The text goes to the device whole (uploaded, or inflated there: gz.open_inflated) and dgrp_rm_parse (csrc/annotation_kernels.hip,
DESIGN 5t) finds the lines, takes each through the token statement of parse_rm's two patterns, numbers it from the tables built
HERE from that script's REPEATS and pentamer_sets(), and returns the kept rows as arrays in file order plus the first row of every
run of one contig name.  Python reads one name per run: no line and no row is touched on the host.

NOT PLAIN -> HOST.  The device does not decide a file that holds a byte outside 0x20..0x7e other than tab and line feed, a carriage
return that no line feed follows, or a coordinate of more than 18 digits: it raises a flag and the WHOLE file goes to the host path,
which is parse_rm's own `read_repeatmasker` on the decoded text (UTF-8, universal newlines, as the script opens its input) -- not a
second grammar.  The same pattern as gzip input, where what the device does not take goes to zlib.  `device=False`, and a listing
above the resident-bytes limit of the ingest (DGRP_FASTA_RESIDENT_BYTES), take the host path too.

What the table's readers then do to the rows is applied on the arrays: evaluation.read_annotation's skip of a contig that opens with
'#', its checks and its --repeats filter (`evaluation_rows`), training.read_truth_rows' rules (`Listing.truth_rows`).  An error names
the listing and ITS line."""
from __future__ import annotations

import io
import os
import re
import zlib
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from ._scripts import parse_rm

TILE_BYTES = 32768                       # DGRP_RM_TILE_BYTES: text per workgroup of the device parser
MIN_LINE_BYTES = 22                      # the shortest line that matches: n // 22 + 1 rows always suffice
SNIFF_BYTES = 64 << 10
SNIFF_LINES = 16
FORMATS = ("auto", "table", "repeatmasker", "gff3")
_BASES = {"A": 0, "C": 1, "G": 2, "T": 3}


def _segment_dtype():
    from .pipeline import SEGMENT_DTYPE                              # (imports torch: the sniffer above the refusals does without)
    return SEGMENT_DTYPE


def tables():
    """What the device numbers with, from the port's own statements: (the names of REPEATS back to back, int64 offsets [len + 1],
    uint8 [1024] by 5-mer -- the bases as base-4 digits, first base highest: 1 in pentamer_sets()'s exact set, 2 in its one_off set,
    0 in neither --, the number of HSATII)."""
    from ._lib import name_blob
    _raw, blob, off = name_blob(parse_rm.REPEATS)
    exact, one_off = parse_rm.pentamer_sets()
    pent = np.zeros(1024, np.uint8)

    def code(word):
        c = 0
        for ch in word:
            c = c * 4 + _BASES[ch]
        return c
    for w in one_off:
        pent[code(w)] = 2
    for w in exact:                                                  # (the sets are disjoint; exact wins if they were not)
        pent[code(w)] = 1
    return np.frombuffer(blob, np.uint8).copy(), off, pent, int(parse_rm.NUMBER["HSATII"])


def _head(path) -> bytes:
    with open(path, "rb") as fh:
        head = fh.read(SNIFF_BYTES)
    if head[:2] == b"\x1f\x8b":
        try:
            head = zlib.decompressobj(31).decompress(head, SNIFF_BYTES)
        except zlib.error:
            head = b""
    return head


def sniff(path) -> str:
    """"gff3" when the first line begins with `##gff-version 3` (gffin.py); else "repeatmasker" when one of the first 16 lines of
    `path` that are not blank and do not open with '#' matches a pattern of parse_rm, else "table"; decided on the first 64 KiB
    (inflated with zlib when the magic bytes say gzip)."""
    head = _head(path)
    if head.startswith(b"##gff-version 3"):
        return "gff3"
    lines = head.decode("utf-8", "replace").splitlines()
    if len(head) >= SNIFF_BYTES and lines:
        lines.pop()                                                  # (cut somewhere)
    seen = 0
    for line in lines:
        f = line.split()
        if not f or f[0][0] == "#":
            continue
        if parse_rm.parse_line(line).ctg is not None:
            return "repeatmasker"
        seen += 1
        if seen >= SNIFF_LINES:
            break
    return "table"


def resolve_format(path, fmt: str) -> str:
    if fmt not in FORMATS:
        raise ValueError(f"annotation format {fmt!r}: one of {', '.join(FORMATS)}")
    return sniff(path) if fmt == "auto" else fmt


def _read_text(path) -> str:
    """The decoded text of the listing as parse_rm's `open(path, "r")` reads it: UTF-8, universal newlines."""
    from . import gz
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:2] == gz.MAGIC:
        data = bytes(gz.inflate_host(data, path, 1 << 62))
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError as exc:
        from .evaluation import AnnotationError
        raise AnnotationError(f"{path}: not UTF-8 text at byte {exc.start}") from None
    return io.StringIO(text, newline=None).getvalue()


def line_text(path, lineno: int) -> str:
    """Line `lineno` (from 1) of the listing, for an error message: the file is read once more, on the host."""
    for k, line in enumerate(io.StringIO(_read_text(path)), 1):
        if k == lineno:
            return line.rstrip("\n")
    return ""


_DIV_OUT = re.compile(r"^\s*\d+\s+(\S+)")                          # token 1 of a line _OUT_LINE matches
_DIV_RMSK = re.compile(r"^\d+\t\d+\t(\d+)")                         # field 2 of a line _RMSK_LINE matches
_DIV_PERCENT = re.compile(r"([0-9]{1,6})(?:\.([0-9]*))?")
_DIV_MILLI = re.compile(r"[0-9]{1,7}")


def millidiv_of_line(line: str) -> int:
    """The divergence of a listing's line from its consensus in tenths of a percent, -1 where it states none: the rule of
    dgrp_rm_parse_fields on a decoded line, `.out` or `rmsk` decided exactly as parse_rm.parse_line decides.  `.out`: token 1
    (`perc div.`) as a whole is D, `D.` or `D.d...` with D 1..6 digits -> 10 * int(D) + the first digit behind the point (0 if
    none; further digits dropped, not rounded).  `rmsk`: field 2 (`milliDiv`) is that integer when it has at most 7 digits.
    Anything else -- and a line that matches neither pattern -- is -1."""
    if parse_rm._OUT_LINE.match(line):
        m = _DIV_PERCENT.fullmatch(_DIV_OUT.match(line).group(1))
        if m is None:
            return -1
        frac = m.group(2)
        return 10 * int(m.group(1)) + (int(frac[0]) if frac else 0)
    if parse_rm._RMSK_LINE.match(line):
        tok = _DIV_RMSK.match(line).group(1)
        return int(tok) if _DIV_MILLI.fullmatch(tok) else -1
    return -1


class Listing:
    """The numbered rows of a listing in file order: `begin`, `end`, `line` (int64), `number`, `millidiv` (int32; the divergence in
    tenths of a percent, -1 where not stated), and the runs of one contig name -- run r is rows run_first[r] .. run_first[r + 1]
    and is named run_names[r].  `route`: "device" or "host".  A listing of ALL rows (read_listing(all_rows=True)) holds every line
    that matches a pattern, `number` 0 where the rule finds none, and also `family_id` (int32 per row: the rank of its family token
    among the distinct tokens of the listing in ascending byte order) and `families` (those tokens in id order); else both are
    None."""

    def __init__(self, path, begin, end, number, line, run_first, run_names: List[str], lines: int, route: str, millidiv=None,
                 family_id=None, families: Optional[List[str]] = None):
        self.path, self.route, self.lines = path, route, int(lines)
        self.begin, self.end, self.line = (np.ascontiguousarray(a, np.int64) for a in (begin, end, line))
        self.number = np.ascontiguousarray(number, np.int32)
        self.run_first = np.ascontiguousarray(run_first, np.int64)
        self.run_names = list(run_names)
        self.millidiv = np.full(self.begin.size, -1, np.int32) if millidiv is None else np.ascontiguousarray(millidiv, np.int32)
        if self.millidiv.shape != self.begin.shape:
            raise ValueError(f"{self.millidiv.size} divergences for {self.begin.size} rows")
        self.family_id = None if family_id is None else np.ascontiguousarray(family_id, np.int32)
        self.families = None if families is None else list(families)
        if self.family_id is not None and self.family_id.shape != self.begin.shape:
            raise ValueError(f"{self.family_id.size} family ids for {self.begin.size} rows")

    def __len__(self) -> int:
        return int(self.begin.size)

    def contigs(self):
        """(names in order of first appearance, the index into them of every row): runs of one name merged with a dict."""
        ids: Dict[str, int] = {}
        run_id = np.fromiter((ids.setdefault(nm, len(ids)) for nm in self.run_names), np.int64, count=len(self.run_names))
        return list(ids), np.repeat(run_id, np.diff(self.run_first))

    def grouped(self, keep: Optional[np.ndarray] = None):
        """({contig: SEGMENT_DTYPE rows with label = number}, {contig: their lines}) of the rows `keep` marks (None: all), file order
        within a contig, contigs sorted by name as read_annotation's dict is; contigs without a kept row are left out."""
        return self.grouped_fields(keep)[:2]

    def grouped_fields(self, keep: Optional[np.ndarray] = None):
        """`grouped` plus {contig: the millidiv of its rows}, the same rows in the same order."""
        rows_of: Dict[str, np.ndarray] = {}
        lines_of: Dict[str, np.ndarray] = {}
        div_of: Dict[str, np.ndarray] = {}
        for name, sel in self.grouped_index(keep).items():
            rows = np.zeros(sel.size, _segment_dtype())
            rows["start"], rows["end"], rows["label"] = self.begin[sel], self.end[sel], self.number[sel]
            rows_of[name] = rows
            lines_of[name] = self.line[sel]
            div_of[name] = self.millidiv[sel]
        return rows_of, lines_of, div_of

    def grouped_index(self, keep: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
        """{contig: the indices of its rows among those `keep` marks}, in the order `grouped` states."""
        names, cid = self.contigs()
        idx = np.arange(len(self)) if keep is None else np.flatnonzero(keep)
        out: Dict[str, np.ndarray] = {}
        if idx.size == 0:
            return out
        order = idx[np.argsort(cid[idx], kind="stable")]
        counts = np.bincount(cid[idx], minlength=len(names))
        parts = np.split(order, np.cumsum(counts)[:-1])
        for k in sorted(range(len(names)), key=lambda i: names[i]):
            if parts[k].size:
                out[names[k]] = parts[k]
        return out

    def _bad(self, k: int, why: str):
        from .evaluation import _bad
        ln = int(self.line[k])
        return _bad(self.path, ln, line_text(self.path, ln), why)

    def table_mask(self) -> np.ndarray:
        """The rows evaluation.read_annotation reads from the table: it skips a line whose contig opens with '#'."""
        names, cid = self.contigs()
        hashed = np.fromiter((nm.startswith("#") for nm in names), bool, count=len(names))
        return ~hashed[cid] if len(self) else np.zeros(0, bool)

    def truth_rows(self, names: Sequence[str], repeats_to_search) -> Dict[str, np.ndarray]:
        """training.read_truth_rows of the table of this listing, on the arrays: rows of the contigs `names` whose number is in
        `repeats_to_search`; such a row whose number has no truth row, or with a negative coordinate, is a ValueError naming its
        line (the first in file order); `end <= begin` is dropped."""
        classes = len(repeats_to_search) + 1
        all_names, cid = self.contigs()
        picked = np.fromiter((nm in set(names) for nm in all_names), bool, count=len(all_names))
        wanted = np.isin(self.number, np.array(sorted(set(int(r) for r in repeats_to_search)), np.int64))
        use = (picked[cid] if len(self) else np.zeros(0, bool)) & wanted
        no_row = use & ~((self.number >= 1) & (self.number < classes))
        negative = use & ((self.begin < 0) | (self.end < 0))
        bad = np.flatnonzero(no_row | negative)
        if bad.size:
            k = int(bad[0])
            ln = int(self.line[k])
            text = line_text(self.path, ln)
            if no_row[k]:
                raise ValueError(f"{self.path}:{ln}: repeat number {int(self.number[k])} has no row in a truth of {classes} classes "
                                 f"(repeats_to_search = {list(repeats_to_search)}): {text.rstrip()!r}")
            raise ValueError(f"{self.path}:{ln}: negative coordinate: {text.rstrip()!r}")
        rows_of, _lines = self.grouped(use & (self.end > self.begin))
        return {n: rows_of.get(n, np.zeros(0, _segment_dtype())) for n in names}


class Rows(dict):
    """{contig: SEGMENT_DTYPE rows}; `lines[contig]`: the line of the listing each row came from (None for a table);
    `millidiv[contig]`: the divergence of each row in tenths of a percent, -1 where not stated (None for a table: all -1).
    From evaluation_rows(offtarget=True) also the UN-MODELLED rows of the listing: `offtarget_rows[contig]` (SEGMENT_DTYPE, label =
    the row's number, 0 where it has none), `offtarget_keys[contig]` (uint32: 64 + family id) and `families` (the tokens in id order)."""
    lines: Optional[Dict[str, np.ndarray]] = None
    millidiv: Optional[Dict[str, np.ndarray]] = None
    route: str = "table"
    offtarget_rows: Optional[Dict[str, np.ndarray]] = None
    offtarget_keys: Optional[Dict[str, np.ndarray]] = None
    families: Optional[List[str]] = None


def _runs_of(names: List[str]):
    first = [i for i in range(len(names)) if i == 0 or names[i] != names[i - 1]]
    return np.asarray(first + [len(names)], np.int64), [names[i] for i in first]


def family_ranks(tokens: Sequence[str]):
    """(family_id int32 per token, the distinct tokens in id order): ranks in ascending order of the tokens' bytes (UTF-8), a proper
    prefix first -- the order dgrp_token_ids states."""
    raw = [t.encode("utf-8", "surrogateescape") for t in tokens]
    distinct = sorted(set(raw))
    rank = {t: k for k, t in enumerate(distinct)}
    return (np.fromiter((rank[t] for t in raw), np.int32, count=len(raw)), [t.decode("utf-8", "surrogateescape") for t in distinct])


def _listing_host_all(path) -> Listing:
    """The host path for ALL rows: every line parse_rm.parse_line finds a contig in is a row, numbered as read_repeatmasker numbers
    it (0 where that yields nothing), with its family token as parse_line states it."""
    from .evaluation import AnnotationError
    exact, one_off = parse_rm.pentamer_sets()
    names, vals, fams = [], [], []
    k = 0
    for k, line in enumerate(io.StringIO(_read_text(path)), 1):
        r = parse_rm.parse_line(line)
        if r.ctg is None:
            continue
        for what, v in (("begin", r.start), ("end", r.end)):
            if not -(1 << 63) <= v < (1 << 63):
                raise AnnotationError(f"{path}:{k}: {what} '{v}' is not an integer: {line.rstrip()!r}")
        numbered = list(parse_rm.read_repeatmasker(exact, one_off, [line]))
        names.append(r.ctg)
        fams.append(r.fam)
        vals.append((r.start, r.end, numbered[0].typ if numbered else 0, k, millidiv_of_line(line)))
    a = np.asarray(vals, np.int64).reshape(-1, 5)
    run_first, run_names = _runs_of(names)
    fid, families = family_ranks(fams)
    return Listing(path, a[:, 0], a[:, 1], a[:, 2], a[:, 3], run_first, run_names, k, "host", a[:, 4], fid, families)


def _listing_host(path, all_rows: bool = False) -> Listing:
    """The host path: parse_rm.read_repeatmasker on the decoded text."""
    if all_rows:
        return _listing_host_all(path)
    from .evaluation import AnnotationError
    exact, one_off = parse_rm.pentamer_sets()
    at = [0]

    def numbered(fh):
        for k, line in enumerate(fh, 1):
            at[0] = k
            yield line
    names, vals = [], []
    now = [""]

    def noted(lines):
        for line in lines:
            now[0] = line
            yield line
    for r in parse_rm.read_repeatmasker(exact, one_off, noted(numbered(io.StringIO(_read_text(path))))):
        for what, v in (("begin", r.start), ("end", r.end)):
            if not -(1 << 63) <= v < (1 << 63):
                raise AnnotationError(f"{path}:{at[0]}: {what} '{v}' is not an integer: {line_text(path, at[0]).rstrip()!r}")
        names.append(r.ctg)
        vals.append((r.start, r.end, r.typ, at[0], millidiv_of_line(now[0])))
    a = np.asarray(vals, np.int64).reshape(-1, 5)
    run_first, run_names = _runs_of(names)
    return Listing(path, a[:, 0], a[:, 1], a[:, 2], a[:, 3], run_first, run_names, at[0], "host", a[:, 4])


_DEVICE_TABLES: Dict[object, tuple] = {}


def _device_tables(dev):
    import torch
    if dev not in _DEVICE_TABLES:
        blob, off, pent, unit = tables()
        _DEVICE_TABLES[dev] = (torch.from_numpy(blob).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(pent).to(dev),
                               len(parse_rm.REPEATS), unit)
    return _DEVICE_TABLES[dev]


def parse_device(d_text, n: Optional[int] = None, cap: Optional[int] = None, fields: bool = False, all_rows: bool = False):
    """dgrp_rm_parse on the uint8 device tensor `d_text` (its first `n` bytes): -> (counts = [lines, kept rows, runs, not-plain
    flag], the device arrays begin, end, number, name_pos, name_len, line, run_first of `cap` rows -- default n // 22 + 1 --, the
    return code).  Nothing is raised for DGRP_ENOMEM (-3: more rows than `cap`; counts[1] tells the need).  fields:
    dgrp_rm_parse_fields, and `millidiv` among the arrays.  all_rows: dgrp_rm_parse_all -- every matching line is a row -- with
    `millidiv` and the family spans `fam_pos`, `fam_len`, `fam2_pos`, `fam2_len` among the arrays."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    n = int(d_text.numel()) if n is None else int(n)
    dev = d_text.device
    d_names, d_off, d_pent, nnames, unit = _device_tables(dev)
    cap = n // MIN_LINE_BYTES + 1 if cap is None else int(cap)
    i64 = lambda: torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    i32 = lambda: torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    out = dict(begin=i64(), end=i64(), number=i32(), name_pos=i64(), name_len=i32(), line=i64(), run_first=i64())
    wb = int(L.dgrp_rm_parse_all_workspace_bytes(n) if all_rows else L.dgrp_rm_parse_workspace_bytes(n))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    counts = (C.c_int64 * 4)()
    head = (d_text.data_ptr() if n else None, n, d_names.data_ptr(), d_off.data_ptr(), nnames, d_pent.data_ptr(), unit,
            out["begin"].data_ptr(), out["end"].data_ptr(), out["number"].data_ptr(), out["name_pos"].data_ptr(),
            out["name_len"].data_ptr(), out["line"].data_ptr(), out["run_first"].data_ptr())
    tail = (cap, counts, work.data_ptr(), wb, stream_ptr())
    if all_rows:
        out.update(millidiv=i32(), fam_pos=i64(), fam_len=i32(), fam2_pos=i64(), fam2_len=i32())
        rc = L.dgrp_rm_parse_all(*head, *(out[k].data_ptr() for k in ("millidiv", "fam_pos", "fam_len", "fam2_pos", "fam2_len")), *tail)
    elif fields:
        out["millidiv"] = i32()
        rc = L.dgrp_rm_parse_fields(*head, out["millidiv"].data_ptr(), *tail)
    else:
        rc = L.dgrp_rm_parse(*head, *tail)
    if rc not in (0, -3):
        check(rc, "dgrp_rm_parse_all" if all_rows else "dgrp_rm_parse_fields" if fields else "dgrp_rm_parse")
    return [int(c) for c in counts], out, rc


TOKEN_MAX = 16384                        # DGRP_TOKEN_MAX: distinct tokens the device numbers
NAMES_BYTES = 1 << 20                    # room for the distinct tokens' bytes; the call tells the need when it is more


def token_ids_device(d_text, n: int, rows: int, d_pos, d_len, d_pos2, d_len2, names_cap: int = NAMES_BYTES):
    """dgrp_token_ids on `rows` tokens given as spans of the uint8 device tensor `d_text`: -> (int32 device tensor of ids, the
    distinct tokens in id order as bytes), or None when there are more than TOKEN_MAX distinct tokens (the overflow flag)."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    dev = d_text.device
    d_fid = torch.empty(max(rows, 1), dtype=torch.int32, device=dev)
    for _attempt in range(2):
        wb = int(L.dgrp_token_ids_workspace_bytes(rows, names_cap))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        names = np.zeros(max(names_cap, 1), np.uint8)
        off = np.zeros(TOKEN_MAX + 1, np.int64)
        counts = (C.c_int64 * 3)()
        rc = L.dgrp_token_ids(d_text.data_ptr(), int(n), int(rows), d_pos.data_ptr(), d_len.data_ptr(), d_pos2.data_ptr(), d_len2.data_ptr(),
                              d_fid.data_ptr(), names.ctypes.data, names_cap, off.ctypes.data, counts, work.data_ptr(), wb, stream_ptr())
        if rc == -3 and int(counts[2]) > names_cap:
            names_cap = int(counts[2])
            continue
        check(rc, "dgrp_token_ids")
        break
    if counts[1]:
        return None
    F = int(counts[0])
    blob = names.tobytes()
    return d_fid[:rows], [blob[int(off[k]):int(off[k + 1])] for k in range(F)]


def listing_of_device_text(path, d_text, n: int, all_rows: bool = False) -> Optional[Listing]:
    """The Listing of the text in device memory, or None when the device raised the not-plain flag -- or, with all_rows, the
    overflow flag of the family ids."""
    import torch
    counts, out, rc = parse_device(d_text, n, fields=True, all_rows=all_rows)
    if counts[3]:
        return None
    if rc != 0:
        from ._lib import check
        check(rc, "dgrp_rm_parse_all" if all_rows else "dgrp_rm_parse_fields")
    lines, kept, runs = counts[:3]
    fid = families = None
    if all_rows:
        ids = token_ids_device(d_text, n, kept, out["fam_pos"], out["fam_len"], out["fam2_pos"], out["fam2_len"])
        if ids is None:
            return None
        fid, families = ids[0].cpu().numpy(), [t.decode("ascii") for t in ids[1]]
    host = lambda k: out[k][:kept].cpu().numpy()
    first = out["run_first"][:runs]
    names: List[str] = []
    if runs:
        # one name per run: their bytes in one gather and one copy
        pos, ln = out["name_pos"][first], out["name_len"][first].to(torch.int64)
        total = int(ln.sum())
        offs = torch.cumsum(ln, 0) - ln
        shift = torch.repeat_interleave(pos - offs, ln, output_size=total)
        blob = d_text[torch.arange(total, device=d_text.device) + shift].cpu().numpy().tobytes()
        cut = np.concatenate([offs.cpu().numpy(), [total]])
        names = [blob[cut[r]:cut[r + 1]].decode("ascii") for r in range(runs)]
    run_first = np.concatenate([first.cpu().numpy(), [kept]]).astype(np.int64)
    return Listing(path, host("begin"), host("end"), host("number"), host("line"), run_first, names, lines, "device", host("millidiv"),
                   fid, families)


def read_listing(path, device: bool = True, all_rows: bool = False) -> Listing:
    """The numbered rows of the RepeatMasker listing `path` (plain, gzip or BGZF): parsed on the device, or by the host path (module
    docstring) with device=False, on the not-plain flag and above the resident-bytes limit.  all_rows: EVERY row that matches a
    pattern, with `family_id` and `families` (dgrp_rm_parse_all, dgrp_token_ids; more than TOKEN_MAX distinct family tokens take the
    host path too)."""
    if not device:
        return _listing_host(path, all_rows)
    from . import gz
    from .fasta import RESIDENT_BYTES, _upload_file
    from .pipeline import require_gpu
    if gz.is_gzip(path):
        try:
            _text, d_text, size = gz.open_inflated(path, RESIDENT_BYTES, require_gpu, _upload_file)
        except gz.GzipError:
            raise
        except ValueError:                                           # inflates to more than the limit
            return _listing_host(path, all_rows)
    else:
        size = os.path.getsize(path)
        if size > RESIDENT_BYTES:
            return _listing_host(path, all_rows)
        d_text = _upload_file(path, size, require_gpu()) if size else None
    if size == 0:
        return Listing(path, [], [], [], [], [0], [], 0, "device", None, [] if all_rows else None, [] if all_rows else None)
    got = listing_of_device_text(path, d_text, size, all_rows)
    return _listing_host(path, all_rows) if got is None else got


def read_rows(path, fmt: str = "auto", device: bool = True) -> Rows:
    """{contig: SEGMENT_DTYPE rows} of the annotation `path`, label = repeat number, file order within a contig: for a RepeatMasker
    listing exactly what evaluation.read_annotation(table, None) returns for the table parse_rm writes from it, with `.lines` =
    {contig: the listing's line of every row}; for a table read_annotation itself (`.lines` None)."""
    fmt = resolve_format(path, fmt)
    if fmt == "gff3":
        raise ValueError(f"{path}: GFF3 is read with names for its labels: gffin.read_annotation")
    if fmt == "table":
        from .evaluation import read_annotation
        return Rows(read_annotation(path, None))
    listing = read_listing(path, device)
    rows_of, lines_of, div_of = listing.grouped_fields(listing.table_mask())
    out = Rows(rows_of)
    out.lines, out.millidiv, out.route = lines_of, div_of, listing.route
    return out


def evaluation_rows(path, repeats: Optional[Iterable[int]] = None, device: bool = True, offtarget: bool = False) -> Rows:
    """evaluation.read_annotation(table of the listing `path`, repeats) without the table: the same rows, and the same
    AnnotationError for a negative begin or an end below its begin -- checked on every row before `repeats` filters, the first in
    file order named as "<listing>:<its line>: <why>: <the line>".  `.lines` and `.millidiv` travel beside the rows.
    offtarget: the listing is parsed once for ALL its rows; the rows kept without it are the MODELLED rows and are returned as
    before, every other row -- no number, or a number outside `repeats` -- is un-modelled and travels as `.offtarget_rows`,
    `.offtarget_keys` (64 + family id) and `.families`; the two checks then apply to every row of the listing."""
    listing = read_listing(path, device, all_rows=offtarget)
    if offtarget and len(listing.families) > TOKEN_MAX:
        from .evaluation import AnnotationError
        raise AnnotationError(f"{path}: {len(listing.families)} distinct class/family tokens; --offtarget has room for {TOKEN_MAX}")
    read = listing.table_mask()
    if offtarget:
        read &= listing.number > 0
        bad = np.flatnonzero((listing.begin < 0) | (listing.end < listing.begin))
        if bad.size:
            k = int(bad[0])
            raise listing._bad(k, "negative begin" if listing.begin[k] < 0 else "end below begin")
    bad = np.flatnonzero(read & ((listing.begin < 0) | (listing.end < listing.begin)))
    if bad.size:
        k = int(bad[0])
        raise listing._bad(k, "negative begin" if listing.begin[k] < 0 else "end below begin")
    if repeats is not None:
        read &= np.isin(listing.number, np.array(sorted(set(int(r) for r in repeats)), np.int64))
    rows_of, lines_of, div_of = listing.grouped_fields(read)
    out = Rows(rows_of)
    out.lines, out.millidiv, out.route = lines_of, div_of, listing.route
    if offtarget:
        out.offtarget_rows, out.offtarget_keys, out.families = {}, {}, list(listing.families)
        for name, sel in listing.grouped_index(~read).items():
            rows = np.zeros(sel.size, _segment_dtype())
            rows["start"], rows["end"], rows["label"] = listing.begin[sel], listing.end[sel], listing.number[sel]
            out.offtarget_rows[name] = rows
            out.offtarget_keys[name] = (64 + listing.family_id[sel].astype(np.int64)).astype(np.uint32)
    return out


def refuse_npz(command: str, path) -> str:
    """The refusal of a RepeatMasker listing where only the table is read (.npz sides of `train`, `optimize`)."""
    return (f"{command}: {path} is RepeatMasker output, and with .npz inputs the annotation is read as the table of parse_rm: write it "
            f"with `python -m deepgrp_amd._scripts.parse_rm {path} -o table.bed`, or give `train` sequence files (FASTA, gzip, BGZF, "
            ".2bit) as trainfile and validfile, which takes the listing itself")
