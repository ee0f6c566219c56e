"""RepeatMasker `.out` listing of the scored repeats (`predict --bed_dir DIR --bed_rmout`): for every input file one
`DIR/<basename>.out` in the place of the `.bed` (`.out.gz`, BGZF, with --bed_gzip), the format the project's own readers take as an
ANNOTATION (annotation.py, `parse_rm`) and that repeat tooling downstream of RepeatMasker expects.

The file.  It begins with HEADER -- RepeatMasker's two title lines, spaced to stand over the columns at their minimum widths, and one
empty line -- also when the input has no row (in a `.out.gz` the header is a BGZF member of its own).  Then one line per emitted row
(score >= --bed_min_score), in TSV order, the Python expression

    b"%5d %5s %4s %4s  %-16s %9d %9d %11s +  %-12s %-16s %6d %6d %6s %6d\\n" % (
        score, b"0.0", b"0.0", b"0.0", name, start + 1, end, b"(%d)" % (rec_end - end),
        repeat, family, 1, end - start, b"(0)", ident)

in which a field longer than its width grows, exactly as `%` does.  score is the BED line's score 0..1000, R(sum, bases * 2^24, 1000)
of bed.py; name the record's name (evaluation.record_name); start and end the TSV's (the listing is 1-based and closed, hence
start + 1); rec_end the record's end coordinate as the bigBed and tabix entries receive it, startpos + the record's evaluated bases:
TRAILING N BASES ARE NOT COUNTED IN `(left)`.  The position in the repeat is written 1 .. end - start with nothing left.

WHAT THE MODEL DOES NOT PREDICT.  Divergence, deletions and insertions are written `0.0` and the strand is always `+`: the model
predicts none of them.  A consumer must not read a divergence (or a strand) out of this file; the columns are there because the
format has them.

Names of a label L (1..C-1).  By default they come from the repeat number n = repeats[L - 1] (--rmout_repeats, 1..C-1 unless given)
and parse_rm.REPEATS[n - 1]: `HSATII` gives (`HSATII`, `Satellite`), `ALR/Alpha` gives (`ALR/Alpha`, `Satellite/centr`), every other
`X/Y` gives (`Y`, `X/Y`) -- the pairs parse_rm.parse_line numbers back to n (`pairs_of_repeats`).  With --bed_names entry L is
`repeat#class/family`, the naming of RepeatMasker's libraries, split at its only `#` (`pairs_of_names`, `names_refusal`): other
species, more than ten labels.

IDs.  ident runs through the file from 1.  Without --rmout_join every line has its own.  With --rmout_join G (G >= 0) an emitted row
takes the ID of the emitted row directly in front of it when both are rows of the same record, both have the same label and
start - previous end <= G: RepeatMasker's meaning of a shared ID, fragments of one element (the counterpart on the prediction side of
`evaluate --boundary_join`).  A filtered row neither joins nor breaks a run of its neighbours.  Internally no join is G = -1.

A record name that is empty or holds a byte <= 0x20 or 0x7f cannot stand in a blank-separated column (`record_name_refusal`): the
input gets one warning and no `.out`.

`HEADER`, `reference_lines` and `reference_ids` are the statements the device entry (dgrp_rmout_text_batch) and `BedFiles` are tested
against, in Python integers and bytes only."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

from ._scripts import parse_rm

HEADER = (b"   SW   perc perc perc  query           position in query                  matching     repeat           position in repeat\n"
          b"score   div. del. ins.  sequence            begin       end      (left)    repeat       class/family      begin    end (left)     ID\n"
          b"\n")
LINE = b"%5d %5s %4s %4s  %-16s %9d %9d %11s +  %-12s %-16s %6d %6d %6s %6d\n"
MAX_NAME = 255                                      # bytes of a --bed_names entry
MAX_REPEATS = len(parse_rm.REPEATS)
NO_JOIN = -1


def _raw(name) -> bytes:
    return name if isinstance(name, bytes) else name.encode("utf-8", "surrogateescape")


def _blank(raw: bytes) -> bool:
    return any(b <= 0x20 or b == 0x7f for b in raw)


def pair_of_repeat(n: int) -> Tuple[bytes, bytes]:
    """(repeat, class/family) of repeat number n (1..10): the pair parse_rm.parse_line numbers back to n."""
    if not 1 <= n <= MAX_REPEATS:
        raise ValueError(f"repeat number {n} outside 1..{MAX_REPEATS}")
    name = parse_rm.REPEATS[n - 1]
    if name == "HSATII":
        return b"HSATII", b"Satellite"
    if name == "ALR/Alpha":
        return b"ALR/Alpha", b"Satellite/centr"
    return name.split("/", 1)[1].encode(), name.encode()


def pairs_of_repeats(repeats: Sequence[int]) -> Tuple[Tuple[bytes, bytes], ...]:
    return tuple(pair_of_repeat(int(n)) for n in repeats)


def names_refusal(names: Sequence) -> Optional[str]:
    """Why --bed_names cannot name the labels of a listing (`repeat#class/family`), or None."""
    for i, nm in enumerate(names):
        raw = _raw(nm)
        if len(raw) > MAX_NAME:
            return f"--bed_names: the name of label {i + 1} has {len(raw)} bytes, above {MAX_NAME}"
        if raw.count(b"#") != 1:
            return (f"--bed_names: with --bed_rmout the name of label {i + 1} must be repeat#class/family with exactly one '#', "
                    f"not {raw.decode('utf-8', 'replace')!r}")
        if not all(raw.split(b"#")):
            return f"--bed_names: the name of label {i + 1} has an empty side of its '#' (repeat#class/family)"
        if _blank(raw):
            return (f"--bed_names: the name of label {i + 1} holds a blank or a control character, which cannot stand in a "
                    "blank-separated column of the listing")
    return None


def pairs_of_names(names: Sequence) -> Tuple[Tuple[bytes, bytes], ...]:
    """--bed_names entries `repeat#class/family` -> ((repeat, class/family), ...); names_refusal has passed them."""
    why = names_refusal(names)
    if why is not None:
        raise ValueError(why)
    return tuple(tuple(_raw(nm).split(b"#")) for nm in names)


def repeats_refusal(repeats: Sequence[int]) -> Optional[str]:
    """Why --rmout_repeats cannot be these numbers, or None."""
    if not repeats:
        return "--rmout_repeats: no number given"
    for n in repeats:
        if not 1 <= n <= MAX_REPEATS:
            return f"--rmout_repeats: {n} lies outside 1..{MAX_REPEATS} (the numbered families of parse_rm)"
    if len(set(repeats)) != len(repeats):
        return "--rmout_repeats: the numbers must be distinct"
    return None


def record_name_refusal(name) -> Optional[str]:
    """Why a record of this name cannot be written to a listing, or None."""
    raw = _raw(name)
    if not raw:
        return "a record with an empty name"
    if _blank(raw):
        return f"the record name {raw.decode('utf-8', 'replace')!r} holds a blank or a control character"
    return None


class RmoutText(NamedTuple):
    """What one write adds to the file once its first ID is known: `data` (the text of a plain `.out`, the BGZF members without EOF
    member of a `.out.gz`), the lines in it and the IDs they use."""
    data: bytes
    lines: int
    ids: int


class RmoutWrite(NamedTuple):
    """One write (a record, or a batch) of a listing: the records' names as they come and `render(id0) -> RmoutText`, called by
    `BedFiles.write` with the IDs the file has used so far.  render None: no row."""
    names: List[bytes]
    render: Optional[Callable[[int], RmoutText]] = None


# ---- the statements ------------------------------------------------------------------------------------------------------------------
def reference_ids(rows, emitted: Sequence[bool], by_contig: bool, join_gap: Optional[int] = None, id0: int = 0) -> Tuple[List[int], int]:
    """-> (the ID of every emitted row, in order; the number of IDs used).  join_gap None or -1: every row its own ID."""
    gap = NO_JOIN if join_gap is None else int(join_gap)
    if gap < NO_JOIN:
        raise ValueError("join gap below -1")
    if id0 < 0:
        raise ValueError("id0 below 0")
    ids: List[int] = []
    used, prev = 0, None
    for row, keep in zip(rows, emitted):
        if not keep:
            continue
        key = (int(row["contig"]) if by_contig else 0, int(row["label"]))
        joins = gap >= 0 and prev is not None and prev[0] == key and int(row["start"]) - prev[1] <= gap
        if not joins:
            used += 1
        ids.append(id0 + used)
        prev = (key, int(row["end"]))
    return ids, used


def reference_lines(names: Sequence, by_contig: bool, rows, scores, min_score: int, rec_end: Sequence[int], pairs: Sequence,
                    join_gap: Optional[int] = None, id0: int = 0) -> Tuple[bytes, int, int]:
    """The lines (no header) in Python integers -> (text, lines, IDs used).  names as they come; pairs[L - 1] = (repeat,
    class/family) of label L; rec_end[r] the end coordinate of record r (a row's contig with by_contig, else 0)."""
    from .bed import _half_up
    raw = [_raw(nm) for nm in names]
    figures = []
    for row, sc in zip(rows, scores):
        total, bases = int(sc["sum"]), int(sc["bases"])
        if bases <= 0:
            raise ValueError("a row without a scored base")
        figures.append(_half_up(total, bases << 24, 1000))
    emitted = [f >= min_score for f in figures]
    ids, used = reference_ids(rows, emitted, by_contig, join_gap, id0)
    out = []
    for row, score, keep in zip(rows, figures, emitted):
        if not keep:
            continue
        r = int(row["contig"]) if by_contig else 0
        start, end, label = int(row["start"]), int(row["end"]), int(row["label"])
        if not 1 <= label <= len(pairs):
            raise ValueError(f"label {label} outside the {len(pairs)} names")
        if not (0 <= start < end <= int(rec_end[r])):
            raise ValueError(f"row [{start}, {end}) outside its record [0, {int(rec_end[r])})")
        repeat, family = pairs[label - 1]
        out.append(LINE % (score, b"0.0", b"0.0", b"0.0", raw[r], start + 1, end, b"(%d)" % (int(rec_end[r]) - end),
                           _raw(repeat), _raw(family), 1, end - start, b"(0)", ids[len(out)]))
    return b"".join(out), len(out), used


def header_member(level: int) -> bytes:
    """HEADER as the BGZF member a `.out.gz` begins with (the library's host encoder, as the device writes the members behind it)."""
    from .gz import bgzf_compress_host
    return bgzf_compress_host(HEADER, eof=False, level=level)
