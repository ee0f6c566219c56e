"""Inputs shared by the tests of `compare` and dgrp_rows_parse: seeded texts whose lines meet the 128-byte chunks and the 32768-byte
tiles of the device parser in every way, and hand-made foreign rows for the flattening rule."""
import numpy as np

CHUNK, TILE = 128, 32768
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


def _aligned(out, line, eol, rng, pad):
    """`line` padded so that it (with its line end) ends exactly on a chunk boundary -- on the tile boundary where one is near."""
    at = len(out) + len(line) + len(eol)
    to_tile = -at % TILE
    if to_tile < 400 and (at // TILE) % 2 == 1:
        return line                                                              # every second tile boundary is straddled
    want = to_tile if to_tile < 400 else -at % CHUNK
    if want == 0:
        return line
    if want < 2:
        want += CHUNK
    return line + pad(want)


def table_text(seed=0, size=3 * TILE + 2000):
    """About three tiles of a `contig begin end number` table: blank lines, '#' lines, CRLF, leading blanks, tabs and spaces mixed,
    extra columns, 18-digit coordinates; every few lines one ends exactly on a chunk boundary, near the first and the third tile
    boundary on the tile boundary (so the next line starts there); the second tile boundary and most chunk boundaries are straddled."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    names = ["chr1", "chr2", "scaffold_0012", "chrUn_KI270302v1", "x", "#not_a_contig"]
    name = names[0]
    seps = [b" ", b"\t", b"  ", b" \t", b"\t\t "]
    sep = lambda: seps[int(rng.integers(0, len(seps)))]
    pad = lambda k: sep()[:1] + b"p" * (k - 1)                                   # one more column
    k = 0
    while len(out) < size:
        k += 1
        kind = int(rng.integers(0, 14))
        eol = b"\r\n" if rng.random() < 0.15 else b"\n"
        if rng.random() < 0.1:
            name = names[int(rng.integers(0, len(names)))]
        if kind == 0:
            line = b""
        elif kind == 1:
            line = b"# a comment line " + str(k).encode()
        elif kind == 2:
            line = b"  \t "
        else:
            begin = int(rng.integers(0, 10 ** 9)) if kind != 3 else 10 ** 17 + int(rng.integers(0, 10 ** 15))
            end = begin + int(rng.integers(0, 5000))
            lead = sep() if rng.random() < 0.2 else b""
            line = lead + name.encode() + sep() + str(begin).encode() + sep() + str(end).encode() + sep() + str(int(rng.integers(0, 9))).encode()
            if rng.random() < 0.4:
                line += sep() + b"name" + sep() + b"fam/ily extra"
            if rng.random() < 0.1:
                line += sep()                                                    # trailing blanks
            if k % 5 == 0 or -(len(out) + len(line) + len(eol)) % TILE < 400:
                line = _aligned(out, line, eol, rng, pad)
        out += line + eol
    out += b"chr1 5 9 2"                                                         # no final newline
    return bytes(out)


def tsv_text(seed=0, size=3 * TILE + 2000):
    """The same for a prediction TSV: file, header (spaces and tabs inside), start, end, label; `.npz` file fields; CRLF; empty
    lines."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    recs = [("genome.fa", "chr1"), ("genome.fa", "chr2 assembled by hand"), ("genome.fa", "chr3\twith\ttabs in it"),
            ("genome.fa", "  chr4 after blanks"), ("data/run1/chrA.fa.gz.npz", "chrA.fa.gz"), ("/abs/chrB.npz", "whatever here"),
            ("other.fa", ""), ("-", "stdin_rec x")]
    rec = recs[0]
    k = 0
    while len(out) < size:
        k += 1
        eol = b"\r\n" if rng.random() < 0.15 else b"\n"
        if rng.random() < 0.05:
            out += eol
            continue
        if rng.random() < 0.1:
            rec = recs[int(rng.integers(0, len(recs)))]
        begin = int(rng.integers(0, 10 ** 9)) if k % 11 else 10 ** 17 + int(rng.integers(0, 10 ** 15))
        header = rec[1]
        tail = f"\t{begin}\t{begin + int(rng.integers(1, 5000))}\t{int(rng.integers(1, 5))}".encode()
        line = rec[0].encode() + b"\t" + header.encode()
        if k % 5 == 0 or -(len(out) + len(line) + len(tail) + len(eol)) % TILE < 400:
            at = len(out) + len(line) + len(tail) + len(eol)
            to_tile = -at % TILE
            want = to_tile if to_tile < 400 else -at % CHUNK
            if to_tile < 400 and (at // TILE) % 2 == 1:
                want = 0                                                         # every second tile boundary is straddled
            if 0 < want < 2:
                want += CHUNK
            if want and not rec[0].endswith(".npz") and header.split():         # (the header grows; its first word stays)
                line += b" " + b"h" * (want - 1)
        out += line + tail + eol
    out += b"genome.fa\tchr1\t5\t9\t2"
    return bytes(out)


def boundary_profile(text: bytes):
    """How the lines of `text` meet the boundaries: (lines that start on a chunk boundary, on a tile boundary, lines that straddle a
    tile boundary)."""
    starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10 and i + 1 < len(text)]
    ends = starts[1:] + [len(text)]
    on_chunk = sum(1 for s in starts if s % CHUNK == 0)
    on_tile = sum(1 for s in starts if s % TILE == 0 and s)
    straddle = sum(1 for s, e in zip(starts, ends) if s // TILE != (e - 1) // TILE)
    return on_chunk, on_tile, straddle


def rows(*triples):
    out = np.zeros(len(triples), SEG)
    for k, (s, e, lab) in enumerate(triples):
        out[k] = (s, e, lab, 0)
    return out


# Foreign rows on a record whose evaluated span is [100, 160): (rows, what flattening must give)
FOREIGN = {
    "nested": (rows((110, 140, 3), (120, 130, 1)), rows((110, 120, 3), (120, 130, 1), (130, 140, 3))),
    "nested_larger_inside": (rows((110, 140, 1), (120, 130, 3)), rows((110, 140, 1))),
    "overlap_smallest_wins": (rows((110, 130, 2), (125, 150, 1)), rows((110, 125, 2), (125, 150, 1))),
    "abutting_same_label": (rows((110, 120, 2), (120, 135, 2)), rows((110, 135, 2))),
    "unsorted": (rows((140, 150, 4), (105, 110, 1)), rows((105, 110, 1), (140, 150, 4))),
    "sticks_out": (rows((90, 105, 2), (150, 170, 3)), rows((100, 105, 2), (150, 159, 3), (159, 160, 3))),
    "last_base_rule": (rows((155, 160, 1)), rows((155, 159, 1), (159, 160, 1))),
    "last_base_alone": (rows((159, 160, 2)), rows((159, 160, 2))),
    "outside": (rows((10, 50, 1), (160, 190, 2)), rows()),
    "duplicate": (rows((110, 120, 1), (110, 120, 1)), rows((110, 120, 1))),
}
FOREIGN_SPAN = (100, 60)
