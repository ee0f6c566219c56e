"""Shared by the --mask_twobit tests: the 2bit file of a masked text, stated a second time.  The building blocks are
twobit_corpus.pack_dna / twobit_corpus.write and a per-character statement of the rules (regular expressions over the sequence
characters); nothing here comes from deepgrp_amd/twobit.py.  And the cases: the smallest record bodies at which the packing
kernels can go wrong."""
import re

import numpy as np

import twobit_corpus as tc

TILE = 4096                                     # text bytes of one workgroup of the kernels as built
_TWO = {c: i for i, c in enumerate(b"TCAG")}
_TWO.update({c | 0x20: i for c, i in list(_TWO.items())})
_N_RUN = re.compile(rb"[^ACGTacgt]+")            # any other sequence character is N
_MASK_RUN = re.compile(rb"[a-z]+")               # a lower-case character lies in a mask block
_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)?")  # text mode's universal newlines
_STRIP = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"


def sequence(body: bytes) -> bytes:
    """The sequence characters of a plain record body: every byte that is neither CR nor LF."""
    return body.replace(b"\r", b"").replace(b"\n", b"")


def rec(name: bytes, seq: bytes) -> tc.Rec:
    """The record of the sequence characters `seq`: two bits per base (N: 0), the maximal runs as blocks, zero padding."""
    codes = np.array([_TWO.get(c, 0) for c in seq], np.uint8)
    blocks = lambda rx: [(m.start(), m.end() - m.start()) for m in rx.finditer(seq)]
    return tc.Rec(name, codes, blocks(_N_RUN), blocks(_MASK_RUN), np.zeros(3, np.uint8))


def blob(seq: bytes) -> bytes:
    """The record blob: what follows the 16-byte header and the 9-byte index of a one-record file with a four-byte name."""
    return tc.write([rec(b"name", seq)])[25:]


def counts(seq: bytes):
    r = rec(b"", seq)
    return [len(seq), len(r.nblocks), len(r.mblocks)]


def records(text: bytes):
    """[(name, sequence characters)] of the records the reference's line loop yields from `text` (ASCII): lines stripped, a line
    that starts with '>' opens a record, a record without a header or with an empty one is none; the name is the first word."""
    out, header, parts = [], b"", []
    for m in _LINE.finditer(text):
        line = m.group().strip(_STRIP)
        if not m.group():
            continue
        if line[:1] == b">":
            if header:
                out.append((header.split()[0], b"".join(parts)))
            header, parts = line[1:], []
        else:
            parts.append(line)
    if header:
        out.append((header.split()[0], b"".join(parts)))
    return out


def file_of(text: bytes) -> bytes:
    """The 2bit file of the masked text."""
    return tc.write([rec(name, seq) for name, seq in records(text)])


def normalised(text: bytes) -> bytes:
    """What reading the 2bit file back as text gives: names cut to their first word, 50 bases per line, non-ACGT letters N or n."""
    out = []
    for name, seq in records(text):
        seq = bytes((c if c in _TWO else (110 if 97 <= c <= 122 else 78)) for c in seq)
        out.append(b">" + name + b"\n" + b"".join(seq[o:o + 50] + b"\n" for o in range(0, len(seq), 50)))
    return b"".join(out)


def lay(seq: bytes, width: int, eol: bytes = b"\n", last: bool = True) -> bytes:
    """`seq` as a record body: `width` characters per line, every line ended by `eol`, the last one only with `last`."""
    lines = [seq[o:o + width] for o in range(0, len(seq), width)]
    body = eol.join(lines) + (eol if lines and last else b"")
    return body


def _mixed(rng, n):
    """ACGT in both cases with N, n and IUPAC letters sprinkled in, in runs of 1..6."""
    out = bytearray()
    alphabets = (b"ACGT", b"ACGT", b"acgt", b"N", b"n", b"RYKMSWBDHV", b"rykmswbdhv")
    while len(out) < n:
        ab = alphabets[int(rng.integers(0, len(alphabets)))]
        out += bytes(ab[int(i)] for i in rng.integers(0, len(ab), int(rng.integers(1, 7))))
    return bytes(out[:n])


def body_cases():
    """[(label, record body)]: the sizes, line layouts and runs of the issue, none longer than a few tiles."""
    rng = np.random.default_rng(tc.SEED + 40)
    cases = []
    add = lambda label, body: cases.append((label, bytes(body)))
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65):
        add(f"size{n}", lay(_mixed(rng, n), 60))
        add(f"size{n}_acgt", lay(bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)), 60, last=False))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 37):
        add(f"oneline{n}", _mixed(rng, n))                               # no line end: sequence bytes = text bytes
        add(f"size{n}", lay(_mixed(rng, n), 60))
    add("lineends_only", b"\n\n\r\n\n")
    add("empty", b"")
    seq = _mixed(rng, 301)
    for width in (1, 3, 50, 60, 61):
        for eol in (b"\n", b"\r\n"):
            for last in (True, False):
                add(f"w{width}_{len(eol)}_{int(last)}", lay(seq, width, eol, last))
    big = 2 * TILE + 3
    add("runs_of_1", lay(b"ACnGTaCNGtANcG" * 9, 50))
    add("case_alternates", lay(b"aC" * 100, 60))
    add("case_alternates_tiles", lay(b"gT" * (big // 2) + b"a", 61, b"\r\n"))
    add("n_alternates", lay(b"NA" * 100, 60))
    add("n_alternates_tiles", lay(b"AN" * (big // 2) + b"N", 61))
    add("n_alternates_lower", lay(b"nA" * 77, 3))
    add("run_at_0", lay(b"nnnacgACGT" * 7, 50))
    add("run_to_the_end", lay(b"ACGTACGTAC" * 7 + b"acgNN", 50))
    add("run_is_the_last_base", lay(b"ACGT" * 16 + b"n", 60, last=False))
    # the tile edge lies TILE bytes behind the 16-byte word in which the body starts: 16-byte aligned bodies have it at byte TILE
    up, lo = b"ACGT" * (TILE // 4), b"acgt" * 8
    add("run_starts_the_tile", up + lo + b"ACGTAC")
    add("run_crosses_the_tile", up[:-5] + lo + b"ACG")
    add("run_ends_with_the_tile", up[:-32] + lo + b"ACGTA")
    add("lf_before_the_tile_run", up[:-1] + b"\n" + lo + b"AC\n")
    add("crlf_straddles_the_tile_run", up[:-1] + b"\r\n" + lo + b"AC\r\n")
    add("crlf_straddles_the_tile_open_run", up[:-9] + b"nnnnnnnn" + b"\r\n" + b"nnnACGT\r\n")
    add("crlf_before_the_tile_n_run", up[:-2] + b"\r\n" + b"NNNNACGT")
    add("n_inside_mask", lay(b"ACGTacgtnnnacgtACGT", 60))
    add("n_overlaps_mask", lay(b"ACGTacgtnnNNNACGTNNnnacgA", 60))
    add("n_covers_mask", lay(b"ACGNNnnnNNACG", 60))
    add("iupac", lay(b"ACGTRYKMSWBDHVNacgtrykmswbdhvn-*.ACGTU", 60))
    add("only_n", lay(b"N" * 130, 60))
    add("only_n_tiles", lay(b"N" * (TILE + 100), 60))
    add("all_lower", lay(b"acgt" * 40, 50, b"\r\n"))
    add("all_lower_n", lay(b"n" * 70, 50))
    add("last_byte_shared", lay(b"ACGTA" * 13, 7) + lay(b"G", 1))
    return cases


def batch_bodies(count=3000):
    """`count` short records of 20..400 characters, every eighth one without a byte (no tile), every ninth of line ends only."""
    rng = np.random.default_rng(tc.SEED + 41)
    bodies = []
    for i in range(count):
        if i % 8 == 5:
            bodies.append(b"")
        elif i % 9 == 4:
            bodies.append(b"\n")
        else:
            bodies.append(lay(_mixed(rng, int(rng.integers(20, 401))), (50, 60, 61)[i % 3], (b"\n", b"\r\n")[i % 2], i % 5 != 0))
    return bodies


def place(bodies, aligned: bool):
    """(buffer, offsets, lengths): the bodies in one buffer with header-like filler between them -- each body at a multiple of 16
    (`aligned`), or with fillers of growing length so that the bodies start at every address mod 16."""
    buf, off, ln = bytearray(b">first\n"), [], []
    for i, body in enumerate(bodies):
        if aligned:
            buf += b">" * ((-len(buf)) % 16)
        off.append(len(buf))
        ln.append(len(body))
        buf += body + b">" + b"x" * (i % 17) + b"\n"
    return bytes(buf), np.array(off, np.int64), np.array(ln, np.int64)


def masked_texts():
    """{label: text}: small masked texts as --mask_dir writes them, for the host packer and the file writer."""
    rng = np.random.default_rng(tc.SEED + 42)
    cases = body_cases()
    texts = {
        "every_case": b"".join(b">c%d %s\n" % (i, label.encode()) + body + (b"" if body.endswith(b"\n") or not body else b"\n")
                               for i, (label, body) in enumerate(cases) if label != "lineends_only"),   # (blank lines end the loop)
        "no_records": b"",
        "text_before_the_first_header": b"ACGT\nacgt\n>real one\nACGTNNacgt\n",
        "empty_header_is_no_record": b">a\nACGT\n>\nGGGG\n>b\tx\nnnnn\n",
        "names_are_first_words": b">  chr1  homo sapiens \nACGT\n>chr2|x y\nAC\n",
        "crlf": b">r1\r\nACGTnn\r\nNNac\r\n>r2\r\n",
        "lone_cr": b">r1\rACGTnn\rNNac\r>r2\rGG",
        "no_final_line_end": b">r1\nACGTacgtN",
    }
    texts["mixed"] = b"".join(b">m%d\n" % i + lay(_mixed(rng, int(n)), 60) for i, n in enumerate(rng.integers(0, 300, 40)))
    return texts
