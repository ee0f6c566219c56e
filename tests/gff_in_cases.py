"""The corpus of the GFF3 reader (a plain helper, no tests here): texts as bytes with what the grammar of dgrp_gff_parse
(include/deepgrp_hip.h) makes of them, written down by hand or known from the way the text was put together -- never taken from a
parser.  A case is Case(text, names, key, want): want is ROWS = (lines in front of E, E, [(line, seqid bytes, begin, end, number)]),
UNDECIDED, or ("malformed", line)."""
from typing import List, NamedTuple, Optional

import numpy as np

CHUNK, TILE = 128, 32768
UNDECIDED = "undecided"
NAMES4 = [[b"LTR", b"ERV1", b"ERVK"], [b"LINE", b"L1"], [b"Alu"], [b"Satellite", b"a/b", b"100%", b"x;y"]]
DEFAULT4 = [[b"class1"], [b"class2"], [b"class3"], [b"class4"]]
KEY = b"Name"


class Case(NamedTuple):
    text: bytes
    names: List[List[bytes]]
    key: Optional[bytes]
    want: object


def feature(seqid=b"chr1", start=11, end=20, attrs=b"ID=r1;Name=Alu", typ=b"repeat_region", source=b"deepgrp", tail=b"0.9\t.\t."):
    """One feature line without its line end."""
    return b"\t".join([seqid, source, typ, b"%d" % start if isinstance(start, int) else start, b"%d" % end if isinstance(end, int) else end,
                       tail, attrs])


FILL = feature() + b"\n"                  # chr1 10 20, Alu = 3 under NAMES4
FILL_ROW = (b"chr1", 10, 20, 3)


def pad(text: bytes, target: int) -> bytes:
    """`text` grown to exactly `target` bytes with whole FILL lines and one comment or empty line; -> (text, FILL lines added)."""
    assert target >= len(text)
    k = (target - len(text)) // len(FILL)
    text += FILL * k
    r = target - len(text)
    return text + (b"" if r == 0 else b"\n" if r == 1 else b"#" + b"x" * (r - 2) + b"\n"), k


def _rows_of(text: bytes, feature_rows):
    """ROWS of a text whose feature lines are known: feature_rows = [(offset of the line, seqid, begin, end, number)]."""
    return [(text[:o].count(b"\n") + 1, s, b, e, n) for o, s, b, e, n in feature_rows]


def _lines(text: bytes) -> int:
    return text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)


def sized(n: int) -> Case:
    """A file of exactly n bytes: FILL lines, then one comment."""
    text, k = pad(b"", n)
    rows = [(i * len(FILL),) + FILL_ROW for i in range(k)]
    return Case(text, NAMES4, KEY, (_lines(text), n, _rows_of(text, rows)))


def whole(text: bytes, rows, names=NAMES4, key=KEY) -> Case:
    """A text without an end of features: rows = [(line, seqid, begin, end, number)] written by hand."""
    return Case(text, names, key, (_lines(text), len(text), rows))


def _one(attrs, number, names=NAMES4, key=KEY, typ=b"repeat_region"):
    text = b"##gff-version 3\n" + feature(attrs=attrs, typ=typ) + b"\n"
    return Case(text, names, key, (2, len(text), [(2, b"chr1", 10, 20, number)]))


def _behind(prefix_len: int, what=b"##FASTA\n") -> Case:
    """`what` starting exactly at offset prefix_len, feature-shaped lines behind it in the same chunk, a later chunk and a later tile."""
    text, k = pad(b"##gff-version 3\n", prefix_len)
    rows = [(16 + i * len(FILL),) + FILL_ROW for i in range(k)]
    lines = _lines(text)
    tail = what + FILL + b"ACGT" * 40 + b"\n" + FILL + (b"ACGTACGTAC" * 6 + b"\n") * 600 + FILL
    assert len(tail) > TILE + 1000
    return Case(text + tail, NAMES4, KEY, (lines, prefix_len, _rows_of(text, rows)))


def straddles() -> Case:
    """A seqid, a coordinate and an attribute value across a chunk edge and across a tile edge: each placed by hand."""
    text, rows = b"##gff-version 3\n", []
    seqid, value = b"scaffold_000123", b"Satellite"
    line = feature(seqid=seqid, start=123456789, end=123456999, attrs=b"ID=x;Name=" + value + b";note=long")
    at_seqid, at_start, at_value = 5, line.index(b"123456789") + 4, line.index(value) + 4
    edges = [3 * CHUNK, 7 * CHUNK, 11 * CHUNK, TILE, 2 * TILE, 3 * TILE]
    for edge, inside in zip(edges, [at_seqid, at_start, at_value] * 2):
        before = len(text)
        text, k = pad(text, edge - inside)
        rows += [(before + i * len(FILL),) + FILL_ROW for i in range(k)]
        rows.append((len(text), seqid, 123456788, 123456999, 4))
        text += line + b"\n"
        assert len(text) > edge
    return Case(text, NAMES4, KEY, (_lines(text), len(text), _rows_of(text, rows)))


def bulk(seed: int = 0, count: int = 4000) -> Case:
    """`count` generated lines over three records (one of them in two spellings), with CRLF ends, comments and empty lines among them,
    labels by every alternative, escaped and not; the last line has no line feed."""
    rng = np.random.default_rng(seed)
    seqids = [b"chr1", b"chr2", b"chr%7C3", b"chr|3"]
    labels = [(b"LTR", 1), (b"ERVK", 1), (b"L1", 2), (b"Alu", 3), (b"%41lu", 3), (b"a%2Fb", 4), (b"a%2fb", 4), (b"100%25", 4), (b"100%", 4),
              (b"x%3By", 4), (b"Unknown", 0), (b"Al", 0), (b"Alus", 0), (b"", 0)]
    parts, rows, at, line_no = [b"##gff-version 3\n"], [], 16, 1
    rec = 0
    for i in range(count):
        if rng.random() < 0.002:
            rec = (rec + 1) % len(seqids)
        kind = rng.random()
        eol = b"\r\n" if rng.random() < 0.1 else b"\n"
        if i == count - 1:
            kind, eol = 1.0, b""
        if kind < 0.03:
            ln = [b"", b"###", b"# a comment", b"##sequence-region chr1 1 1000"][int(rng.integers(0, 4))]
        else:
            label, number = labels[int(rng.integers(0, len(labels)))]
            start = int(rng.integers(1, 10 ** int(rng.integers(1, 18))))
            end = start + int(rng.integers(0, 5000))
            where = int(rng.integers(0, 4))
            attrs = [b"Name=%s;ID=r%d" % (label, i), b"ID=r%d;Name=%s;score=5" % (i, label), b"ID=r%d;Names=no;Name=%s" % (i, label),
                     b"ID=r%d" % i][where]
            if where == 3:
                number = 0
            ln = feature(seqids[rec], start, end, attrs)
            rows.append((line_no + 1, seqids[rec], start - 1, end, number))
        parts.append(ln + eol)
        at += len(ln) + len(eol)
        line_no += 1
    text = b"".join(parts)
    return Case(text, NAMES4, KEY, (line_no, len(text), rows))


def many_names(count: int = 4096):
    """A table of `count` alternatives under 4 labels, among them proper prefixes of each other."""
    names = [[], [], [], []]
    for k in range(count):
        names[k % 4].append(b"fam%d" % k)
    return names


def cases():
    c = {}
    for n in (0, 1, 127, 128, 129, TILE - 1, TILE, TILE + 1):
        c[f"size {n}"] = sized(n)
    c["directives"] = whole(b"##gff-version 3\n###\n##sequence-region chr1 1 500\n# a comment\n\n" + FILL + b"###\n", [(6,) + FILL_ROW])
    c["CRLF"] = whole(b"##gff-version 3\r\n" + feature() + b"\r\n\r\n" + feature(seqid=b"chr2") + b"\r\n",
                      [(2,) + FILL_ROW, (4, b"chr2", 10, 20, 3)])
    c["last line without LF"] = whole(FILL + feature(seqid=b"chr2"), [(1,) + FILL_ROW, (2, b"chr2", 10, 20, 3)])
    c["nine fields exactly"] = whole(b"c\ts\tt\t1\t2\t.\t.\t.\t\n", [(1, b"c", 0, 2, 0)])
    c["shortest line"] = whole(b"\t\t\t1\t2\t\t\t\t\n\t\t\t3\t4\t\t\t\t", [(1, b"", 0, 2, 0), (2, b"", 2, 4, 0)])
    c["tenth tab"] = _one(b"ID=1;note=a\tb;Name=L1\tx", 0)
    c["tenth tab, value before it"] = _one(b"Name=L1;note=a\tb", 2)
    c["eight fields"] = Case(FILL + b"# c\n" + b"\t".join(feature().split(b"\t")[:8]) + b"\n" + FILL, NAMES4, KEY, ("malformed", 3))
    c["eight fields twice"] = Case(FILL * 3 + b"x\n" + FILL + b"chr1\t1\t2\n", NAMES4, KEY, ("malformed", 4))
    c["start 0"] = whole(feature(start=0, end=5) + b"\n", [(1, b"chr1", -1, 5, 3)])
    c["empty row"] = whole(feature(start=8, end=7) + b"\n", [(1, b"chr1", 7, 7, 3)])
    c["end below begin"] = whole(feature(start=8, end=6) + b"\n", [(1, b"chr1", 7, 6, 3)])
    d18 = b"9" * 18
    c["18 digits"] = whole(feature(start=d18, end=d18) + b"\n", [(1, b"chr1", 10 ** 18 - 2, 10 ** 18 - 1, 3)])
    c["19 digits"] = Case(FILL + feature(start=5, end=b"1" * 19) + b"\n", NAMES4, KEY, UNDECIDED)
    c["a sign"] = Case(FILL + feature(start=b"+5", end=9) + b"\n", NAMES4, KEY, UNDECIDED)
    c["an empty start"] = Case(FILL + feature(start=b"", end=9) + b"\n", NAMES4, KEY, UNDECIDED)
    c["a byte above 0x7e"] = Case(FILL + feature(attrs=b"Name=Al\xc3\xbc") + b"\n", NAMES4, KEY, UNDECIDED)
    c["a lone CR"] = Case(FILL + feature(attrs=b"Name=Alu\rx") + b"\n", NAMES4, KEY, UNDECIDED)
    c["key first"] = _one(b"Name=LINE;ID=r1;x=y", 2)
    c["key in the middle"] = _one(b"ID=r1;Name=ERV1;x=y", 1)
    c["key last"] = _one(b"ID=r1;x=y;Name=Satellite", 4)
    c["key last, trailing ;"] = _one(b"ID=r1;x=y;Name=Satellite;", 4)
    c["key absent"] = _one(b"ID=r1;x=y", 0)
    c["no attributes"] = _one(b"", 0)
    c["empty value"] = _one(b"ID=r1;Name=;x=y", 0)
    c["first piece wins"] = _one(b"Name=Alu;Name=L1", 3)
    c["Names= in front of Name="] = _one(b"Names=LTR;Name=L1", 2)
    c["a piece without ="] = _one(b"Name;Name=L1", 2)
    c["value with ="] = _one(b"Name=L1=x", 0)
    c["no trimming"] = _one(b"ID=1; Name=L1", 0)
    c["no comma split"] = _one(b"Name=L1,Alu", 0)
    c["%2F"] = _one(b"Name=a%2Fb", 4)
    c["%2f"] = _one(b"Name=a%2fb", 4)
    c["% as the last byte"] = _one(b"ID=1;Name=100%", 4)
    c["% as the last byte, not a name"] = _one(b"ID=1;Name=Alu%", 0)
    c["%4"] = _one(b"Name=%4", 0)
    c["%4 then piece end"] = _one(b"Name=Al%4;x=1", 0)
    c["%zz"] = _one(b"Name=%zzAlu", 0)
    c["%41lu"] = _one(b"Name=%41lu", 3)
    c["%3B inside a value"] = _one(b"Name=x%3By;z=1", 4)
    c["value a proper prefix"] = _one(b"Name=Satel", 0)
    c["alternative a proper prefix"] = _one(b"Name=Alus", 0)
    c["type mode"] = _one(b"Name=L1", 3, key=None, typ=b"Alu")
    c["type mode, escaped"] = _one(b"Name=L1", 4, key=None, typ=b"a%2Fb")
    c["type mode, no name"] = _one(b"Name=L1", 0, key=None)
    c["default names"] = _one(b"ID=r7;Name=class4;label=4;score=900", 4, names=DEFAULT4)
    c["another key"] = _one(b"ID=r7;Name=x;class=LINE", 2, key=b"class")
    c["0 alternatives"] = _one(b"Name=L1", 0, names=[])
    c["1 alternative"] = _one(b"Name=L1", 1, names=[[b"L1"]])
    big = many_names()
    c["4096 alternatives, first"] = _one(b"Name=fam0", 1, names=big)
    c["4096 alternatives, last"] = _one(b"Name=fam4095", 4, names=big)
    c["4096 alternatives, prefix"] = _one(b"Name=fam40", 1, names=big)
    c["4096 alternatives, none"] = _one(b"Name=fam4096", 0, names=big)
    two = feature(seqid=b"chr%7C3") + b"\n" + feature(seqid=b"chr|3") + b"\n" + feature(seqid=b"chr|3") + b"\n"
    c["escaped seqid"] = whole(two, [(1, b"chr%7C3", 10, 20, 3), (2, b"chr|3", 10, 20, 3), (3, b"chr|3", 10, 20, 3)])
    c["##FASTA at offset 0"] = Case(b"##FASTA\n>chr1\nACGT\n" + FILL, NAMES4, KEY, (0, 0, []))
    c["##FASTA as the only line"] = Case(b"##FASTA", NAMES4, KEY, (0, 0, []))
    c["##FASTA with CRLF"] = Case(FILL + b"##FASTA\r\n" + FILL, NAMES4, KEY, (1, len(FILL), [(1,) + FILL_ROW]))
    c["##FASTA as a last line without LF"] = Case(FILL + b"##FASTA", NAMES4, KEY, (1, len(FILL), [(1,) + FILL_ROW]))
    c["##FASTAX is a comment"] = whole(b"##FASTAX\n" + FILL + b"##FASTA x\n" + FILL, [(2,) + FILL_ROW, (4,) + FILL_ROW])
    c["a > line"] = Case(FILL + b">chr1 a record\n" + FILL + b"ACGT\n", NAMES4, KEY, (1, len(FILL), [(1,) + FILL_ROW]))
    c["junk behind E"] = Case(FILL + b"##FASTA\n>c\n\xff\xfe\rAC\tGT\n" + b"chr1\tx\n", NAMES4, KEY, (1, len(FILL), [(1,) + FILL_ROW]))
    c["##FASTA at a chunk edge"] = _behind(3 * CHUNK)
    c["##FASTA at a tile edge"] = _behind(TILE)
    c["> at the second tile edge"] = _behind(2 * TILE, b">chr1\n")
    c["##FASTA inside a chunk"] = _behind(5 * CHUNK + 77)
    c["straddles"] = straddles()
    c["bulk"] = bulk()
    return c


CASES = cases()


def gff_of_table(rows, names) -> bytes:
    """A GFF3 text of table rows [(contig, begin, end, number)]: the first alternative of the number's entry as Name."""
    out = [b"##gff-version 3\n"]
    for i, (contig, begin, end, number) in enumerate(rows):
        out.append(feature(contig.encode(), begin + 1, end, b"ID=t%d;Name=%s" % (i, names[number - 1][0])) + b"\n")
    return b"".join(out)
