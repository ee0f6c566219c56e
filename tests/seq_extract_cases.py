"""An independent statement of `predict --seq_dir` (the FASTA of the predicted repeats) for tests/test_seq_extract_host.py and
tests/test_gpu_seq_extract.py, in Python integers and slices only: the byte-position walk over a FASTA text, the text of the rows
and its `.fai`, and the spec lists both test files use.  No torch, no numpy in the statement itself.

For a row (start, end, label) of a record with `n` sequence positions: A = start - min(flank, start), B = end + min(flank, n - end);
    >NAME:A-B class<label>LF                      (flank == 0)
    >NAME:A-B class<label> core=<start>-<end>LF   (flank > 0)
then the bytes of the positions [A, B), `width` per line, every line LF-terminated.  NAME = the first word of the header."""
import random

WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"
TILE = 4096


def brute_records(data: bytes):
    """[(name, [byte positions of its sequence characters] or None if a sequence line is not ASCII)] in file order: lines end at
    LF, CRLF or a lone CR, every line is stripped, a '>' line opens a record, a record without a header is dropped."""
    recs, cur, pos = [], None, 0
    while pos < len(data):
        e = pos
        while e < len(data) and data[e] not in (10, 13):
            e += 1
        term = 2 if data[e:e + 2] == b"\r\n" else (1 if e < len(data) else 0)
        line, s0 = data[pos:e], pos
        pos = e + term
        a, b = 0, len(line)
        while a < b and line[a] in WS:
            a += 1
        while b > a and line[b - 1] in WS:
            b -= 1
        if a == b:
            raise IndexError("blank line")
        if line[a] == 62:
            cur = None
            header = line[a + 1:b]
            if header:
                words = header.split()
                cur = [words[0] if words else b"", []]
                recs.append(cur)
        elif cur is not None and cur[1] is not None:
            if not line.isascii():
                cur[1] = None
            else:
                cur[1] += list(range(s0 + a, s0 + b))
    return [(n, p) for n, p in recs]


def sequences(data: bytes):
    """[(name, the record's sequence bytes or None)] of brute_records."""
    return [(n, None if p is None else bytes(data[i] for i in p)) for n, p in brute_records(data)]


def row_text(name: bytes, seq: bytes, start: int, end: int, label: int, flank: int, width: int) -> bytes:
    a = start - min(flank, start)
    b = end + min(flank, len(seq) - end)
    head = b">" + name + (":%d-%d class%d" % (a, b, label)).encode()
    if flank > 0:
        head += (" core=%d-%d" % (start, end)).encode()
    part = seq[a:b]
    if width == 1:
        body = b"".join(bytes([c, 10]) for c in part)
    else:
        body = b"".join(part[i:i + width] + b"\n" for i in range(0, len(part), width))
    return head + b"\n" + body


def brute_extract(data: bytes, rows_per_record, flank: int = 0, width: int = 60, classes=None, seqs=None) -> bytes:
    """rows_per_record[k] = [(start, end, label), ...] of the k-th record brute_records finds (`seqs`: sequences(data), when the
    caller already has them).  Rows outside `classes` (None: every label > 0) are left out."""
    out = []
    for k, (name, seq) in enumerate(sequences(data) if seqs is None else seqs):
        if seq is None or k >= len(rows_per_record):
            continue
        for start, end, label in sorted(rows_per_record[k]):
            if (label in classes) if classes is not None else label > 0:
                assert 0 <= start < end <= len(seq)
                out.append(row_text(name, seq, start, end, label, flank, width))
    return b"".join(out)


def fasta_records(text: bytes):
    """The records of a FASTA text as written here: [(offset of '>', header line without '>' and LF, offset of the first base,
    bases, length of the first sequence line)]."""
    out, pos = [], 0
    while pos < len(text):
        assert text[pos] == 62, pos
        lf = text.index(b"\n", pos)
        header, base0 = text[pos + 1:lf], lf + 1
        p, bases, first = base0, 0, None
        while p < len(text) and text[p] != 62:
            e = text.index(b"\n", p)
            first = e - p if first is None else first
            bases += e - p
            p = e + 1
        out.append((pos, header, base0, bases, first or 0))
        pos = p
    return out


def brute_fai(text: bytes) -> bytes:
    """The index `samtools faidx` writes for `text`: name (the header's first word), bases, offset of the first base, bases per
    line, bytes per line."""
    lines = []
    for _at, header, base0, bases, first in fasta_records(text):
        lines.append(header.split()[0] + ("\t%d\t%d\t%d\t%d\n" % (bases, base0, first, first + 1)).encode())
    return b"".join(lines)


def brute_entries(text: bytes):
    """[(text_off, base_off, bases)] of the records of `text`: what dgrp_extract_entry states."""
    return [(at, base0, bases) for at, _h, base0, bases, _f in fasta_records(text)]


# ---------------------------------------------------------------- the spec lists
ALPHABET = b"ACGTNacgtnRYKMswbdhv*-"
FLANKS = (0, 1, 5000)
WIDTHS = (1, 7, 60, 100_000)
CLASSES = (1, 3)
# (sequence length, line width, CRLF): the fixed bodies of the kernel test, then forty random small ones
FIXED_BODIES = [(1, 60, False), (5, 1, False), (200, 60, True), (4097, 61, False), (70_000, 70_000, False), (150_000, 66_000, True),
                (9000, 1, True), (0, 60, False), (777, 60, False)]
DENSE, LONG, EMPTY, NO_ROWS = 6, 5, 7, 8         # indices into FIXED_BODIES with rows of their own


def body_specs(seed: int = 5):
    rng = random.Random(seed)
    return FIXED_BODIES + [(rng.randrange(1, 5000), rng.randrange(1, 100), bool(rng.randrange(2))) for _ in range(40)]


def body(rng: random.Random, n: int, width: int, crlf: bool, final_nl: bool = True) -> bytes:
    seq = bytes(rng.choice(ALPHABET) for _ in range(n))
    nl = b"\r\n" if crlf else b"\n"
    return nl.join(seq[i:i + width] for i in range(0, n, width)) + (nl if final_nl and n else b"")


def random_rows(rng: random.Random, n: int, gap: int = 400, longest: int = 300):
    rows, p = [], 0
    while p < n:
        p += rng.randrange(0, gap)
        if p >= n:
            break
        ln = rng.randrange(1, longest)
        rows.append((p, min(p + ln, n), rng.randrange(0, 5)))
        p = min(p + ln, n)
    return rows


def kernel_case(seed: int = 5):
    """(buffer, [body offset], [body length], [name], [rows]) of the kernel test: every body behind 0..16 pad bytes, every third
    without its last line end.  Rows: the whole body (body 1), the first and the last base with a row outside CLASSES between kept
    ones (body 2), more than 256 one-base rows inside one 4096-byte tile of the source (DENSE), one row over more than 20 tiles
    (LONG), none (EMPTY, NO_ROWS), random ones elsewhere."""
    rng = random.Random(seed)
    buf, offs, lens, names, rowsets = bytearray(b"\n"), [], [], [], []
    for k, (n, w, crlf) in enumerate(body_specs(seed)):
        buf += b"x" * rng.randrange(0, 17)
        text = body(rng, n, w, crlf, final_nl=k % 3 != 1)
        offs.append(len(buf))
        lens.append(len(text))
        names.append(b"h%d" % k if k != 3 else b"")
        buf += text + b"\n"
        if k == 0:
            rows = [(0, 1, 1)]
        elif k == 1:
            rows = [(0, n, 3)]
        elif k == 2:
            rows = [(0, 1, 1), (50, 60, 2), (60, 61, 4), (100, 120, 3), (n - 1, n, 1)]
        elif k == DENSE:
            # body bytes are 3 per base (one base, CR, LF): the bases of the source tile that starts at or behind the body's start
            tile1 = (offs[k] & ~15) + TILE
            p0 = (tile1 - offs[k] + 2) // 3 + 1
            rows = [(p0 + 4 * j, p0 + 4 * j + 1, 1 if j % 10 else 2) for j in range(300)]
            assert tile1 <= offs[k] + 3 * rows[0][0] and offs[k] + 3 * rows[-1][0] < tile1 + TILE
            assert sum(1 for r in rows if r[2] in CLASSES) > 256
        elif k == LONG:
            rows = [(3, 20, 1), (1000, 140_000, 3), (140_000, 140_001, 1), (149_999, 150_000, 1)]
        elif k in (EMPTY, NO_ROWS):
            rows = []
        else:
            rows = random_rows(rng, n)
            if n > 2 and rng.random() < 0.5:
                rows = [(0, 1, 1)] + [r for r in rows if r[0] >= 2]
        rowsets.append(rows)
    return bytes(buf), offs, lens, names, rowsets


def odd_records_file() -> bytes:
    """Records the device path does not take (and two it does): lone CR, CRLF, lines padded with blanks and tabs, text before the
    first header, a record with an empty name, a record with a non-ASCII line, a last line without a line end."""
    rng = random.Random(9)
    parts = [b"text before the first header\nmore of it\n"]
    parts.append(b">plain one\n" + body(rng, 5000, 60, False))
    parts.append(b">crlf two\r\n" + body(rng, 3000, 70, True))
    parts.append(b">padded\n" + b"\n".join(b"  " + body(rng, 50, 50, False, False) + b" \t" for _ in range(30)) + b"\n")
    parts.append(b">\n" + body(rng, 300, 60, False))                  # no header: dropped
    parts.append(b">  \tsecond word only\n" + body(rng, 90, 60, False))
    parts.append(b">nonascii\nACGT\xc3\xa9ACGT\nACGT\n")
    parts.append(b">lone cr\rACGTACGTNN\rACgt\n")
    parts.append(b">empty\n")
    parts.append(b">last\n" + body(rng, 20_000, 80, False, False))
    return b"".join(parts)


def headerless_chunk() -> bytes:
    return b"ACGT\nACGT\n"


def rows_for(data: bytes, seed: int = 2):
    """Random rows for every record of `data` (a record that is not ASCII gets rows as well: they must be ignored)."""
    rng = random.Random(seed)
    per = []
    for _name, pos in brute_records(data):
        n = len(pos) if pos is not None else 10
        rows = random_rows(rng, n, gap=200, longest=150)
        if n > 3:
            rows = [(0, 1, 1)] + [r for r in rows if r[0] >= 2 and r[1] <= n - 2] + [(n - 1, n, 3)]
        per.append(rows)
    return per
