"""The corpus of tests/test_gpu_summary.py and tests/test_summary_host.py (a plain helper, no tests here): record bodies of one
buffer and their rows, built so that every case dgrp_repeat_summary_batch can meet occurs -- and checked here that it does.

Bodies: LF and CRLF line ends, ragged line widths, no final line end; body sizes of 0, 1, 15, 16, 17, 4095, 4096, 4097 and
3 * 4096 + 5 bytes; a body that starts at every offset 0..15 inside its 16-byte word; all 256 byte values except CR and LF; upper
case, lower case and N / n / IUPAC letters.  Rows (per class count C): a record without rows, a row at position 0 and one that ends
at the last position, two touching rows with different labels, a row over a tile edge, a one-base row, labels up to C - 1."""
import random

import numpy as np

TILE = 4096
SIZES = (0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)
ALPHABETS = (b"ACGT", b"ACGTacgt", b"ACGTacgtNnRYKMSWBDHVrykmswbdhv", b"acgtn")
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
NO_ROWS = 5                                    # index of a record with bytes and no rows


def body(rng: random.Random, nbytes: int, crlf: bool, alphabet: bytes) -> bytes:
    """Exactly `nbytes` bytes of lines of ragged widths (1..90); the cut may fall inside a line: then there is no final line end."""
    nl = b"\r\n" if crlf else b"\n"
    out = bytearray()
    while len(out) < nbytes:
        out += bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 91))) + nl
    return bytes(out[:nbytes])


def every_byte_body(rng: random.Random) -> bytes:
    """All 254 byte values that are neither CR nor LF, three times over, in lines of 50 with LF."""
    vals = [v for v in range(256) if v not in (10, 13)] * 3
    rng.shuffle(vals)
    return b"\n".join(bytes(vals[i:i + 50]) for i in range(0, len(vals), 50))


def positions(buf: bytes, off: int, ln: int) -> np.ndarray:
    """The offsets in `buf` of the sequence bytes of the body [off, off + ln): every byte that is neither CR nor LF."""
    a = np.frombuffer(buf, np.uint8)[off:off + ln]
    return np.flatnonzero((a != 10) & (a != 13)).astype(np.int64) + off


def random_rows(rng: random.Random, n: int, C: int, longest: int):
    """Ascending, disjoint rows over n positions: the first starts at 0, the last ends at n, some touch, some have one base."""
    rows, p, first = [], 0, True
    while p < n:
        p += 0 if first or rng.random() < 0.3 else rng.randrange(1, 40)
        first = False
        if p >= n:
            break
        e = min(p + (1 if rng.random() < 0.2 else rng.randrange(1, longest)), n)
        lab = rng.randrange(0, C)
        if rows and rows[-1][1] == p and rows[-1][2] == lab:
            lab = (lab + 1) % C                        # touching rows get different labels
        rows.append((p, e, lab))
        p = e
    if rows and rows[-1][1] < n:
        rows.append((n - 1, n, C - 1))
    return rows


def corpus(C: int, seed: int = 11):
    """-> (buffer, offsets, lengths, rows per record as [(start, end, label)]) for a model of C classes."""
    rng = random.Random(seed * 100 + C)
    specs = [(n, k % 2 == 1, ALPHABETS[k % len(ALPHABETS)], None) for k, n in enumerate(SIZES)]
    specs += [(rng.randrange(100, 400), k % 3 == 0, ALPHABETS[k % len(ALPHABETS)], k) for k in range(16)]     # start offset k mod 16
    specs.append((None, False, None, None))
    buf, offs, lens = bytearray(b"xx\n"), [], []
    for n, crlf, alphabet, align in specs:
        text = every_byte_body(rng) if n is None else body(rng, n, crlf, alphabet)
        buf += b"x" * rng.randrange(1, 40)
        if align is not None:
            buf += b"x" * ((align - len(buf)) % 16)
        offs.append(len(buf))
        lens.append(len(text))
        buf += text
    buf += b"\nxx"
    buf = bytes(buf)
    rowsets = []
    for k, (off, ln) in enumerate(zip(offs, lens)):
        n = int(positions(buf, off, ln).size)
        if n == 0 or k == NO_ROWS:
            rowsets.append([])
        elif n < 4:
            rowsets.append([(0, n, C - 1)])
        else:
            rowsets.append(random_rows(rng, n, C, 3000 if ln > 2 * TILE else 60))
    # ---- the corpus holds what its docstring says
    assert sorted(lens[:len(SIZES)]) == sorted(SIZES) and lens.count(0) == 1
    assert {o % 16 for o in offs} == set(range(16))
    seen = set()
    for off, ln in zip(offs, lens):
        seen |= set(buf[off:off + ln])
    assert seen | {10, 13} == set(range(256))
    assert any(b"\r\n" in buf[o:o + n] for o, n in zip(offs, lens)) and any(n and b"\r" not in buf[o:o + n] for o, n in zip(offs, lens))
    assert any(n > 1 and buf[o + n - 1] not in (10, 13) for o, n in zip(offs, lens))
    flat = [r for rows in rowsets for r in rows]
    assert rowsets[NO_ROWS] == [] and lens[NO_ROWS] > 0
    assert any(r[1] - r[0] == 1 for r in flat) and max(r[2] for r in flat) == C - 1
    assert any(a[1] == b[0] and a[2] != b[2] for rows in rowsets for a, b in zip(rows, rows[1:]))
    big = lens.index(3 * TILE + 5)
    pos = positions(buf, offs[big], lens[big])
    word0 = offs[big] & ~15
    assert any((pos[s] - word0) // TILE != (pos[e - 1] - word0) // TILE for s, e, _l in rowsets[big])       # a row over a tile edge
    for k, rows in enumerate(rowsets):
        if rows:
            assert rows[0][0] == 0 and rows[-1][1] == positions(buf, offs[k], lens[k]).size
    return buf, np.array(offs, np.int64), np.array(lens, np.int64), rowsets


WALK_GRID = 2048                               # SUMMARY_GRID of summary_kernels.hip: a workgroup walks ceil(tiles / 2048) tiles


def tiles_of(off: int, ln: int) -> int:
    """body_tiles_of of body_tiles.h: the 4096-byte tiles of a body, counted from the 16-byte word it starts in."""
    return (off + ln - (off & ~15) + TILE - 1) // TILE if ln > 0 else 0


def many_tiles(C: int, seed: int = 23):
    """The walk as a chromosome meets it, at the smallest size that does: more than 2 * 2048 tiles, so that a workgroup walks
    several consecutive tiles.  About 4500 records of a few dozen bytes (one tile each: every workgroup changes record inside its
    range, flushes and counts on in the zeroed counters), a record without bytes now and then, and two records of five and nine
    tiles that begin in one workgroup's range and end in another's.  -> as corpus()."""
    rng = random.Random(seed * 100 + C)
    buf, offs, lens = bytearray(b"x\n"), [], []
    for k in range(4500):
        if k in (1000, 3001):                                          # the long records, at odd tile indices
            n = (5 if k == 1000 else 9) * TILE - rng.randrange(1, 2000)
        elif k % 97 == 5:
            n = 0
        else:
            n = rng.randrange(1, 70)
        text = body(rng, n, k % 2 == 1, ALPHABETS[k % len(ALPHABETS)])
        buf += b"x" * rng.randrange(0, 5)
        offs.append(len(buf))
        lens.append(len(text))
        buf += text
    buf = bytes(buf + b"\nxx")
    rowsets = []
    for k, (off, ln) in enumerate(zip(offs, lens)):
        n = int(positions(buf, off, ln).size)
        if n == 0 or k % 11 == 3:
            rowsets.append([])
        elif n < 4:
            rowsets.append([(0, n, C - 1)])
        else:
            rowsets.append(random_rows(rng, n, C, 3000 if ln > TILE else 30))
    # ---- it holds what its docstring says
    tile0 = np.zeros(len(offs) + 1, np.int64)
    np.cumsum([tiles_of(o, n) for o, n in zip(offs, lens)], out=tile0[1:])
    ntiles = int(tile0[-1])
    per = (ntiles + WALK_GRID - 1) // WALK_GRID
    assert ntiles > 2 * WALK_GRID and per >= 2 and len(buf) < 400_000
    assert ntiles % per != 0                                           # the last workgroup ends on a partial range
    for k in (1000, 3001):
        first, last = int(tile0[k]), int(tile0[k + 1]) - 1
        assert last - first >= 4 and first // per != last // per      # one record over two workgroups
        assert first % per != 0                                       # and it begins inside a range, behind other records
        assert len(rowsets[k]) > 5
    assert lens.count(0) > 20
    return buf, np.array(offs, np.int64), np.array(lens, np.int64), rowsets


def seg_array(rowsets):
    """-> (rows as SEG, contig = record; row offsets [nrec + 1])"""
    rows = np.array([(s, e, lab, k) for k, rs in enumerate(rowsets) for s, e, lab in rs], SEG)
    off = np.zeros(len(rowsets) + 1, np.int64)
    np.cumsum([len(r) for r in rowsets], out=off[1:])
    return rows, off


def reserved_bins(lens: np.ndarray, bin: int) -> np.ndarray:
    """The bin offsets the host reserves without knowing the sequence lengths: ceil(body bytes / bin) per record."""
    off = np.zeros(len(lens) + 1, np.int64)
    if bin:
        np.cumsum((lens + bin - 1) // bin, out=off[1:])
    return off
