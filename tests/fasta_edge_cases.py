"""The deterministic corpus of the FASTA ingest kernels (deepgrp_amd/csrc/fasta_kernels.hip) and the statement they are held to (a
plain helper, no tests here; test_fasta_edge_cases_host.py holds the corpus to the reference's line loop, test_gpu_fasta_edges.py
holds the kernels to the corpus).  Plain Python and numpy: nothing here calls the library.

Every case is a record BODY -- the bytes between a header line and the next header -- with the plain flag it must get, written by
hand.  The bodies put what the kernels look at on the boundaries the kernels have: the 2048-byte tile whose last bytes look ahead
into the next tile, the lane / wave / workgroup / tile steps of the N stripping, the 1 MiB switch between the one-workgroup kernel
and the count / scan / scatter chain of the batch entry, and the 64 MiB sweep of the chunk finder's capped grid."""
import functools
from collections import namedtuple

import numpy as np

TILE = 2048                       # scan.h: `#define SCAN_TILE 2048`
SMALL = 1 << 20                   # fasta_kernels.hip, dgrp_fasta_encode_batch: `const int64_t SMALL_BYTES = 1 << 20;`
VEC = 16                          # fasta_kernels.hip, fasta_gt_kernel: `const int64_t nvec = n / 16;` (one uint4 per lane)
GT_SWEEP = 16384 * 256 * 16       # fasta_kernels.hip, dgrp_fasta_chunks: the grid is capped at 16384u workgroups of 256 lanes

ALPHABET = b"ACGTNacgtnRYKM"
LINE = 62                         # a line feed every 62 bytes: no multiple of a tile, so a kept index is never its byte offset
EDGES = (TILE, 2 * TILE)
EDGE_BODY = 2 * TILE + 700

# body: the bytes; plain: the flag by hand; blank: the body has an empty line (the reference's loop raises IndexError on it);
# feature / at: the name of the planted feature and the offset of its first byte (None / -1 where the case has none)
Case = namedtuple("Case", "name body plain blank feature at")

# name -> (bytes, plain flag).  Plain: deleting CR and LF equals stripping every line, and no line is empty.
FEATURES = {
    "lf": (b"\n", 1),
    "crlf": (b"\r\n", 1),
    "bang": (b"!", 1),                       # 33: the first byte above the whitespace range
    "del": (b"\x7f", 1),                     # 127: the last ASCII byte; str.strip leaves it
    "gt": (b">", 1),                         # inside a line it opens nothing
    "lone_cr": (b"\rA", 0),                  # a line break in text mode; the kernels do not judge which, they hand the record back
    "lf_lf": (b"\n\n", 0),
    "lf_crlf": (b"\n\r\n", 0),
    "crlf_crlf": (b"\r\n\r\n", 0),
    "space": (b" ", 0),
    "tab": (b"\t", 0),
    "vt": (b"\x0b", 0),
    "us": (b"\x1f", 0),
    "nul": (b"\x00", 0),
    "x80": (b"\x80", 0),
    "xff": (b"\xff", 0),
}
BLANK_FEATURES = ("lf_lf", "lf_crlf", "crlf_crlf")

_CLASS = np.full(256, 4, np.uint8)
for _k, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _CLASS[list(_pair)] = _k


def reference(body: bytes):
    """(plain, total, startpos, kept, idx) of a record body as include/deepgrp_hip.h states dgrp_fasta_encode: `plain` is the
    package's host statement of the rule (fasta._plain), `total` the bytes that are neither CR nor LF, `startpos` / `kept` the
    leading N count and the length between the N flanks of those bytes after upper() -- (total, -total) for an all-N body, (0, 0)
    for an empty one --, `idx` the class of every one of the `total` bytes (A,a=0 C,c=1 G,g=2 T,t=3 else 4)."""
    from deepgrp_amd import fasta
    body = bytes(body)
    seq = body.translate(None, b"\r\n")
    up = seq.upper()
    total = len(up)
    startpos = total - len(up.lstrip(b"N"))
    kept = -total if startpos == total else len(up.strip(b"N"))
    idx = _CLASS[np.frombuffer(seq, np.uint8)] if total else np.zeros(0, np.uint8)
    return int(bool(fasta._plain(body))), total, startpos, kept, idx


def letters(rng, n: int) -> bytearray:
    return bytearray(rng.choice(np.frombuffer(ALPHABET, np.uint8), size=n).tobytes())


def _lined(rng, n: int, lo: int, hi: int) -> bytearray:
    """n letters with a line feed at every byte 61, 123, ... that lies in [lo, hi)."""
    out = letters(rng, n)
    for p in range(LINE - 1, n, LINE):
        if lo <= p < hi:
            out[p] = 10
    return out


def _planted(rng, n: int, feature: bytes, at: int) -> bytes:
    """A body of n bytes with `feature` at offset `at`: regular lines in front of it, the last line feed at least three bytes away
    (the feature is the only thing that decides the flag: no planted byte completes a pair with a regular line end, and a '>' never
    opens a line); letters only behind it."""
    out = _lined(rng, n, 1, at - 2)
    out[at:at + len(feature)] = feature
    assert len(out) == n
    return bytes(out)


def edge_bodies(name: str):
    """The feature at every offset from `edge - len - 1` to `edge + 1`, for both tile edges of a body of 2 * TILE + 700 bytes:
    wholly in front of the edge (twice: one byte of cover, then none), split at every byte, wholly behind (twice)."""
    feat, plain = FEATURES[name]
    rng = np.random.default_rng(1000 + sorted(FEATURES).index(name))
    out = []
    for edge in EDGES:
        for at in range(edge - len(feat) - 1, edge + 2):
            out.append(Case(f"{name}@{at}", _planted(rng, EDGE_BODY, feat, at), plain, name in BLANK_FEATURES, name, at))
    return out


def end_bodies():
    """The first and the last bytes of a body (where the look-ahead has nothing to read, and where a line break has nothing in
    front of it), and the lengths around one and two tiles."""
    rng = np.random.default_rng(77)
    out = []
    for tag, tail, plain, blank in (("cr", b"\r", 0, False), ("crlf", b"\r\n", 1, False), ("lf", b"\n", 1, False), ("none", b"", 1, False),
                                    ("lflf", b"\n\n", 0, True)):
        out.append(Case(f"ends_{tag}", _planted(rng, TILE, tail, TILE - len(tail)), plain, blank, None, -1))
    for tag, head in (("lf", b"\n"), ("crlf", b"\r\n"), ("cr", b"\r")):
        body = bytearray(_lined(rng, TILE + 5, 5, TILE))
        body[:len(head)] = head
        out.append(Case(f"opens_{tag}", bytes(body), 0, True, None, -1))
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        out.append(Case(f"len{n}", bytes(_lined(rng, n, 1, n)), 1, False, None, -1))
    return out


N_TOTAL = 3 * TILE + 300
# kept indices that get the only base: the first and last byte of a lane's eight (7 | 8), of a wave's 512 (511 | 512; 63 | 64 are
# lane 7 | 8), of a tile (2047 | 2048) and of the body, and one inside
N_PLANTS = (0, 7, 8, 63, 64, 255, 511, 512, 1535, 1536, 2047, 2048)


def _n_body(rng, total: int, crlf: bool, plants: dict) -> bytes:
    """`total` sequence bytes, N or n at random except plants (kept index -> letter); one line, or CRLF lines of 60."""
    seq = bytearray(rng.choice(np.frombuffer(b"Nn", np.uint8), size=total).tobytes())
    for k, c in plants.items():
        seq[k] = c
    if not crlf:
        return bytes(seq)
    return b"\r\n".join(bytes(seq[i:i + 60]) for i in range(0, total, 60)) + b"\r\n"


def n_bodies():
    """All-N bodies of more than three tiles with one base, two bases or none: the N flanks come out of a reduction over lanes,
    waves, the workgroup and the tiles, and every step of it gets the only base on either side of its edge.  The base is 'R' as
    often as a letter of ACGT: class 4 like N, and no N."""
    rng = np.random.default_rng(5)
    out = []
    for crlf in (False, True):
        tag = "crlf" if crlf else "oneline"
        for j, k in enumerate(N_PLANTS + (N_TOTAL - 1,)):
            out.append(Case(f"n_{tag}_one@{k}", _n_body(rng, N_TOTAL, crlf, {k: b"AcRg"[j % 4]}), 1, False, None, -1))
        out.append(Case(f"n_{tag}_two", _n_body(rng, N_TOTAL, crlf, {1000: ord("r"), N_TOTAL - 100: ord("T")}), 1, False, None, -1))
        out.append(Case(f"n_{tag}_two_edges", _n_body(rng, N_TOTAL, crlf, {TILE - 1: ord("t"), 3 * TILE: ord("K")}), 1, False, None, -1))
        out.append(Case(f"n_{tag}_none", _n_body(rng, N_TOTAL, crlf, {}), 1, False, None, -1))
    out.append(Case("n_single_N", b"N", 1, False, None, -1))
    out.append(Case("n_single_n", b"n", 1, False, None, -1))
    out.append(Case("n_single_A", b"A", 1, False, None, -1))
    return out


def matrix():
    """Every case of the small corpus (a record of a few tiles), in a fixed order."""
    out = []
    for name in FEATURES:
        out += edge_bodies(name)
    return out + end_bodies() + n_bodies()


def position(case: Case, edge: int) -> str:
    """Where the case's feature lies about the tile edge: 'before' (its last byte in front of the edge), 'straddle' (bytes on both
    sides) or 'behind'."""
    n = len(FEATURES[case.feature][0])
    return "before" if case.at + n <= edge else "behind" if case.at >= edge else "straddle"


def boundary_profile(corpus):
    """How the planted features of `corpus` (Cases) meet the tile edges: {feature: {edge: [before, straddle, behind, flush, ahead]}}.
    The first three count the cases by position() at the edge nearest the feature; `flush` counts those whose last byte is the
    last byte of a tile or whose first byte is the first of one (a feature of one byte cannot straddle: that pair is its whole
    meeting with the edge); `ahead` counts those in which a CR or LF in front of the edge has its look-ahead (one byte behind a CR,
    two behind an LF) reach across it -- the reads that leave the tile."""
    out = {}
    for case in corpus:
        if case.feature is None:
            continue
        feat = FEATURES[case.feature][0]
        edge = min(EDGES, key=lambda e: abs(case.at - e))
        row = out.setdefault(case.feature, {e: [0, 0, 0, 0, 0] for e in EDGES})[edge]
        row[("before", "straddle", "behind").index(position(case, edge))] += 1
        row[3] += case.at + len(feat) == edge or case.at == edge
        row[4] += any(c in b"\r\n" and case.at + j < edge <= case.at + j + (2 if c == 10 else 1) for j, c in enumerate(feat))
    return out


# ------------------------------------------------------------------------------------------------------------------ path switch
Batch = namedtuple("Batch", "text off len bodies plain names")


def _tiled(rng, n: int, eol: bytes, width: int = 60) -> bytearray:
    """n bytes of lines: a few KB of random lines, repeated."""
    unit = b"".join(bytes(letters(rng, width)) + eol for _ in range(67))
    return bytearray((unit * (n // len(unit) + 1))[:n])


def _batch(bodies, plain) -> Batch:
    text, off, names = bytearray(), [], []
    for r, body in enumerate(bodies):
        names.append("r%d%s" % (r, "x" * (r % 3)))                         # header lines of 4, 5, 6 ... bytes: odd and even offsets
        text += b">" + names[-1].encode() + b"\n"
        off.append(len(text))
        text += body
        if body and body[-1] != 10:
            text += b"\n"                                                   # (the line end of a body's last line is not the body's)
    return Batch(bytes(text), np.array(off, np.int64), np.array([len(b) for b in bodies], np.int64), bodies, list(plain), names)


@functools.lru_cache(maxsize=None)
def mixed_batch() -> Batch:
    """Eleven records of one buffer for one dgrp_fasta_encode_batch: empty, one byte, the three sizes about the 1 MiB switch (the same
    bytes, then one and two letters appended: the last one-workgroup record, and large records of 513 tiles), 1.5 MiB (768 tiles:
    the carry loop of scan_sums_kernel ends on a full round), empty, a large body spoiled by one space in its last tile, a large
    CRLF body, 5 000 bytes, empty.  The large records share the tile area of the workspace, each at its running offset."""
    rng = np.random.default_rng(2024)
    base = b"NNnNn" + bytes(_tiled(rng, SMALL - 1 - 5, b"\n"))
    spoiled = _tiled(rng, SMALL + 3 * TILE + 77, b"\n")
    at = len(spoiled) - 40
    spoiled[at - 3:at + 4] = b"ACG TAC"
    crlf = bytes(_tiled(rng, SMALL + 5 * TILE + 1, b"\r\n")[:-8]) + b"ACnN\r\nnN"
    bodies = [b"", b"c", base, base + b"A", base + b"AN", bytes(_tiled(rng, 3 * SMALL // 2, b"\n", 70)), b"", bytes(spoiled), crlf,
              bytes(_tiled(rng, 5000, b"\n", 50)), b""]
    return _batch(bodies, [1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1])


def empty_batch() -> Batch:
    return _batch([b"", b"", b""], [1, 1, 1])


def ntiles(nbytes: int) -> int:
    return (nbytes + TILE - 1) // TILE


# ------------------------------------------------------------------------------------------------------------------ chunk seam
SEAM_BYTES = GT_SWEEP + 4 * VEC + 5
SEAM_SHIFTS = (-1, 0, 1)


def seam_text(shift: int) -> np.ndarray:
    """GT_SWEEP + 4 * VEC + 5 bytes of 'A' for dgrp_fasta_chunks: a grid of 16 384 workgroups takes the first GT_SWEEP bytes in its
    first sweep, four more vectors in its second, and one lane takes the five bytes of the scalar tail.  A "\\n>" puts its '>' at
    GT_SWEEP + shift (shift -1: the last byte of the first sweep; 0: the first byte of the second, its line feed in the other
    sweep; +1) -- the three cannot share one text, so there are three texts.  In each: "\\n>" across three vector edges of the first
    sweep (the second also a workgroup's edge), a '>' as the last byte of the tail behind a line feed, a "\\n>" inside the second
    sweep, and '>' that follow no line feed (one of them the first byte of a vector).  Every planted header line but the last has its
    line feed two bytes on."""
    d = np.full(SEAM_BYTES, ord("A"), np.uint8)

    def header(gt: int, lf: bool = True):
        d[gt - 1], d[gt] = 10, ord(">")
        if lf:
            d[gt + 3] = 10

    for gt in (5 * VEC, 7 * 256 * VEC, 100_003 * VEC, GT_SWEEP + shift, GT_SWEEP + 2 * VEC + 7):
        header(gt)
    header(SEAM_BYTES - 1, lf=False)
    for gt in (1000, 9 * VEC, GT_SWEEP - 3 * VEC, GT_SWEEP + VEC):
        assert d[gt - 1] != 10
        d[gt] = ord(">")
    return d


def seam_answer(d: np.ndarray):
    """(chunk starts, first line feed of every chunk or the size) by the definition, in numpy."""
    starts = np.concatenate([[0], np.flatnonzero((d[:-1] == 10) & (d[1:] == 62)) + 1]).astype(np.int64)
    lf_pos = np.flatnonzero(d == 10)
    k = np.searchsorted(lf_pos, starts)
    first = np.where(k < lf_pos.size, lf_pos[np.minimum(k, lf_pos.size - 1)], d.size)
    stop = np.concatenate([starts[1:], [d.size]])
    return starts, np.where(first < stop, first, d.size).astype(np.int64)


def seam_region(start: int) -> str:
    """Which part of fasta_gt_kernel's walk finds a chunk start of a seam text."""
    tail0 = SEAM_BYTES // VEC * VEC
    return "tail" if start >= tail0 else "second" if start >= GT_SWEEP else "first"
