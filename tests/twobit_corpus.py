"""Shared by the 2bit tests: an independent writer of the format (struct.pack, either byte order, the block lists written as they are
given -- unmerged, adjacent, overlapping, zero-length -- and any two bits under N blocks and behind the last base), a restatement in
Python of the text of a file and of the class indices of a record, and the corpus: the smallest shapes at which the parser or the
kernels can go wrong.  Nothing here comes from deepgrp_amd/twobit.py."""
import struct
from collections import namedtuple

import numpy as np

SIGNATURE = 0x1A412743
SEED = 20260207
SPAN = 16384                                    # bases of one workgroup of the kernels as built
SIZES = [0, 1, 2, 3, 4, 5, 15, 16, 17, 49, 50, 51, 63, 64, 65, 100, 4095, 4096, 4097, 70001]

# name, two-bit values (T=0 C=1 A=2 G=3) of every base, N blocks and mask blocks as written [(start, size)], bits behind the last base
Rec = namedtuple("Rec", "name codes nblocks mblocks pad")


def pack_dna(codes, pad):
    n = len(codes)
    full = np.concatenate([np.asarray(codes, np.uint8), np.asarray(pad, np.uint8)[:(-n) % 4]])
    q = full.reshape(-1, 4)
    return ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8).tobytes()


def write(records, order="<", version=0):
    """The bytes of a 2bit file of `records`."""
    u = lambda *v: struct.pack(order + "%dI" % len(v), *v)
    blobs = []
    for r in records:
        b = u(len(r.codes))
        for blocks in (r.nblocks, r.mblocks):
            b += u(len(blocks)) + u(*[s for s, _z in blocks]) + u(*[z for _s, z in blocks])
        blobs.append(b + u(0) + pack_dna(r.codes, r.pad))
    pos = 16 + sum(1 + len(r.name) + 4 for r in records)
    index = b""
    for r, b in zip(records, blobs):
        index += bytes([len(r.name)]) + r.name + u(pos)
        pos += len(b)
    return u(SIGNATURE, version, len(records), 0) + index + b"".join(blobs)


def _paint(n, blocks):
    inside = np.zeros(n, bool)
    for s, z in blocks:
        inside[s:s + z] = True
    return inside


def intervals(n, blocks):
    """The disjoint ascending [start, end) intervals the blocks cover, from the painted bases."""
    edge = np.diff(np.concatenate(([0], _paint(n, blocks).astype(np.int8), [0])))
    return np.stack((np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)), axis=1).astype(np.int64)


def indices(r):
    """Class index per base: A=0 C=1 G=2 T=3, N=4 inside an N block whatever the two bits say."""
    idx = np.array([3, 1, 0, 2], np.uint8)[np.asarray(r.codes, np.uint8)]
    idx[_paint(len(idx), r.nblocks)] = 4
    return idx


def strip_n(idx):
    """(startpos, kept) as the FASTA ingest reports them: kept = -length for a record of N only."""
    keep = np.flatnonzero(idx != 4)
    if keep.size == 0:
        return len(idx), -len(idx)
    return int(keep[0]), int(keep[-1]) + 1 - int(keep[0])


def letters(r):
    b = np.frombuffer(b"TCAG", np.uint8)[np.asarray(r.codes, np.uint8)].copy()
    b[_paint(len(b), r.nblocks)] = ord("N")
    b[_paint(len(b), r.mblocks)] |= 0x20
    return b.tobytes()


def text(records):
    """The text of the file: '>' name LF, the bases 50 per line, every line LF-terminated."""
    out = []
    for r in records:
        seq = letters(r)
        out.append(b">" + r.name + b"\n" + b"".join(seq[o:o + 50] + b"\n" for o in range(0, len(seq), 50)))
    return b"".join(out)


def block_kinds(n, rng):
    """{kind: [(start, size)]} for a record of n >= 64 bases (the span kinds need n > SPAN + 1000)."""
    kinds = {
        "none": [],
        "whole": [(0, n)],
        "leading": [(0, 7)],
        "trailing": [(n - 9, 9)],
        "single": [(8, 1), (13, 1), (22, 1), (31, 1)],          # p mod 4 = 0, 1, 2, 3
        "adjacent": [(5, 6), (11, 9)],
        "overlapping": [(5, 20), (12, 30)],
        "nested": [(5, 40), (12, 3), (50, 2)],
        "zero": [(3, 0), (20, 4), (30, 0)],
        "cross16": [(10, 30)],
        "ends": [(0, 3), (n - 2, 2)],
    }
    if n > SPAN + 1000:
        kinds["crossspan"] = [(SPAN - 300, 1000)]
        first = np.sort(rng.choice(n // 2, 5000, replace=False)) * 2            # 5 000 one-base blocks, never adjacent
        kinds["many"] = [(int(s), 1) for s in first]
    return kinds


def _rec(rng, name, n, nblocks=(), mblocks=()):
    return Rec(name, rng.integers(0, 4, n).astype(np.uint8), list(nblocks), list(mblocks), rng.integers(0, 4, 3).astype(np.uint8))


def _name(i, length):
    return (b"r%d_" % i + b"x" * 17)[:length]


def sizes_file(rng=None):
    """One record per dnaSize of SIZES, name lengths 0..17 in turn; blocks where the record has room for them."""
    rng = rng or np.random.default_rng(SEED)
    recs = []
    for i, n in enumerate(SIZES):
        nb = mb = ()
        if n >= 64:
            kinds = block_kinds(n, rng)
            keys = [k for k in kinds if k not in ("whole", "many")]
            nb, mb = kinds[keys[i % len(keys)]], kinds[keys[(i + 3) % len(keys)]]
        elif n >= 3:
            nb, mb = [(n - 1, 1)][:i % 2], [(0, 2)][:(i // 2) % 2]
        recs.append(_rec(rng, _name(i, i % 18), n, nb, mb))
    return recs


def blocks_file(rng=None):
    """Every kind of N block, each with a mask kind of its own (one of them covers the N block), on short records and on records of
    more than two workgroup spans."""
    rng = rng or np.random.default_rng(SEED + 1)
    recs = []
    for n in (300, 2 * SPAN + 5001):
        kinds = block_kinds(n, rng)
        keys = list(kinds)
        for i, k in enumerate(keys):
            recs.append(_rec(rng, b"%s_%d" % (k.encode(), n), n, kinds[k], kinds[keys[(i + 4) % len(keys)]]))
        recs.append(_rec(rng, b"covered_%d" % n, n, [(40, 10)], [(30, 30)]))
    return recs


def batch_file(count=3000, rng=None):
    """`count` records of 20..400 bases: the batch path."""
    rng = rng or np.random.default_rng(SEED + 2)
    recs = []
    for i in range(count):
        n = int(rng.integers(20, 401))
        nb = mb = ()
        if i % 3 == 0:
            s = int(rng.integers(0, n - 4))
            nb = [(s, int(rng.integers(1, min(12, n - s))))]
        if i % 5 == 0:
            nb = [(0, int(rng.integers(1, 5)))] + list(nb if nb and nb[0][0] >= 5 else ())
        if i % 4 == 0:
            s = int(rng.integers(0, n - 4))
            mb = [(s, int(rng.integers(1, n - s)))]
        recs.append(_rec(rng, b"s%d" % i, n, nb, mb))
    return recs


def cli_file():
    """What `predict` is run on: every size, every kind of block (the long records only where the kind needs one), the odd records;
    no record of N only, which ends the command."""
    long_kinds = (b"crossspan", b"many")
    recs = sizes_file() + [r for r in blocks_file() if len(r.codes) == 300 or r.name.startswith(long_kinds)] + odd_file()
    return [r for r in recs if strip_n(indices(r))[1] >= 0]


def odd_file(rng=None):
    """Records the ingest treats specially: an empty name (dropped), a record of N only (the reference's ValueError), no base at all,
    leading and trailing N, a name with blanks around it."""
    rng = rng or np.random.default_rng(SEED + 3)
    return [_rec(rng, b"first", 120, [(0, 11)], [(5, 20)]), _rec(rng, b"", 90, [(10, 5)]), _rec(rng, b"allN", 77, [(0, 40), (40, 37)]),
            _rec(rng, b"nothing", 0), _rec(rng, b" padded ", 130, [(0, 4), (120, 10)], [(100, 30)]), _rec(rng, b"last", 61, [(60, 1)])]
