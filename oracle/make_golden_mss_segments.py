#!/usr/bin/env python3
"""Generate tests/golden/mss_segments.npz from the REFERENCE ITSELF (build container only): the reference's own
mss.c (``make -C oracle ref`` -> oracle/_ref/libdeepgrp_ref_c.so) run on the score folds of ``folds()``, stored as
data -- per fold and (min score, xdrop) pair, the number of segments it found and the SHA-256 of their bytes
(``segments_digest``: start, end as int32, score as float64, little-endian).  Nothing of the reference's source
text is stored.

The folds are not stored: ``folds()`` makes them from splitmix64 with integer arithmetic and IEEE additions only,
so every host and numpy version computes the same bits; their digests are stored too, so a drift in the inputs
shows as such.

Usage:  make -C oracle ref && python oracle/make_golden_mss_segments.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OUT = os.path.join(ROOT, "tests", "golden")
PARAMS = ((0.0, -1.0), (3.7, 2.5), (229.756, 2297.56), (1.0, 0.5))
SIZES = (0, 1, 5, 100, 3000, 50000)
TRIALS = 6


def _mix(z: np.ndarray) -> np.ndarray:
    """splitmix64's output function (uint64 arithmetic wraps)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _splitmix64(n: int, seed: int) -> np.ndarray:
    """n outputs of splitmix64 started at a state derived from `seed` (streams of different seeds do not overlap)."""
    g = np.uint64(0x9E3779B97F4A7C15)
    start = _mix(np.array([seed + 1], np.uint64) * g)
    return _mix(np.arange(1, n + 1, dtype=np.uint64) * g + start)


def folds():
    """(n, trial, scores): 6 folds per size -- even trials integers in [-5, 3], odd trials near-Gaussian with mean -0.2
    and standard deviation 2 (sum of 12 uniforms, Irwin-Hall), as float64."""
    out = []
    for i, n in enumerate(SIZES):
        for trial in range(TRIALS):
            seed = (i * TRIALS + trial) * 16
            if trial % 2:
                acc = np.zeros(n, np.float64)
                for j in range(12):
                    acc = acc + (_splitmix64(n, seed + j) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
                S = (acc - 6.0) * 2.0 - 0.2
            else:
                S = (_splitmix64(n, seed) % np.uint64(9)).astype(np.int64).astype(np.float64) - 5.0
            out.append((n, trial, S))
    return out


def segments_digest(segs) -> np.ndarray:
    """SHA-256 (32 uint8) of a list of (start, end, score) segments."""
    st = np.array([s[0] for s in segs], "<i4")
    en = np.array([s[1] for s in segs], "<i4")
    sc = np.array([s[2] for s in segs], "<f8")
    return np.frombuffer(hashlib.sha256(st.tobytes() + en.tobytes() + sc.tobytes()).digest(), np.uint8).copy()


def fold_digest(S: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(S, "<f8").tobytes()).digest(), np.uint8).copy()


def main():
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    if orc.ref_c() is None:
        sys.exit("oracle/_ref/libdeepgrp_ref_c.so is missing: make -C oracle ref")
    fs = folds()
    nseg = np.zeros((len(fs), len(PARAMS)), np.int64)
    sha = np.zeros((len(fs), len(PARAMS), 32), np.uint8)
    for k, (_n, _trial, S) in enumerate(fs):
        for p, (msc, xd) in enumerate(PARAMS):
            segs = orc.mss_find_all(S, msc, xd, use_ref=True)
            nseg[k, p] = len(segs)
            sha[k, p] = segments_digest(segs)
    out = {"params": np.array(PARAMS, np.float64), "folds": np.stack([fold_digest(S) for _n, _t, S in fs]),
           "nseg": nseg, "sha": sha}
    np.savez_compressed(os.path.join(OUT, "mss_segments.npz"), **out)


if __name__ == "__main__":
    main()
