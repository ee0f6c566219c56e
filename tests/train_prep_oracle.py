"""The numpy statement of what `train` prepares on the device for a sequence file: the multi-hot truth of a side, the
class index sets, the map from a uniform rank to a start, and the resolution of (set, rank) picks.  Written from the definitions,
not from the kernels and not from _calc_indices; tests/test_train_prep_host.py pins it to the reference's host functions for one
record, tests/test_gpu_train_prep.py holds the device entries to it byte for byte.

A side: records r = 0.. back to back in a buffer of n_total bases, record r at [off[r], off[r] + length[r]), its first base at the
original coordinate origin[r]; rows[r] = (start, end, label) triples in original coordinates."""
import numpy as np


def truth(classes, n_total, off, length, origin, rows):
    """int8 [classes, n_total]: truth[label, b:e] = 1 for every row clipped to its record, truth[0] = 1 where no row covers."""
    y = np.zeros((classes, n_total), np.int8)
    for r, (o, n, g) in enumerate(zip(off, length, origin)):
        for start, end, label in rows[r]:
            a, e = min(max(start - g, 0), n), min(max(end - g, 0), n)
            if e > a:
                y[label, o + a:o + e] = 1
    y[0] = (y[1:].sum(axis=0) == 0)
    return y


def class_starts(row, off, length, T):
    """int64 ascending buffer positions off[r] + s of the members of every record: 1 <= s <= length[r] - 1 - T with a non-zero byte
    of the record's row in [s + 1, s + T]."""
    out = []
    for o, n in zip(off, length):
        rec = np.asarray(row[o:o + n]) != 0
        last = n - 1 - T
        if last < 1:
            continue
        ones = np.concatenate(([0], np.cumsum(rec, dtype=np.int64)))           # ones[i] = ones among rec[:i]
        s = np.arange(1, last + 1, dtype=np.int64)
        out.append(o + s[ones[s + T + 1] - ones[s + 1] > 0])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def window_prefix(length, T):
    """Exclusive prefix sums [nrec + 1] of W_r = max(length[r] - T, 0)."""
    w = np.maximum(np.asarray(length, np.int64) - T, 0)
    return np.concatenate(([0], np.cumsum(w))).astype(np.int64)


def uniform_start(k, off, length, T):
    """Rank k of [0, W) -> the start: record r with prefix[r] <= k < prefix[r + 1], start off[r] + k - prefix[r]."""
    prefix = window_prefix(length, T)
    r = int(np.searchsorted(prefix, k, side="right")) - 1
    assert 0 <= r < len(length) and prefix[r] <= k < prefix[r + 1]
    return int(off[r]) + int(k - prefix[r])


def resolve(picks, sets, off, length, T):
    """Starts of (set, rank) picks: an element of sets[set], or the uniform start for any other set or an empty one; ranks clamped;
    0 where there is no window at all."""
    W = int(window_prefix(length, T)[-1])
    out = np.zeros(len(picks), np.int64)
    for i, (k, rank) in enumerate(np.asarray(picks, np.int64).tolist()):
        rank = max(rank, 0)
        if 0 <= k < len(sets) and len(sets[k]):
            out[i] = sets[k][min(rank, len(sets[k]) - 1)]
        elif W > 0:
            out[i] = uniform_start(min(rank, W - 1), off, length, T)
    return out
