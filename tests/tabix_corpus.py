"""Shared by the tabix index tests: class columns, bedGraph texts, the brute-force overlap filter, query regions, and a restatement
in Python of what dgrp_track_index_batch hands out (chunks and linear index per record, in text offsets), from the text alone."""
import numpy as np

BLOCK = 0xff00


def noisy(n, seed, step=7):
    """A class column that changes its second decimal every few bases and is 0 in stretches (lines, runs and gaps)."""
    rng = np.random.default_rng(seed)
    v = np.repeat(rng.integers(0, 60, size=n // step + 1), step)[:n].astype(np.float32) / np.float32(100)
    v[rng.integers(0, 4, size=n // step + 1).repeat(step)[:n] == 0] = 0
    return v


def parse(text):
    """[(line, name, start, end)] of a bedGraph text."""
    out = []
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        out.append((line, f[0], int(f[1]), int(f[2])))
    return out


def brute(lines, name, beg, end):
    return [l for l, nm, s, e in lines if nm == name and s < end and e > beg]


def regions(lines, seed, count=200):
    """`count` seeded random regions and the regions at the edges of every 16 kb window the text reaches."""
    rng = np.random.default_rng(seed)
    names = list(dict.fromkeys(nm for _l, nm, _s, _e in lines))
    top = max(e for _l, _nm, _s, e in lines)
    out = []
    for _ in range(count):
        beg = int(rng.integers(0, top + 20_000))
        out.append((names[int(rng.integers(0, len(names)))], beg, beg + int(rng.choice([1, 10, 500, 20_000, 200_000]))))
    for nm in names:
        for w in range(1, (top >> 14) + 2):
            e = w << 14
            out += [(nm, e - 1, e), (nm, e, e + 1), (nm, e - 1, e + 1)]
    return out


def device_like(rec_texts):
    """What the device entry gives for one class of a write whose records have the texts `rec_texts` (b"" for a record without a
    line): (chunks as [(beg, end, rec, bin)], linear as one list per record up to its last line, text) -- the rule of the header."""
    from deepgrp_amd.tabix import reg2bin
    chunks, linear, u = [], [], 0
    for r, t in enumerate(rec_texts):
        lin, prev = [], None
        for line, _nm, s, e in parse(t):
            b = reg2bin(s, e)
            if prev == b:
                chunks[-1][1] = u + len(line) + 1
            else:
                chunks.append([u, u + len(line) + 1, r, b])
            prev = b
            lin += [u] * (((e - 1) >> 14) + 1 - len(lin))
            u += len(line) + 1
        linear.append(lin)
    return chunks, linear, b"".join(rec_texts)
