"""Inputs of the level-1 BGZF encoder's tests (test_deflate_lz_host.py, test_gpu_deflate_lz.py) beside deflate_corpus.corpus(): the
texts the match finder is for (bedGraph tracks, N runs) and the edges of its rule (window, length cap, member ends)."""
import ctypes as C

import numpy as np

from deflate_corpus import BLOCK, corpus

BEDGRAPH = ("bedgraph_d2_bin1", "bedgraph_d2_bin50", "bedgraph_d3_bin1_long_name", "bedgraph_d3_bin50_long_name")


def random_walk(n: int, seed: int) -> np.ndarray:
    """float32 [n] in [0, 1]: a reflected random walk with flat stretches at 0 (left out of a track) and at 1."""
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.normal(0, 0.02, n))
    return np.clip(np.abs((w + 0.5) % 3 - 1.5) - 0.25, 0, 1).astype(np.float32)


def bedgraph_texts():
    from deepgrp_amd import tracks
    return {"bedgraph_d2_bin1": tracks.reference_text(random_walk(60_000, 1), 1000, b"chr1", 2, 1),
            "bedgraph_d2_bin50": tracks.reference_text(random_walk(3_000_000, 2), 1000, b"chr1", 2, 50),
            "bedgraph_d3_bin1_long_name": tracks.reference_text(random_walk(60_000, 3), 123_456_789, b"NC_000001.11", 3, 1),
            "bedgraph_d3_bin50_long_name": tracks.reference_text(random_walk(3_000_000, 4), 123_456_789, b"NC_000001.11", 3, 50)}


def edge_texts():
    rng = np.random.default_rng(29)
    rnd = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    out = {"n_run": b"N" * 300_000}
    # a member of 64 byte values drawn at random (6 bits a byte under any code, and 4-byte repeats by chance are few): one stretch of
    # 2000 bytes returns 32 768 back (the farthest a distance reaches), another 32 769 back
    few = lambda n: rng.integers(48, 112, size=n, dtype=np.uint8).tobytes()
    m = bytearray(few(BLOCK))
    m[3000 + 32768:5000 + 32768] = m[3000:5000]
    m[300 + 32769:2300 + 32769] = m[300:2300]
    out["window_edge"] = bytes(m)
    p258, p259, p600 = rnd(258), rnd(259), rnd(600)
    out["length_cap"] = rnd(50) + p258 + rnd(50) + p258 + rnd(50) + p259 + rnd(50) + p259 + rnd(50) + p600 + rnd(7) + p600
    m = bytearray(few(BLOCK))
    m[BLOCK - 2000:] = m[BLOCK - 22000:BLOCK - 20000]
    out["match_ends_the_member"] = bytes(m) + few(500)
    m = few(BLOCK)
    out["source_in_previous_member"] = m + m[-2000:] + few(400) + m[:200]
    out["periods"] = b"".join(rnd(30) + pat * k for pat, k in ((b"x", 700), (b"xy", 500), (b"xyz", 400), (b"N", 3), (b"ab", 2), (b"q", 259),
                                                               (b"r", 260), (b"s", 5)))
    for k in range(1, 5):
        out[f"bytes_{k}"] = b"ACGT"[:k]
        out[f"same_bytes_{k}"] = b"N" * k
    pat = rnd(40)
    out["one_distance"] = rnd(500) + pat + rnd(300) + pat + rnd(200)
    out["one_distance_run"] = b"N" * 1000
    return out


def all_texts():
    out = dict(corpus())
    out.update(bedgraph_texts())
    out.update(edge_texts())
    return out


def compress_host_level(data: bytes, eof: bool = True, level: int = 1) -> bytes:
    from deepgrp_amd._lib import lib
    L = lib()
    cap = L.dgrp_bgzf_bound(len(data), int(eof))
    out = (C.c_uint8 * max(cap, 1))()
    got = C.c_int64(-1)
    rc = L.dgrp_bgzf_compress_host_level(data, len(data), out, cap, C.byref(got), int(eof), level)
    assert rc == 0, L.dgrp_last_error()
    assert 0 <= got.value <= cap
    return bytes(memoryview(out)[:got.value])


def member_sizes(out: bytes):
    from deepgrp_amd import gz
    m = gz.walk_members(out)
    return np.diff(np.r_[m.start, len(out)])
