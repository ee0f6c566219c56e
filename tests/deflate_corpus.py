"""Inputs of the BGZF encoder's tests (test_deflate_host.py, test_gpu_deflate.py) and the checks both run on an output."""
import ctypes as C
import gzip
import zlib

import numpy as np

BLOCK = 0xff00
EINVAL, ENOMEM = -1, -3


def _fasta(seq: bytes, name: bytes = b"chr1 synthetic", width: int = 60) -> bytes:
    return b">" + name + b"\n" + b"\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + b"\n"


def synthetic_texts(n_bases: int = 2_000_000):
    """The 60-column FASTA of synthetic_chromosome(n_bases) as it is, with its planted repeats in lower case, and with them as N."""
    from deepgrp_amd import synthetic
    idx, lab = synthetic.synthetic_truth(n_bases)
    seq = np.frombuffer(b"ACGTN", np.uint8)[idx]
    soft = np.where(lab > 0, seq | 0x20, seq).astype(np.uint8)
    hard = np.where(lab > 0, np.uint8(78), seq).astype(np.uint8)
    return {"unmasked": _fasta(seq.tobytes()), "soft": _fasta(soft.tobytes()), "hard": _fasta(hard.tobytes())}


def records_10k(nrec: int = 400) -> bytes:
    """`nrec` soft-masked records of 10 kbp under long header lines: rare bytes beside the few frequent ones (the 15-bit limit)."""
    from deepgrp_amd import synthetic
    idx, lab = synthetic.synthetic_truth(nrec * 10_000, contig=2, flank=0)
    seq = np.frombuffer(b"ACGTN", np.uint8)[idx]
    soft = np.where(lab > 0, seq | 0x20, seq).astype(np.uint8).tobytes()
    out = []
    for k in range(nrec):
        name = b"scaffold_%05d|len=10000|Assembly: GRCx-%d.p%d (synthetic) [taxon=%d] {Quality~%d%%} #%x" % (k, k % 7, k % 13, 9606 + k,
                                                                                                          90 + k % 10, k * 2654435761)
        out.append(_fasta(soft[k * 10_000:(k + 1) * 10_000], name))
    return b"".join(out)


def fibonacci_text() -> bytes:
    """Byte counts 2, 3, 5, 8, ... as far as one member holds them: with end-of-block's 1 in front, every merge of the unlimited
    Huffman code takes the tree built so far, so it is as deep as it has symbols."""
    fib = [2, 3]
    while sum(fib) + fib[-1] + fib[-2] <= BLOCK:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(6)
    data = np.concatenate([np.full(f, 40 + i, np.uint8) for i, f in enumerate(fib)])
    return rng.permutation(data).tobytes()


def corpus():
    rng = np.random.default_rng(17)
    acgt = rng.choice(list(b"ACGTacgtN\n"), size=BLOCK + 1, p=[.2, .2, .2, .2, .04, .04, .04, .04, .02, .02]).astype(np.uint8).tobytes()
    out = {"empty": b"", "one_byte": b"G", "one_symbol": b"N" * 300_000, "two_symbols": b"AB" * 40_000 + b"A" * 77,
           "all_bytes": bytes(range(256)) * 5, "random": rng.integers(0, 256, size=200_000, dtype=np.uint8).tobytes(),
           "records_10k": records_10k(), "fibonacci": fibonacci_text(),
           "len_block_minus_1": acgt[:BLOCK - 1], "len_block": acgt[:BLOCK], "len_block_plus_1": acgt}
    out.update(synthetic_texts())
    return out


SIZE_BOUND = ("unmasked", "soft", "hard", "records_10k")           # at most 1.03 x zlib's Z_HUFFMAN_ONLY


def compress_host(data: bytes, eof: bool = True) -> bytes:
    from deepgrp_amd._lib import lib
    L = lib()
    cap = L.dgrp_bgzf_bound(len(data), int(eof))
    out = (C.c_uint8 * max(cap, 1))()
    got = C.c_int64(-1)
    rc = L.dgrp_bgzf_compress_host(data, len(data), out, cap, C.byref(got), int(eof))
    assert rc == 0, L.dgrp_last_error()
    assert 0 <= got.value <= cap
    return bytes(memoryview(out)[:got.value])


def check_file(out: bytes, data: bytes, eof: bool) -> None:
    """`out` is a BGZF file of `data` as the encoder promises it."""
    from deepgrp_amd import gz
    from deepgrp_amd._lib import lib
    L = lib()
    assert len(out) <= L.dgrp_bgzf_bound(len(data), int(eof))
    if out or eof:
        assert gzip.decompress(out) == data
    else:
        assert data == b""
    m = gz.walk_members(out)
    assert m.kind == "bgzf"
    isize = m.isize.tolist()
    if eof:
        assert out.endswith(gz.BGZF_EOF) and isize[-1] == 0
        isize = isize[:-1]
    nmem = (len(data) + BLOCK - 1) // BLOCK
    assert len(isize) == nmem and sum(isize) == len(data)
    assert all(v == BLOCK for v in isize[:-1]) and (not isize or 0 < isize[-1] <= BLOCK)
    ends = m.start.tolist()[1:] + [len(out)]
    pos = 0
    for k in range(nmem):
        piece = data[pos:pos + isize[k]]
        pos += isize[k]
        assert ends[k] - int(m.start[k]) <= len(piece) + 31
        raw = out[int(m.data_off[k]):int(m.data_off[k] + m.data_len[k])]
        d = zlib.decompressobj(-15)
        assert d.decompress(raw) == piece and d.eof and d.unused_data == b""        # the stream ends exactly at the trailer
        buf = (C.c_uint8 * len(piece))()
        ol, iu, r = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
        assert L.dgrp_inflate_raw_host(raw, len(raw), buf, len(piece), C.byref(ol), C.byref(iu), C.byref(r)) == 0
        assert (ol.value, iu.value, r.value) == (len(piece), len(raw), 0) and bytes(buf) == piece
