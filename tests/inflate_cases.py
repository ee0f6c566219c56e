"""The corpus of raw DEFLATE streams the decode core is held to on the host (test_inflate_host.py), in the member kernel
(test_gpu_inflate_members.py) and in the span path (test_gpu_gzip_stream.py): a hand-written fixed-Huffman encoder for streams zlib
never emits, the corrupt corpus with the recorded results of its fixed-reason cases, and grids of valid members at the sizes where
the kernel's lane-split copies and per-lane CRC pieces change shape.  Expected text comes from zlib, never from the code under test."""
import functools
import struct
import zlib

import numpy as np

EINPUT, EBLOCK, ESTORED, ECODES, ESYMBOL, EDIST, EOUTPUT, ECRC, EISIZE, ETRAIL = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10


def deflate(data: bytes, level: int, strategy: int) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


# ---------------------------------------------------------------- a hand-written fixed-Huffman encoder (streams zlib never emits)
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v: int, k: int):                 # k bits of v, LSB first (header fields, extra bits)
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, c: int, k: int):                 # a Huffman code: MSB first
        self.put(int(format(c, f"0{k}b")[::-1], 2), k)

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b: Bits, sym: int):
    if sym < 144:
        b.code(0x30 + sym, 8)
    elif sym < 256:
        b.code(0x190 + sym - 144, 9)
    elif sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xC0 + sym - 280, 8)


def fixed_match(b: Bits, length: int, dist: int):
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
    dext = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
    i = max(k for k in range(29) if lbase[k] <= length and (k == 28) == (length == 258))
    fixed_lit(b, 257 + i)
    b.put(length - lbase[i], lext[i])
    d = max(k for k in range(30) if dbase[k] <= dist)
    b.code(d, 5)
    b.put(dist - dbase[d], dext[d])


def fixed_items(b: Bits, items):
    for it in items:
        if isinstance(it, tuple):
            fixed_match(b, *it)
        else:
            fixed_lit(b, it)


def fixed_stream(items, final=True) -> bytes:
    """items: ints (literals / raw symbols) or (length, distance) pairs; one fixed block ended by symbol 256."""
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    fixed_items(b, items)
    fixed_lit(b, 256)
    return b.bytes()


# ---------------------------------------------------------------- inputs
def _inputs():
    rng = np.random.default_rng(11)
    acgt = rng.choice(list(b"ACGT"), size=50_000).astype(np.uint8).tobytes()
    fasta = b">chr1 test\n" + b"\n".join(acgt[i:i + 60] for i in range(0, len(acgt), 60)) + b"\n"
    nrun = b"N" * 30_000 + acgt[:500] + b"N" * 20_000 + b"n" * 3
    rand = rng.integers(0, 256, size=40_000, dtype=np.uint8).tobytes()
    x = rng.integers(0, 256, size=300, dtype=np.uint8).tobytes()
    far = x + rng.integers(0, 256, size=32_768 - 300, dtype=np.uint8).tobytes() + x + x[:100] * 3
    return {"fasta": fasta, "nrun": nrun, "random": rand, "far": far, "empty": b"", "max": (acgt + acgt)[:65536]}


INPUTS = _inputs()
GOOD_TEXT = INPUTS["fasta"][:20_000]                                  # the member every corrupt case is cut or flipped from
GOOD = deflate(GOOD_TEXT, 6, zlib.Z_DEFAULT_STRATEGY)


def _dynamic_header(clen, hlit=0, hdist=0):
    """A dynamic block header: BFINAL=1, BTYPE=2, the code length code lengths `clen` in transmission order."""
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(hlit, 5)
    b.put(hdist, 5)
    b.put(len(clen) - 4, 4)
    for v in clen:
        b.put(v, 3)
    return b


def _corrupt_corpus():
    """(name, stream, output cap, expected reason or None = any failure)."""
    data, good = GOOD_TEXT, GOOD
    cases = []
    for k in (0, 1, 2, 5, len(good) // 2, len(good) - 1):
        cases.append((f"truncated_{k}", good[:k], len(data), EINPUT))
    cases.append(("block_type_3", bytes([0x07, 0, 0, 0]), 100, EBLOCK))
    cases.append(("stored_len_nlen", bytes([0x01, 5, 0, 0, 0]) + b"hello", 100, ESTORED))
    cases.append(("stored_truncated", bytes([0x01, 5, 0, 0xFA, 0xFF]) + b"hel", 100, EINPUT))
    cases.append(("stored_over_cap", bytes([0x01, 5, 0, 0xFA, 0xFF]) + b"hello", 4, EOUTPUT))
    cases.append(("distance_too_far", fixed_stream([65, (3, 2)]), 100, EDIST))
    cases.append(("distance_before_any_output", fixed_stream([(3, 1)]), 100, EDIST))
    cases.append(("literal_286", fixed_stream([65, 286]), 100, ESYMBOL))
    b = Bits()
    b.put(1, 1), b.put(1, 2), fixed_lit(b, 65), fixed_lit(b, 257), b.code(30, 5)
    cases.append(("distance_code_30", b.bytes() + b"\0" * 4, 100, ESYMBOL))
    cases.append(("clen_oversubscribed", _dynamic_header([1] * 19).bytes() + b"\0" * 8, 100, ECODES))
    cases.append(("clen_incomplete", _dynamic_header([2, 0, 0, 0]).bytes() + b"\0" * 8, 100, ECODES))
    b = _dynamic_header([1, 0, 1, 0])                    # codes for 16 and 18 only: the first symbol is a repeat of nothing
    b.put(0, 1)
    cases.append(("repeat_without_previous", b.bytes() + b"\0" * 8, 100, ECODES))
    b = _dynamic_header([0] * 3 + [1] + [0] * 14 + [1], hlit=31)     # 0 and 1 only; hlit = 288 lengths > 286
    cases.append(("too_many_lengths", b.bytes() + b"\0" * 8, 100, ECODES))
    b = _dynamic_header([0] * 3 + [1] + [0] * 14 + [1])              # every literal/length code length 0: no end-of-block code
    for _ in range(258):
        b.put(0, 1)
    cases.append(("no_end_of_block", b.bytes() + b"\0" * 8, 100, ECODES))
    cases.append(("output_over_cap", good, len(data) - 1, EOUTPUT))
    cases.append(("empty_input", b"", 100, EINPUT))
    rng = np.random.default_rng(9)
    for k in range(40):
        bad = bytearray(good)
        bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        cases.append((f"flipped_{k}", bytes(bad), 1 << 20, None))
    for k in range(20):
        cases.append((f"random_{k}", rng.integers(0, 256, size=int(rng.integers(1, 400)), dtype=np.uint8).tobytes(), 1 << 16, None))
    return cases


CORRUPT = _corrupt_corpus()
FIXED = {c[0]: c for c in CORRUPT if c[3] is not None}                # the 21 cases with a reason of their own
FUZZ = [c for c in CORRUPT if c[3] is None]                           # the 40 flipped and the 20 random streams
TRUNCATED = [c for c in CORRUPT if c[0].startswith("truncated_")]

# (return code, reason, bytes produced, input bytes used) of every fixed-reason case, recorded once on the CPU from the library as it
# was while the member path, the span path and the candidate filter each had a block loop of their own
PINNED = {
    "truncated_0": (-5, 1, 0, 0), "truncated_1": (-5, 1, 0, 1), "truncated_2": (-5, 1, 0, 2), "truncated_5": (-5, 1, 0, 5),
    "truncated_3247": (-5, 1, 9558, 3247), "truncated_6494": (-5, 1, 20000, 6494),
    "block_type_3": (-5, 2, 0, 1), "stored_len_nlen": (-5, 3, 0, 5), "stored_truncated": (-5, 1, 0, 8), "stored_over_cap": (-5, 7, 0, 5),
    "distance_too_far": (-5, 6, 1, 3), "distance_before_any_output": (-5, 6, 0, 2), "literal_286": (-5, 5, 1, 3),
    "distance_code_30": (-5, 5, 1, 3), "clen_oversubscribed": (-5, 4, 0, 10), "clen_incomplete": (-5, 4, 0, 4),
    "repeat_without_previous": (-5, 4, 0, 4), "too_many_lengths": (-5, 4, 0, 3), "no_end_of_block": (-5, 4, 0, 42),
    "output_over_cap": (-5, 7, 19997, 6494), "empty_input": (-5, 1, 0, 0),
}
# the fuzz streams on which dgrp_inflate_raw_host and dgrp_inflate_stream_host refuse with different reasons (chunks of 64 and of
# 1024 bytes): a bad distance is found by the span path's window walk, which runs after the counting pass has decoded the whole
# stream and met whatever error comes later
HOST_ENTRIES_DIFFER = ("random_4", "random_5", "random_6", "random_9", "random_12")


def raw_host(comp: bytes, cap: int):
    """-> (return code, reason, output, input bytes used) of dgrp_inflate_raw_host: where the device tests take a stream's reason"""
    import ctypes as C

    from deepgrp_amd._lib import lib
    out = (C.c_uint8 * max(cap, 1))()
    ol, iu, r = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
    rc = lib().dgrp_inflate_raw_host(comp, len(comp), out, cap, C.byref(ol), C.byref(iu), C.byref(r))
    return rc, r.value, bytes(memoryview(out)[:ol.value]), iu.value


def stream_host(comp: bytes, chunk: int, cap: int, max_span: int = 1 << 22, max_rounds: int = 64):
    """-> (return code, reason, output, input bytes used) of dgrp_inflate_stream_host"""
    import ctypes as C

    from deepgrp_amd._lib import InflateStreamStats, lib
    out = (C.c_uint8 * max(cap, 1))()
    ol, iu, r, st = C.c_int64(-1), C.c_int64(-1), C.c_int(-1), InflateStreamStats()
    rc = lib().dgrp_inflate_stream_host(comp, len(comp), chunk, max_span, max_rounds, out, cap, C.byref(ol), C.byref(iu), C.byref(st),
                                        C.byref(r))
    return rc, r.value, bytes(memoryview(out)[:ol.value]), iu.value


def zlib_says(comp: bytes):
    """(text, input bytes used) when zlib inflates the raw stream to its final block, None when it refuses it or it ends early"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(comp)
    except zlib.error:
        return None
    return (text, len(comp) - len(d.unused_data)) if d.eof else None


# ---------------------------------------------------------------- members
def member(stream: bytes, crc=None, isize=None, cap=None):
    """The raw DEFLATE stream as a gzip member's parts: (data bytes, 8-byte trailer, length of the output slice).  CRC-32, ISIZE and
    the slice are those of the text zlib inflates the stream to unless given; a stream zlib refuses needs all three."""
    if crc is None or isize is None or cap is None:
        text = zlib.decompress(stream, -15)
        crc = zlib.crc32(text) if crc is None else crc
        isize = len(text) if isize is None else isize
        cap = len(text) if cap is None else cap
    return stream, struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff), cap


def bgzf_wrap(data: bytes, trailer: bytes) -> bytes:
    """The member behind an 18-byte BGZF header whose BSIZE frames it (as gz.bgzf_member lays it out, around any bytes)."""
    bsize = 18 + len(data) + len(trailer) - 1
    assert len(trailer) == 8 and bsize <= 0xffff
    return b"\x1f\x8b" + bytes([8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<HBBHH", 6, 66, 67, 2, bsize) + data + trailer


COPY_DIST = (1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 258, 259, 4096, 32768)
COPY_LEN = (3, 4, 63, 64, 65, 66, 127, 128, 129, 257, 258)


@functools.lru_cache(maxsize=None)
def copy_grid():
    """[(name, stream, text)]: for every distance and length of COPY_DIST x COPY_LEN one fixed block of `dist` random literals, the
    match (len, dist), one literal, the match (len, min(len, dist + len + 1)) -- which reads bytes that other lanes wrote for the
    first one, behind a store of lane 0 -- and (258, 1)."""
    out = []
    for dist in COPY_DIST:
        rng = np.random.default_rng(1000 + dist)
        head = Bits()
        head.put(1, 1)
        head.put(1, 2)
        fixed_items(head, rng.integers(0, 256, size=dist).tolist())
        for length in COPY_LEN:
            b = Bits()
            b.acc, b.n = head.acc, head.n
            fixed_items(b, [(length, dist), int(rng.integers(0, 256)), (length, min(length, dist + length + 1)), (258, 1)])
            fixed_lit(b, 256)
            stream = b.bytes()
            text = zlib.decompress(stream, -15)
            assert len(text) == dist + 2 * length + 1 + 258
            out.append((f"d{dist}_l{length}", stream, text))
    return out


STORED_LEN = (0, 1, 63, 64, 65, 4095, 65535)


@functools.lru_cache(maxsize=None)
def stored_grid():
    """[(name, stream, text)]: a final stored block of every LEN of STORED_LEN, alone and behind a fixed block of one literal, which
    ends at bit 18: the stored block's header then starts inside a byte."""
    rng = np.random.default_rng(77)
    out = []
    for n in STORED_LEN:
        body = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        block = struct.pack("<BHH", 1, n, ~n & 0xffff) + body
        out.append((f"stored_{n}", block, body))
        front = fixed_stream([90], final=False)
        assert len(front) == 3 and front[2] < 4                      # 18 bits: the stored block's three header bits are bits 2 .. 4
        joined = front[:2] + bytes([front[2] | 1 << 2]) + block[1:]
        out.append((f"fixed_then_stored_{n}", joined, b"Z" + body))
    for _name, stream, text in out:
        assert zlib.decompress(stream, -15) == text
    return out


SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535, 65536)


@functools.lru_cache(maxsize=None)
def size_grid():
    """[(name, stream, text)]: n bytes of random ACGT at level 6 for every n of SIZES: the edges of the CRC's per-lane piece of
    (n + 63) / 64 bytes, empty pieces among them."""
    rng = np.random.default_rng(64)
    out = []
    for n in SIZES:
        text = rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
        out.append((f"n{n}", deflate(text, 6, zlib.Z_DEFAULT_STRATEGY), text))
    return out
