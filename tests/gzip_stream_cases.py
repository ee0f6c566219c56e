"""The corpus of raw DEFLATE streams that the span decoder is held to on the host (test_inflate_stream_host.py) and on the device
(test_gpu_gzip_stream.py): built once per test run, every stream with the text zlib inflates it to."""
import functools
import zlib

import numpy as np

SETTINGS = {"l1": (1, zlib.Z_DEFAULT_STRATEGY), "l6": (6, zlib.Z_DEFAULT_STRATEGY), "l9": (9, zlib.Z_DEFAULT_STRATEGY),
            "filtered": (6, zlib.Z_FILTERED), "rle": (6, zlib.Z_RLE)}
MAX_SPAN = 1 << 22                    # what the tests allow a span: more than any block of the corpus
MAX_ROUNDS = 64


def deflate(data: bytes, level: int, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: int = 0) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = []
    for k, o in enumerate(range(0, len(data), flush_every)):                 # empty stored blocks, as pigz writes them
        out.append(co.compress(data[o:o + flush_every]) + co.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH))
    return b"".join(out) + co.flush()


def fasta_text(seed: int, nbases: int) -> bytes:
    """Random ACGT with copies of a mutated element, N runs and lower-case stretches, 60 bases a line."""
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=nbases)
    elem = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=300)
    for at in rng.integers(0, nbases - 400, size=nbases // 2000):
        e = elem.copy()
        hit = rng.integers(0, 300, size=6)
        e[hit] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=6)
        seq[at:at + 300] = e
    for at in rng.integers(0, nbases - 6000, size=max(nbases // 200_000, 2)):
        seq[at:at + int(rng.integers(50, 5000))] = ord("N")
    for at in rng.integers(0, nbases - 3000, size=nbases // 20_000):
        n = int(rng.integers(20, 2000))
        seq[at:at + n] |= 0x20
    body = seq.tobytes()
    return b">chr%d synthetic\n" % seed + b"\n".join(body[i:i + 60] for i in range(0, len(body), 60)) + b"\n"


# ---------------------------------------------------------------- hand-written dynamic blocks (streams zlib never emits)
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v: int, k: int):                 # k bits of v, LSB first (header fields, extra bits)
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k

    def code(self, ck):                             # a Huffman code: MSB first
        c, k = ck
        self.put(int(format(c, f"0{k}b")[::-1], 2), k)

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """symbol -> (code, bits) of the canonical code of RFC 1951 3.2.2"""
    code, out = 0, {}
    for bits in range(1, 16):
        for sym, l in enumerate(lengths):
            if l == bits:
                out[sym] = (code, bits)
                code += 1
        code <<= 1
    return out


# literals 9 bits, end of block 2, length 258 (symbol 285) 3, lengths 3 and 4 (257, 258) 4 bits; distance symbols 0 (distance 1) and
# 29 (24577 .. 32768, 13 extra bits) one bit each; the code length code spells every length out (no repeat codes)
_LIT = [9] * 256 + [2, 4, 4] + [0] * 26 + [3]
_DIST = [1] + [0] * 28 + [1]
_CL = {0: 1, 9: 2, 1: 4, 2: 4, 3: 4, 4: 4}
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def hand_block(b: Bits, items, final: bool):
    """One dynamic block of `items`: ints (literals), (258, 1) and (258, 32768) matches."""
    lit, dist, cl = canonical(_LIT), canonical(_DIST), canonical([_CL.get(i, 0) for i in range(19)])
    b.put(int(final), 1)
    b.put(2, 2)
    b.put(286 - 257, 5)
    b.put(30 - 1, 5)
    b.put(19 - 4, 4)
    for i in _ORDER:
        b.put(_CL.get(i, 0), 3)
    for l in _LIT + _DIST:
        b.code(cl[l])
    for it in items:
        if isinstance(it, tuple):
            assert it in ((258, 1), (258, 32768))
            b.code(lit[285])
            if it[1] == 1:
                b.code(dist[0])
            else:
                b.code(dist[29])
                b.put(32768 - 24577, 13)
        else:
            b.code(lit[it])
    b.code(lit[256])


def hand_far() -> bytes:
    """Blocks of 6000 literals; from 32 768 bytes of text on every block opens with three length-258 matches at distance 32 768,
    so at every span start the first symbols are markers for the far end of the window."""
    rng = np.random.default_rng(21)
    b, produced = Bits(), 0
    for k in range(24):
        items = [(258, 32768)] * 3 if produced >= 32768 else []
        items += rng.integers(0, 256, size=6000).tolist()
        if produced + len(items) >= 32768 + 3000:
            items += [(258, 32768)] * 2
        hand_block(b, items, k == 23)
        produced += sum(258 if isinstance(i, tuple) else 1 for i in items)
    return b.bytes()


def hand_run() -> bytes:
    """One literal, then 120 blocks of 64 length-258 matches at distance 1: a run of one byte whose matches cross every span."""
    b = Bits()
    hand_block(b, [ord("N")], False)
    for k in range(120):
        hand_block(b, [(258, 1)] * 64, k == 119)
    return b.bytes()


def hand_big_run(nunits: int, m: int = 1000):
    """-> (stream, bytes of text): the literal `N`, then nunits * 8 blocks of m length-258 matches at distance 1, then a final block
    of three.  Eight equal blocks are a whole number of bytes, so the stream is spliced from the bytes of a two-unit stream
    without encoding every unit: gigabytes of text (all `N`) from a few megabytes, for indices beyond 2^31."""
    def build(units, final):
        b = Bits()
        hand_block(b, [ord("N")], False)
        p0 = b.n
        for k in range(8 * units):
            hand_block(b, [(258, 1)] * m, False)
        if final:
            hand_block(b, [(258, 1)] * 3, True)
        return b.bytes(), p0, b.n
    two, p0, _ = build(2, False)
    one, _, _ = build(1, True)
    unit_bytes = (build(1, False)[2] - p0) // 8
    a = (p0 + 7) // 8
    stream = two[:a] + two[a:a + unit_bytes] * (nunits - 1) + one[a:]
    return stream, 1 + (8 * nunits * m + 3) * 258


@functools.lru_cache(maxsize=None)
def texts():
    rng = np.random.default_rng(17)
    text = fasta_text(1, 1_500_000)
    unit = rng.integers(0, 256, size=40_000, dtype=np.uint8).tobytes()
    u32 = np.tile(np.frombuffer(unit[:32_000], np.uint8), 25)                # every copy differs from the unit in one byte of 20:
    hit = rng.integers(0, u32.size, size=u32.size // 20)                     # short matches at distances of 32 000, many blocks
    u32[hit] = rng.integers(0, 256, size=hit.size, dtype=np.uint8)
    return {"fasta": text, "run": b"A" * 200_000, "unit": unit * 20, "unit32": u32.tobytes(), "flush": text[:700_000],
            "half": text[:300_000] + rng.integers(0, 256, size=200_000, dtype=np.uint8).tobytes()}


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> (stream, text)"""
    out = {}
    for tname, data in texts().items():
        for sname, (level, strategy) in SETTINGS.items():
            comp = deflate(data, level, strategy, 100_000 if tname == "flush" else 0)
            out[f"{tname}-{sname}"] = (comp, data)
    for name, comp in (("hand_far", hand_far()), ("hand_run", hand_run())):
        out[name] = (comp, zlib.decompress(comp, -15))
    return out


# The seed of a level-1 FASTA stream in which the finder accepts a bit offset that is no block start (found by
# tools/find_false_start.py; the bytes are rebuilt from the seed)
FALSE_START = {"seed": 3030, "nbases": 1_500_000, "chunk": 19 << 10}
