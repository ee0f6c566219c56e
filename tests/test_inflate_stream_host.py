"""Plain gzip without a GPU: dgrp_inflate_stream_host -- the finder, the counting pass, the chain with repair, the marker pass, the
window walk and the resolve pass, the code the device runs -- against zlib, byte for byte, over a corpus of raw DEFLATE streams at
chunk sizes of 1, 4 and 32 KiB, with the statistics that show the spans were really cut, and a corrupt corpus.

Two inputs of the corpus cannot give more than one span, whatever decodes them, and the test says so instead of asking for it:
`run` (200 000 times one byte) deflates to 211 .. 891 bytes, less than one chunk; `unit` (a random 40 000-byte unit, 20 times) has no
match inside a 32 KiB window, so under the default strategy zlib writes stored blocks only and the finder has nothing to find.
What they were meant to show is shown by `hand_run` (distance-1 matches across every span start, 14 spans at 1 KiB) and by
`unit32` (a 32 000-byte unit: distances of 32 000 across span starts)."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_stream_cases as gc                         # noqa: E402
from deepgrp_amd._lib import InflateStreamStats, lib   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDATA = -1, -5
EINPUT, EOUTPUT, ESPAN, EROUNDS = 1, 7, 11, 12
NAMES = ("dgrp_inflate_stream_host", "dgrp_inflate_stream_workspace_bytes", "dgrp_inflate_stream_scan", "dgrp_inflate_stream_write")
GUARD = 4096
CHUNKS = (1 << 10, 4 << 10, 32 << 10)


def stream_host(comp: bytes, chunk: int, cap: int, max_span: int = gc.MAX_SPAN, max_rounds: int = gc.MAX_ROUNDS):
    """-> (return code, output, input bytes used, reason, statistics); guard bytes on both sides of the output must survive"""
    buf = np.full(cap + 2 * GUARD, 0xa5, np.uint8)
    ol, iu, r, st = C.c_int64(-1), C.c_int64(-1), C.c_int(-1), InflateStreamStats()
    rc = lib().dgrp_inflate_stream_host(comp, len(comp), chunk, max_span, max_rounds, buf.ctypes.data + GUARD, cap, C.byref(ol), C.byref(iu),
                                        C.byref(st), C.byref(r))
    assert (buf[:GUARD] == 0xa5).all() and (buf[GUARD + cap:] == 0xa5).all(), "wrote outside [0, out_cap)"
    assert 0 <= ol.value <= cap and 0 <= iu.value <= len(comp)
    if rc != 0:
        assert ol.value == 0 and iu.value == 0
    return rc, buf[GUARD:GUARD + ol.value].tobytes(), iu.value, r.value, st.as_dict()


def test_symbols_declared_exported_and_bound():
    from deepgrp_amd import _lib, gz
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    L = lib()
    for name in NAMES:
        assert f" {name}(" in header and name in _lib.exported_symbols() and hasattr(L, name), name
    assert "} dgrp_inflate_stream_stats;" in header and C.sizeof(InflateStreamStats) == 64
    assert "#define DGRP_INFLATE_ESPAN 11" in header and "#define DGRP_INFLATE_EROUNDS 12" in header
    assert set(gz.REASONS) == set(range(1, 13))
    make = open(os.path.join(ROOT, "deepgrp_amd", "csrc", "Makefile")).read()
    assert "inflate_stream_kernels.o: inflate_stream_kernels.hip inflate_stream.h inflate.h" in make
    for const in ("PLAIN_CHUNK_BYTES", "PLAIN_MAX_SPAN_BYTES", "PLAIN_MAX_ROUNDS", "PLAIN_DEVICE_MIN_BYTES"):
        assert getattr(gz, const) > 0
    assert 64 <= gz.PLAIN_CHUNK_BYTES <= gz.PLAIN_MAX_SPAN_BYTES < 1 << 31


ONE_SPAN = {"run": "the stream is shorter than one chunk", "unit": "stored blocks only"}


def one_span_reason(name, comp, st):
    """Why this stream of the corpus has one span at 4 KiB, checked; None for every stream that must have more."""
    text, _, setting = name.partition("-")
    if text == "run":
        assert len(comp) < 1 << 10
        return ONE_SPAN["run"]
    if text == "unit" and setting in ("l1", "l6", "l9"):
        assert st["candidates"] == 0 and len(comp) > 20 * 40_000           # nothing was compressed: stored blocks
        return ONE_SPAN["unit"]
    return None


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(gc.corpus()))
def test_stream_host_equals_zlib(name, chunk):
    comp, want = gc.corpus()[name]
    assert zlib.decompress(comp, -15) == want
    rc, got, used, reason, st = stream_host(comp, chunk, len(want))
    print(name, chunk, len(comp), st)
    assert (rc, reason) == (0, 0)                                          # no refusal: the caller does not fall back
    assert got == want and used == len(comp)
    assert st["chunks"] == max(1, -(-len(comp) // chunk)) and 1 <= st["spans"] <= st["chunks"] and st["rounds"] >= 1
    assert st["longest_span"] <= len(comp) and st["false_starts"] <= st["repaired"]
    if chunk == 4 << 10 and one_span_reason(name, comp, st) is None:
        assert st["spans"] > 1 and st["candidates"] >= 1
    # the same text with room to spare, and refused as a whole one byte short of it
    if chunk == 4 << 10:
        assert stream_host(comp, chunk, len(want) + 100)[1] == want
        if want:
            rc, got, used, reason, _ = stream_host(comp, chunk, len(want) - 1)
            assert (rc, reason, got, used) == (EDATA, EOUTPUT, b"", 0)


def test_short_spans_take_their_window_through_several_spans():
    """hand_far at 1 KiB: spans of 6 000 .. 7 000 bytes of text whose first symbols are markers for window byte 0, 32 768 bytes and
    five spans back -- the case only the window walk sees."""
    comp, want = gc.corpus()["hand_far"]
    rc, got, _, _, st = stream_host(comp, 1 << 10, len(want))
    assert rc == 0 and got == want
    assert st["spans"] == 24 and len(want) / st["spans"] < 8192


def test_the_spliced_run_is_the_stream_it_stands_for():
    """gzip_stream_cases.hand_big_run, which the device test uses for 2.3 GB of text: at a small size the spliced bytes inflate, by
    zlib and by the host entry, to the run they claim."""
    for nunits, m in ((1, 40), (3, 50), (5, 7)):
        comp, total = gc.hand_big_run(nunits, m)
        want = zlib.decompress(comp, -15)
        assert want == b"N" * total
        rc, got, used, reason, st = stream_host(comp, 1 << 10, total)
        assert (rc, reason, used) == (0, 0, len(comp)) and got == want


def test_a_false_start_is_repaired():
    """The seeded level-1 FASTA stream in which a bit offset that is no block start passes the whole candidate filter, in the chunk
    and in front of the block start the chain lands on (tools/find_false_start.py found the seed)."""
    fs = gc.FALSE_START
    text = gc.fasta_text(fs["seed"], fs["nbases"])
    comp = gc.deflate(text, 1)
    rc, got, used, reason, st = stream_host(comp, fs["chunk"], len(text))
    print(st)
    assert (rc, reason) == (0, 0) and got == text and used == len(comp)
    assert st["false_starts"] >= 1 and st["repaired"] >= st["false_starts"] and st["rounds"] >= 2


def _unfindable():
    data = gc.texts()["fasta"][:200_000]
    return {"fixed": (gc.deflate(data, 6, zlib.Z_FIXED), data), "level0": (gc.deflate(data, 0), data),
            "empty": (gc.deflate(b"", 6), b""), "one_byte": (gc.deflate(b"G", 6), b"G")}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ["fixed", "level0", "empty", "one_byte"])
def test_streams_without_findable_starts_are_one_span(name, chunk):
    comp, want = _unfindable()[name]
    rc, got, used, reason, st = stream_host(comp, chunk, len(want), max_span=len(comp))
    assert (rc, reason, got, used) == (0, 0, want, len(comp))
    assert (st["spans"], st["candidates"], st["repaired"], st["rounds"], st["longest_span"]) == (1, 0, 0, 1, len(comp))
    rc, got, used, reason, st = stream_host(comp, chunk, len(want), max_span=len(comp) - 1)
    assert (rc, reason, got, used) == (EDATA, ESPAN, b"", 0)


def test_huffman_only_is_an_ordinary_case_until_the_span_limit_says_otherwise():
    """Z_HUFFMAN_ONLY at level 6: dynamic blocks of 32 767 literals, about 9 KB each at 2.2 bits a base -- found like any other
    block; with a span limit below a block it is refused with the span reason."""
    data = gc.texts()["fasta"][:400_000]
    comp = gc.deflate(data, 6, zlib.Z_HUFFMAN_ONLY)
    rc, got, used, reason, st = stream_host(comp, 4 << 10, len(data))
    print(len(comp), st)
    assert (rc, reason, got, used) == (0, 0, data, len(comp))
    assert st["spans"] == 13 and st["candidates"] == 11 and 8_000 < st["longest_span"] < 12_000
    rc, got, used, reason, st = stream_host(comp, 4 << 10, len(data), max_span=4 << 10)
    assert (rc, reason) == (EDATA, ESPAN)


def test_the_round_limit_refuses():
    comp, want = gc.corpus()["half-l6"]                                     # a stored block behind a stored block: a round each
    rc, got, _, reason, st = stream_host(comp, 4 << 10, len(want))
    assert rc == 0 and st["rounds"] > 3
    rc, got, used, reason, _ = stream_host(comp, 4 << 10, len(want), max_rounds=st["rounds"] - 1)
    assert (rc, reason, got, used) == (EDATA, EROUNDS, b"", 0)
    assert stream_host(comp, 4 << 10, len(want), max_rounds=st["rounds"])[1] == want


def test_error_text_of_the_span_and_round_limits():
    comp, want = _unfindable()["fixed"]
    assert stream_host(comp, 4 << 10, len(want), max_span=len(comp) - 1)[3] == ESPAN
    assert lib().dgrp_last_error().decode() == "dgrp_inflate_stream_host: a span longer than max_span_bytes (reason 11)"
    comp, want = gc.corpus()["half-l6"]
    assert stream_host(comp, 4 << 10, len(want), max_rounds=3)[3] == EROUNDS
    assert lib().dgrp_last_error().decode() == "dgrp_inflate_stream_host: the chain is not closed after max_rounds rounds (reason 12)"


def _edge_stream(valid: bool) -> bytes:
    """A stored block of zero bytes that ends at byte 33 * 1024 (no bit offset inside zeros reads BFINAL = 0, BTYPE = 2), then a
    hand-built non-final dynamic block whose first symbol is a match of distance 32 768, then a final block -- or, in place of it,
    the header of a block of type 3."""
    b = gc.Bits()
    b.put(0, 3)
    b.n = 8
    n = 33 * 1024 - 5
    b.put(n, 16), b.put(~n & 0xffff, 16)
    b.n += 8 * n
    assert b.n == 8 * 33 * 1024
    gc.hand_block(b, [(258, 32768), 65, 66], False)
    if valid:
        gc.hand_block(b, [67], True)
    else:
        b.put(1, 1), b.put(3, 2)
    return b.bytes()


def test_a_candidate_may_reach_the_whole_window_at_position_0():
    """The block at the start of chunk 33 (chunks of 1 KiB) opens with a match of distance 32 768 at span position 0: the candidate
    filter must let a match reach the whole window in front of the span, so it is found and the stream is two spans.  DEFLATE has
    no distance above 32 768 (distance symbol 29 with all 13 extra bits set; a dynamic block has no symbol 30), so the refusal of
    a farther one cannot be put into a stream; the block that must not be found is the same one with a block of type 3 behind it."""
    comp = _edge_stream(True)
    want = zlib.decompress(comp, -15)
    rc, got, used, reason, st = stream_host(comp, 1 << 10, len(want))
    assert (rc, reason, got, used) == (0, 0, want, len(comp))
    assert (st["chunks"], st["candidates"], st["spans"], st["repaired"], st["longest_span"]) == (34, 1, 2, 0, 33 * 1024)
    rc, got, used, reason, st = stream_host(_edge_stream(False), 1 << 10, 100_000)
    assert (rc, reason, st["chunks"], st["candidates"]) == (EDATA, 2, 34, 0)


def _zlib_says(comp: bytes):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp)
    except zlib.error:
        return None
    return (out, len(comp) - len(d.unused_data)) if d.eof else None


def _corrupt():
    comp, want = gc.corpus()["fasta-l6"]
    cases = {}

    def flip(name, byte, bit):
        b = bytearray(comp)
        b[byte] ^= 1 << bit
        cases[name] = bytes(b)
    flip("header0", 1, 3)                      # the first block's header
    flip("header_mid", 0, 1)                   # block type 2 -> 0
    for k, at in enumerate((5_000, 77_777, 200_001, 300_123)):
        flip(f"body{k}", at, k)
    flip("last_block", len(comp) - 300, 2)
    flip("last_byte", len(comp) - 1, 0)
    cases["truncated_mid"] = comp[:len(comp) // 2]
    cases["truncated_end"] = comp[:-1]
    cases["trailing"] = comp + b"\x1f\x8b trailing bytes"
    b = gc.Bits()
    gc.hand_block(b, [65, 66, 67], False)
    gc.hand_block(b, [(258, 32768)], True)     # a distance before the start of the text
    cases["distance_before_start"] = b.bytes()
    comp2 = bytearray(gc.corpus()["hand_far"][0])
    for at in (9_000, 40_000, 100_000):
        comp2[at] ^= 0x10
    cases["hand_far_flips"] = bytes(comp2)
    return cases


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", sorted(_corrupt()))
def test_corrupt_streams_agree_with_zlib_on_validity(name, chunk):
    comp = _corrupt()[name]
    say = _zlib_says(comp)
    cap = len(say[0]) if say else 2_000_000
    rc, got, used, reason, st = stream_host(comp, chunk, cap)
    print(name, chunk, "zlib:", "valid" if say else "invalid", "rc", rc, "reason", reason)
    if say:
        assert (rc, reason) == (0, 0) and got == say[0] and used == say[1]
    else:
        assert rc == EDATA and 1 <= reason <= 12 and "dgrp_inflate_stream_host" in lib().dgrp_last_error().decode()
        assert got == b"" and used == 0


def test_argument_checks():
    L = lib()
    comp, want = gc.corpus()["hand_run"]
    out = (C.c_uint8 * len(want))()
    ol, iu, r, st = C.c_int64(), C.c_int64(), C.c_int(), InflateStreamStats()

    def call(inp=comp, n=len(comp), chunk=4096, span=gc.MAX_SPAN, rounds=8, o=out, cap=len(want), pol=C.byref(ol), piu=C.byref(iu),
             pst=C.byref(st), pr=C.byref(r)):
        return L.dgrp_inflate_stream_host(inp, n, chunk, span, rounds, o, cap, pol, piu, pst, pr)
    assert call() == 0 and bytes(out) == want
    for kw in (dict(n=-1), dict(chunk=63), dict(chunk=(1 << 28) + 1), dict(span=0), dict(span=1 << 31), dict(rounds=0), dict(cap=-1),
               dict(inp=None), dict(o=None), dict(pol=None), dict(piu=None), dict(pst=None), dict(pr=None), dict(n=1 << 40)):
        assert call(**kw) == EINVAL, kw
        assert "dgrp_inflate_stream_host" in L.dgrp_last_error().decode()
    assert call(inp=None, n=0) == EDATA and r.value == EINPUT               # no stream at all
    ws = L.dgrp_inflate_stream_workspace_bytes
    assert ws(0, 4096) > 0 and ws(1 << 20, 4096) > ws(1 << 20, 32768) > 0 and ws(1 << 30, 32768) > ws(1 << 20, 32768)
    assert ws(-1, 4096) == 0 and ws(100, 63) == 0 and ws(100, (1 << 28) + 1) == 0 and ws(1 << 40, 4096) == 0
    # the device entries check their arguments before anything is launched (no device is touched here)
    tot, crc = C.c_int64(), C.c_uint32()
    P, wb = 0x10000, ws(1000, 4096)
    scan, write = L.dgrp_inflate_stream_scan, L.dgrp_inflate_stream_write
    for args in ((None, 1000, 0, 4096, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), None, wb, None),
                 (P, 1000, 1001, 4096, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, -1, 4096, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 32, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, 0, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, 1 << 20, 0, C.byref(tot), C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, 1 << 20, 8, None, C.byref(st), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, 1 << 20, 8, C.byref(tot), None, C.byref(r), P, wb, None)):
        assert scan(*args) == EINVAL, args
    assert scan(P, 1000, 0, 4096, 1 << 20, 8, C.byref(tot), C.byref(st), C.byref(r), P, wb - 1, None) == -3
    for args in ((None, 1000, 0, 4096, P, P, 10, C.byref(crc), C.byref(iu), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, None, P, 10, C.byref(crc), C.byref(iu), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, P, None, 10, C.byref(crc), C.byref(iu), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, P, P, -1, C.byref(crc), C.byref(iu), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, P, P, 10, None, C.byref(iu), C.byref(r), P, wb, None),
                 (P, 1000, 0, 4096, P, P, 10, C.byref(crc), C.byref(iu), C.byref(r), None, wb, None),
                 (P, 1000, 2000, 4096, P, P, 10, C.byref(crc), C.byref(iu), C.byref(r), P, wb, None)):
        assert write(*args) == EINVAL, args
    assert write(P, 1000, 0, 4096, P, P, 10, C.byref(crc), C.byref(iu), C.byref(r), P, wb - 1, None) == -3


def test_plain_member_header():
    import gzip
    from deepgrp_amd import gz
    body = gc.deflate(b"ACGT" * 100, 6)
    tail = b"\0" * 8
    assert gz.plain_data_off(gzip.compress(b"ACGT" * 100, mtime=7)) == 10
    assert gz.plain_data_off(b"\x1f\x8b\x08\x08" + b"\0" * 6 + b"name.fa\0" + body + tail) == 18
    both = b"\x1f\x8b\x08\x1e" + b"\0" * 6 + b"\x03\x00abc" + b"n\0" + b"a comment\0" + b"\x12\x34"
    assert gz.plain_data_off(both + body + tail) == len(both)
    assert gz.plain_data_off(b"\x1f\x8b\x08\x08" + b"\0" * 6 + b"no terminator" + body) is None
    assert gz.plain_data_off(b"\x1f\x8b\x08\x20" + b"\0" * 6 + body + tail) is None      # a reserved flag
    assert gz.plain_data_off(b"\x1f\x8b\x08\x00" + b"\0" * 6 + b"\x03\x00") is None      # no room for a trailer
    assert gz.plain_data_off(b"\x1f\x8b\x07\x00" + b"\0" * 20) is None
