"""Compressed input without a GPU: the host entry of the DEFLATE decode core (dgrp_inflate_raw_host, the same code the device
runs) against zlib, a corrupt corpus that must come back as reasons, the argument checks of both entries, the gzip member walk,
and the refusals of compressed input that happen before any device work."""
import ctypes as C
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inflate_cases import CORRUPT, INPUTS, PINNED, deflate, fixed_stream   # noqa: E402  (the corpus, shared with the GPU tests)

from deepgrp_amd import gz                           # noqa: E402
from deepgrp_amd._lib import lib                     # noqa: E402

EINVAL, ENOMEM, EDATA = -1, -3, -5
EINPUT, EBLOCK, ESTORED, ECODES, ESYMBOL, EDIST, EOUTPUT = 1, 2, 3, 4, 5, 6, 7
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman_only": zlib.Z_HUFFMAN_ONLY,
              "filtered": zlib.Z_FILTERED}


def inflate(comp: bytes, cap: int):
    """-> (return code, output, input bytes used, reason)"""
    out = (C.c_uint8 * max(cap, 1))()
    ol, iu, r = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
    rc = lib().dgrp_inflate_raw_host(comp, len(comp), out, cap, C.byref(ol), C.byref(iu), C.byref(r))
    assert 0 <= ol.value <= cap and 0 <= iu.value <= len(comp)
    return rc, bytes(out[:ol.value]), iu.value, r.value


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_host_entry_equals_zlib(name, level, strategy):
    data = INPUTS[name]
    comp = deflate(data, level, STRATEGIES[strategy])
    want = zlib.decompress(comp, -15)
    assert want == data
    rc, out, used, reason = inflate(comp, len(data))
    assert (rc, reason) == (0, 0)
    assert out == want and used == len(comp)


def test_hand_encoded_longest_match_at_the_farthest_distance():
    rng = np.random.default_rng(2)
    lits = rng.integers(0, 256, size=32_768).tolist()
    items = lits + [(258, 32_768), (258, 32_768), (3, 1), (258, 1)]
    comp = fixed_stream(items)
    want = zlib.decompress(comp, -15)
    assert len(want) == 32_768 + 2 * 258 + 3 + 258
    rc, out, used, reason = inflate(comp, len(want))
    assert (rc, reason) == (0, 0) and out == want and used == len(comp)
    assert inflate(comp, len(want) - 1)[3] == EOUTPUT          # one byte short


def test_output_of_exactly_64k_and_over_the_cap():
    data = INPUTS["max"]
    for level in (0, 6):
        comp = deflate(data, level, zlib.Z_DEFAULT_STRATEGY)
        assert inflate(comp, 65536)[:2] == (0, data)
        rc, out, _used, reason = inflate(comp, 65535)
        assert (rc, reason) == (EDATA, EOUTPUT) and out == data[:len(out)]


@pytest.mark.parametrize("name,stream,cap,reason", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupt_corpus(name, stream, cap, reason):
    rc, out, used, got = inflate(stream, cap)
    if reason is not None:
        assert (rc, got) == (EDATA, reason)
        return
    # no expectation of our own: agree with zlib on whether the stream is valid, and on its output where it is
    d = zlib.decompressobj(-15)
    try:
        want = d.decompress(stream)
        ok = d.eof and len(want) <= cap
    except zlib.error:
        ok = False
    if ok:
        assert (rc, got, out, used) == (0, 0, want, len(stream) - len(d.unused_data))
    else:
        assert rc == EDATA and got > 0


# one case of each reason a host entry can give, and the words dgrp_last_error() has for it
TEXTS = {"truncated_5": "input ends inside the stream", "block_type_3": "invalid block type", "stored_len_nlen": "stored block LEN/NLEN mismatch",
         "clen_incomplete": "invalid code lengths", "literal_286": "invalid symbol", "distance_too_far": "distance too far back",
         "stored_over_cap": "output beyond its size"}


def test_corrupt_corpus_results_are_pinned():
    fixed = {c[0]: c for c in CORRUPT if c[3] is not None}
    assert set(fixed) == set(PINNED)
    for name, (_, stream, cap, reason) in fixed.items():
        rc, out, used, got = inflate(stream, cap)
        assert (rc, got, len(out), used) == PINNED[name] and got == reason, name


def test_error_text_of_both_host_entries():
    from deepgrp_amd._lib import InflateStreamStats
    fixed = {c[0]: c for c in CORRUPT}
    assert sorted(PINNED[name][1] for name in TEXTS) == [EINPUT, EBLOCK, ESTORED, ECODES, ESYMBOL, EDIST, EOUTPUT]
    for name, text in TEXTS.items():
        _, stream, cap, reason = fixed[name]
        rc, _out, used, got = inflate(stream, cap)
        assert (rc, got) == (EDATA, reason)
        assert lib().dgrp_last_error().decode() == f"dgrp_inflate_raw_host: {text} (reason {reason}) near input byte {used}"
        out = (C.c_uint8 * cap)()
        ol, iu, r, st = C.c_int64(), C.c_int64(), C.c_int(), InflateStreamStats()
        rc = lib().dgrp_inflate_stream_host(stream, len(stream), 1 << 10, 1 << 22, 64, out, cap, C.byref(ol), C.byref(iu), C.byref(st), C.byref(r))
        assert (rc, r.value) == (EDATA, reason)
        assert lib().dgrp_last_error().decode() == f"dgrp_inflate_stream_host: {text} (reason {reason})"


def test_reason_nine_keeps_both_wordings():
    """DGRP_INFLATE_EISIZE is what the trailer check of the member kernel gives, and what a span's second decode gives when it
    disagrees with its count, which no stream makes the host do.  So no host entry can show its text: the one table both paths
    share must still hold the member's wording and the span's."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepgrp_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("inflate.h", "inflate_stream.h", "inflate_kernels.hip", "inflate_stream_kernels.hip"))
    assert text.count('"output shorter than ISIZE"') == 1 and text.count('"a span decoded differently than it was counted"') == 1
    assert text.count("case DGRP_INFLATE_EISIZE:") == 1


# ---------------------------------------------------------------- argument checks (DGRP_EINVAL without a GPU)
P = 0x10000
I64 = lambda: C.pointer(C.c_int64())
INT = lambda: C.pointer(C.c_int())

ARG_CASES = [
    ("dgrp_inflate_raw_host", lambda: (P, 10, P, 10, None, I64(), INT()), EINVAL),
    ("dgrp_inflate_raw_host", lambda: (P, 10, P, 10, I64(), I64(), None), EINVAL),
    ("dgrp_inflate_raw_host", lambda: (P, -1, P, 10, I64(), I64(), INT()), EINVAL),
    ("dgrp_inflate_raw_host", lambda: (P, 10, P, 1 << 31, I64(), I64(), INT()), EINVAL),
    ("dgrp_inflate_raw_host", lambda: (None, 10, P, 10, I64(), I64(), INT()), EINVAL),
    ("dgrp_inflate_raw_host", lambda: (P, 10, None, 10, I64(), I64(), INT()), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, -1, None, None, None, P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, None, None, None, P, 100, None, INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, None, None, None, P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, *_tab([0], [93], [0, 10]), P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, *_tab([-1], [10], [0, 10]), P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, *_tab([0], [10], [0, 101]), P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 2, *_tab([0, 20], [10, 10], [0, 10, 5]), P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (None, 100, 1, *_tab([0], [10], [0, 10]), P, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, *_tab([0], [10], [0, 10]), None, 100, I64(), INT(), P, 1 << 20, None), EINVAL),
    ("dgrp_inflate_batch", lambda: (P, 100, 1, *_tab([0], [10], [0, 10]), P, 100, I64(), INT(), P, 8, None), ENOMEM),
]
_KEEP = []


def _tab(in_off, in_len, out_off):
    arrs = [np.asarray(a, np.int64) for a in (in_off, in_len, out_off)]
    _KEEP.append(arrs)
    return [a.ctypes.data for a in arrs]


@pytest.mark.parametrize("k", range(len(ARG_CASES)))
def test_argument_checks(k):
    name, args, code = ARG_CASES[k]
    assert getattr(lib(), name)(*args()) == code
    assert name.encode() in lib().dgrp_last_error()


def test_batch_with_no_members_is_a_no_op():
    bad, reason = C.c_int64(7), C.c_int(7)
    assert lib().dgrp_inflate_batch(None, 0, 0, None, None, None, None, 0, C.byref(bad), C.byref(reason), None, 0, None) == 0
    assert (bad.value, reason.value) == (-1, 0)


# ---------------------------------------------------------------- the member walk
def test_walk_bgzf_with_eof_block():
    data = INPUTS["fasta"] * 3
    comp = gz.bgzf_compress(data)
    m = gz.walk_members(comp)
    assert m.kind == "bgzf" and m.size == len(comp)
    assert m.start.size == (len(data) + gz.BGZF_BLOCK - 1) // gz.BGZF_BLOCK + 1 and m.isize[-1] == 0
    assert int(m.isize.sum()) == len(data) and m.start[0] == 0
    for k in range(m.start.size):                        # every member's DEFLATE data inflates to its ISIZE
        raw = comp[m.data_off[k]:m.data_off[k] + m.data_len[k]]
        assert len(zlib.decompress(raw, -15)) == m.isize[k]
    only_eof = gz.walk_members(gz.BGZF_EOF)
    assert only_eof.kind == "bgzf" and only_eof.isize.tolist() == [0]


def test_walk_other_gzip():
    data = INPUTS["fasta"]
    assert gz.walk_members(gzip.compress(data)).kind == "gzip"                                 # one member, FNAME-less gzip
    assert gz.walk_members(gz.bgzf_compress(data, eof=False) + gzip.compress(data)).kind == "gzip"   # mixed members
    big = gz.bgzf_member(b"A" * 100)
    big = big[:-4] + (70_000).to_bytes(4, "little")                                         # ISIZE above 64 KiB: not BGZF
    assert gz.walk_members(big).kind == "gzip"


def test_walk_truncated_and_trailing_garbage():
    comp = gz.bgzf_compress(INPUTS["fasta"] * 3, eof=False)
    m = gz.walk_members(comp)
    last = int(m.start[-1])
    with pytest.raises(gz.GzipError) as e:
        gz.walk_members(comp[:-10], "t.fa.gz")
    assert e.value.offset == last and "t.fa.gz" in str(e.value) and f"offset {last}" in str(e.value)
    with pytest.raises(gz.GzipError) as e:
        gz.walk_members(comp[:last + 7], "t.fa.gz")
    assert e.value.offset == last
    with pytest.raises(gz.GzipError) as e:
        gz.walk_members(comp + b"trailing garbage here", "t.fa.gz")
    assert e.value.offset == len(comp)


def test_zlib_path_names_the_bad_member():
    a, b = INPUTS["fasta"], INPUTS["nrun"]
    ga, gb = gzip.compress(a), gzip.compress(b)
    assert gz.inflate_host(ga + gb, "x.gz", 1 << 30) == a + b
    bad = bytearray(ga + gb)
    bad[len(ga) + len(gb) - 6] ^= 1                                  # second member's CRC-32
    with pytest.raises(gz.GzipError) as e:
        gz.inflate_host(bytes(bad), "x.gz", 1 << 30)
    assert e.value.offset == len(ga)
    with pytest.raises(gz.GzipError) as e:
        gz.inflate_host(ga + gb[:len(gb) // 2], "x.gz", 1 << 30)
    assert e.value.offset == len(ga) and "truncated" in str(e.value)
    with pytest.raises(ValueError, match="inflates to more than"):
        gz.inflate_host(ga + gb, "x.gz", len(a) + 10)


# ---------------------------------------------------------------- refusals before any device work
@pytest.fixture
def no_gpu(monkeypatch):
    """Any attempt to reach the device fails the test."""
    from deepgrp_amd import pipeline

    def touched(*_a, **_k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(pipeline, "require_gpu", touched)


@pytest.mark.parametrize("form", ["bgzf", "gzip"])
def test_refuses_inflated_size_above_resident_bytes(tmp_path, monkeypatch, no_gpu, form):
    from deepgrp_amd import fasta
    data = INPUTS["fasta"]
    p = tmp_path / "x.fa.gz"
    p.write_bytes(gz.bgzf_compress(data) if form == "bgzf" else gzip.compress(data))
    monkeypatch.setattr(fasta, "RESIDENT_BYTES", len(data) - 1)
    with pytest.raises(ValueError, match="inflates to more than"):
        list(fasta.read_multi_fasta_device(str(p)))


def test_corrupt_plain_gzip_is_refused_before_the_device(tmp_path, no_gpu):
    from deepgrp_amd import fasta
    comp = bytearray(gzip.compress(INPUTS["fasta"]))
    comp[-7] ^= 2
    p = tmp_path / "x.fa.gz"
    p.write_bytes(bytes(comp))
    with pytest.raises(gz.GzipError, match="offset 0"):
        list(fasta.read_multi_fasta_device(str(p)))


def test_cli_refuses_sharded_and_masked_compressed_input(tmp_path, monkeypatch, no_gpu):
    from deepgrp_amd.__main__ import main
    p = tmp_path / "in.fa"                                              # the name does not matter: the magic bytes do
    p.write_bytes(gz.bgzf_compress(INPUTS["fasta"]))
    model = str(tmp_path / "no_model.h5")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        main(["predict", model, str(p)])
    assert "cannot be sharded" in str(e.value.code) and str(p) in str(e.value.code)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit) as e:
        main(["predict", model, str(p), "--mask_dir", str(tmp_path / "m")])
    assert "--mask_dir" in str(e.value.code) and "gzip" in str(e.value.code)
    assert not (tmp_path / "m").exists()
