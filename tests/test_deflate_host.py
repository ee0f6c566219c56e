"""BGZF output without a GPU: the host entry of the DEFLATE encode core (dgrp_bgzf_compress_host, the same code the device runs)
against zlib's and the project's own decoder over a corpus, its size against zlib's Z_HUFFMAN_ONLY, the argument checks of both
entries, and the command line's --mask_gzip parsing and refusals."""
import ctypes as C
import os
import zlib

import pytest

from conftest import GOLDEN
from deflate_corpus import BLOCK, EINVAL, ENOMEM, SIZE_BOUND, check_file, compress_host, corpus

CORPUS = corpus()


@pytest.mark.parametrize("eof", [True, False])
@pytest.mark.parametrize("name", sorted(CORPUS))
def test_host_encoder_output_is_bgzf_of_the_input(name, eof):
    data = CORPUS[name]
    out = compress_host(data, eof)
    check_file(out, data, eof)
    if name == "empty":
        from deepgrp_amd import gz
        assert out == (gz.BGZF_EOF if eof else b"")


def test_random_bytes_become_stored_blocks():
    data = CORPUS["random"]
    out = compress_host(data, True)
    nmem = (len(data) + BLOCK - 1) // BLOCK
    assert len(out) <= len(data) + 31 * nmem + 28
    assert data[:1000] in out                                       # stored: the bytes as they are


def test_fixtures_need_the_length_limit():
    """The unlimited Huffman code of the Fibonacci text is deeper than 15 bits (so the limit is exercised, not assumed)."""
    import heapq
    data = CORPUS["fibonacci"]
    freq = [data.count(bytes([b])) for b in range(256)]
    heap = [(f, 0) for f in freq if f] + [(1, 0)]
    heapq.heapify(heap)
    while len(heap) > 1:
        (fa, da), (fb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1))
    assert heap[0][1] > 15


@pytest.mark.parametrize("name", SIZE_BOUND)
def test_size_against_zlib_huffman_only(name):
    from deepgrp_amd import gz
    data = CORPUS[name]
    ours, theirs = len(compress_host(data, True)), len(gz.bgzf_compress(data, 6, zlib.Z_HUFFMAN_ONLY))
    print(f"{name}: {len(data)} bytes -> {ours} (zlib Z_HUFFMAN_ONLY {theirs}, ratio {ours / theirs:.4f})")
    assert ours <= 1.03 * theirs


def test_python_wrapper_equals_the_entry():
    from deepgrp_amd import gz
    data = CORPUS["len_block_plus_1"]
    assert gz.bgzf_compress_host(data) == compress_host(data, True)
    assert gz.bgzf_compress_host(data, eof=False) == compress_host(data, False)
    assert gz.BGZF_BLOCK == BLOCK


# ---------------------------------------------------------------- argument checks
def test_bound_and_workspace():
    from deepgrp_amd._lib import lib
    L = lib()
    assert L.dgrp_bgzf_bound(0, 1) == 28 and L.dgrp_bgzf_bound(0, 0) == 0
    assert L.dgrp_bgzf_bound(1, 0) == 32 and L.dgrp_bgzf_bound(BLOCK, 1) == BLOCK + 31 + 28
    assert L.dgrp_bgzf_bound(BLOCK + 1, 0) == BLOCK + 1 + 62
    assert L.dgrp_bgzf_workspace_bytes(0) >= 0 and L.dgrp_bgzf_workspace_bytes(BLOCK + 1) >= 2 * (BLOCK + 31)


P = 0x10000
I64 = lambda: C.pointer(C.c_int64())

ARG_CASES = [
    ("dgrp_bgzf_compress_host", lambda: (None, 10, P, 100, I64(), 1), EINVAL),
    ("dgrp_bgzf_compress_host", lambda: (P, 10, None, 100, I64(), 1), EINVAL),
    ("dgrp_bgzf_compress_host", lambda: (P, -1, P, 100, I64(), 1), EINVAL),
    ("dgrp_bgzf_compress_host", lambda: (P, 10, P, -1, I64(), 1), EINVAL),
    ("dgrp_bgzf_compress_host", lambda: (P, 10, P, 100, None, 1), EINVAL),
    ("dgrp_bgzf_compress_host", lambda: (None, 0, None, 100, I64(), 1), EINVAL),
    ("dgrp_bgzf_compress", lambda: (None, 10, P, 100, I64(), 1, P, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, None, 100, I64(), 1, P, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, P, 100, I64(), 1, None, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, -1, P, 100, I64(), 1, P, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, P, -1, I64(), 1, P, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, P, 100, I64(), 1, P, -1, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, P, 100, None, 1, P, 1 << 20, None), EINVAL),
    ("dgrp_bgzf_compress", lambda: (P, 10, P, 100, I64(), 1, P, 8, None), ENOMEM),
    ("dgrp_bgzf_compress", lambda: (None, 0, P, 27, I64(), 1, None, 0, None), ENOMEM),
]


@pytest.mark.parametrize("k", range(len(ARG_CASES)))
def test_argument_checks(k):
    from deepgrp_amd._lib import lib
    name, args, code = ARG_CASES[k]
    assert getattr(lib(), name)(*args()) == code
    assert name.encode() in lib().dgrp_last_error()


def test_nothing_to_do_is_a_no_op():
    from deepgrp_amd._lib import lib
    got = C.c_int64(7)
    assert lib().dgrp_bgzf_compress_host(None, 0, None, 0, C.byref(got), 0) == 0 and got.value == 0
    got = C.c_int64(7)
    assert lib().dgrp_bgzf_compress(None, 0, None, 0, C.byref(got), 0, None, 0, None) == 0 and got.value == 0


@pytest.mark.parametrize("name", ["len_block_plus_1", "random", "empty"])
def test_host_capacity_one_byte_short(name):
    from deepgrp_amd._lib import lib
    L = lib()
    data = CORPUS[name][:3 * BLOCK]
    want = compress_host(data, True)
    cap = len(want) - 1
    buf = (C.c_uint8 * (cap + 64))(*([0xA5] * (cap + 64)))
    got = C.c_int64(-1)
    assert L.dgrp_bgzf_compress_host(data, len(data), buf, cap, C.byref(got), 1) == ENOMEM
    assert got.value == len(want)                                    # the capacity it needs
    assert bytes(buf[cap:]) == b"\xa5" * 64                           # nothing behind the capacity
    assert b"dgrp_bgzf_compress_host" in L.dgrp_last_error()
    got = C.c_int64(-1)
    assert L.dgrp_bgzf_compress_host(data, len(data), buf, cap + 1, C.byref(got), 1) == 0
    assert bytes(buf[:cap + 1]) == want and bytes(buf[cap + 1:]) == b"\xa5" * 63


# ---------------------------------------------------------------- the command line, before any device work
def _args(argv):
    from deepgrp_amd.__main__ import CommandLineParser
    return CommandLineParser().parse_args(argv).args


def test_mask_gzip_parses_in_both_forms():
    a = _args(["--mask_dir", "out", "--mask_gzip", "m.h5", "x.fa"])               # README form, the flags in front
    assert (a.command, a.mask_dir, a.mask_gzip, a.model, a.FASTA) == ("predict", "out", True, "m.h5", ["x.fa"])
    a = _args(["--mask_gzip", "--mask_dir", "out", "-b", "7", "m.h5", "x.fa.gz", "y.fa"])
    assert (a.command, a.mask_gzip, a.model, a.FASTA) == ("predict", True, "m.h5", ["x.fa.gz", "y.fa"])
    a = _args(["predict", "m.h5", "x.fa", "--mask_dir", "d", "--mask_gzip", "--mask", "hard"])
    assert (a.mask_dir, a.mask_gzip, a.mask) == ("d", True, "hard")
    a = _args(["predict", "m.h5", "x.fa", "--mask_dir", "d"])
    assert not getattr(a, "mask_gzip", False)


@pytest.fixture
def no_gpu(monkeypatch):
    """Any attempt to reach the device or to load the model fails the test."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import pipeline

    def touched(*_a, **_k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(pipeline, "require_gpu", touched)
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))


def _refused(argv, *matches):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    for m in matches:
        assert m in str(e.value.code)


def test_mask_gzip_refusals_before_any_device_work(tmp_path, monkeypatch, no_gpu):
    from deepgrp_amd import gz
    data = CORPUS["len_block_plus_1"][:5000]
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\n" + data.replace(b"\n", b"") + b"\n")
    fz = tmp_path / "a.fa.gz"
    fz.write_bytes(gz.bgzf_compress(fa.read_bytes()))
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    out, mdir = str(tmp_path / "o.tsv"), str(tmp_path / "masked")
    _refused(["predict", model, str(fa), "--mask_gzip", "--output", out], "need --mask_dir")
    _refused(["--mask_gzip", model, str(fa), "--output", out], "need --mask_dir")
    # a.fa and a.fa.gz would both become masked/a.fa.gz
    _refused(["predict", model, str(fa), str(fz), "--mask_dir", mdir, "--mask_gzip", "--output", out], "same file name", "a.fa.gz")
    # the compressed copy would land on the compressed input
    _refused(["predict", model, str(fz), "--mask_dir", str(tmp_path), "--mask_gzip", "--output", out], "overwrite the input")
    # ... or the copy of a.fa on its neighbour a.fa.gz, which is an input too
    _refused(["predict", model, str(fz), str(fa), "--mask_dir", str(tmp_path), "--mask_gzip", "--output", out], "a.fa.gz")
    # without the flag a compressed input is still refused, and told about it
    _refused(["predict", model, str(fz), "--mask_dir", mdir, "--output", out], "--mask_dir", "gzip", "--mask_gzip")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(["predict", model, str(fa), "--mask_dir", mdir, "--mask_gzip", "--output", out], "--mask_gzip", "WORLD_SIZE")
    monkeypatch.setenv("WORLD_SIZE", "1")
    _refused(["predict", model, str(fa), "--mask_dir", mdir, "--mask_gzip", "--split_contigs", "--output", out], "--mask_gzip", "--split_contigs")
    assert not os.path.exists(mdir) and not os.path.exists(out)


def test_mask_fasta_refuses_ranges_of_a_compressed_copy(tmp_path, no_gpu):
    import numpy as np

    from deepgrp_amd import gz
    from deepgrp_amd.masking import mask_fasta
    from deepgrp_amd.pipeline import SEGMENT_DTYPE
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGT\n")
    rows = np.zeros(0, SEGMENT_DTYPE)
    with pytest.raises(ValueError, match="byte ranges"):
        mask_fasta(str(fa), str(tmp_path / "o.gz"), rows, ranges=[(0, 8)], compress=True)
    # an empty input needs no device: the compressed copy is the EOF member alone
    empty = tmp_path / "e.fa"
    empty.write_bytes(b"")
    assert mask_fasta(str(empty), str(tmp_path / "e.gz"), rows, compress=True) == 0
    assert (tmp_path / "e.gz").read_bytes() == gz.BGZF_EOF
