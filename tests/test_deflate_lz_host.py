"""The BGZF encoder's second level (deflate.h: matches inside the member) on the host, where it is defined: level 0 through the new
entries is the old encoder, level 1 is a valid BGZF file on every text (deflate_corpus.check_file: zlib and the library's own inflate,
the stream ending exactly at the trailer, the n + 31 bound) and never a larger member than level 0's, its sizes against zlib level 1
on the same member cut, the new entries' argument checks, and the command line's --track_gzip / --gzip_level before any device work."""
import ctypes as C
import os

import pytest

from conftest import GOLDEN
from deflate_corpus import BLOCK, EINVAL, ENOMEM, check_file, compress_host, corpus
from deflate_lz_corpus import BEDGRAPH, all_texts, compress_host_level, member_sizes

TEXTS = all_texts()

# level 1 / zlib level 1 (gz.bgzf_compress(data, level=1): the same members) in bytes, as measured on the host entry (both encoders
# are deterministic); the test allows 0.02 more, for code-length ties and header differences.  The bedGraph texts must be at most
# 1.00: the candidate rule exists for them.  The FASTA texts are reported.
RATIO_VS_ZLIB1 = {"bedgraph_d2_bin1": 0.9216, "bedgraph_d2_bin50": 0.8407, "bedgraph_d3_bin1_long_name": 0.8373,
                  "bedgraph_d3_bin50_long_name": 0.8077, "unmasked": 0.9139, "soft": 0.9414, "hard": 0.9434, "records_10k": 0.9419}


def test_level_0_through_the_new_entry_is_the_old_encoder():
    for name, data in corpus().items():
        for eof in (True, False):
            assert compress_host_level(data, eof, 0) == compress_host(data, eof), (name, eof)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_level_1_is_a_bgzf_file_and_no_member_is_larger_than_at_level_0(name):
    data = TEXTS[name]
    for eof in (True, False):
        out = compress_host_level(data, eof, 1)
        check_file(out, data, eof)
    lz, lit = member_sizes(compress_host_level(data, True, 1)), member_sizes(compress_host_level(data, True, 0))
    assert lz.size == lit.size and (lz <= lit).all()


def test_python_entry_passes_the_level_on():
    from deepgrp_amd import gz
    data = TEXTS["bedgraph_d2_bin1"]
    assert gz.bgzf_compress_host(data) == compress_host(data) == gz.bgzf_compress_host(data, level=0)
    assert gz.bgzf_compress_host(data, eof=False, level=1) == compress_host_level(data, False, 1)


def test_n_run_is_below_a_tenth_of_level_0():
    # an overlapping distance-1 match of 258 bytes costs under 3 bytes of any code; level 0 spends at least 1 bit per byte
    data = TEXTS["n_run"]
    assert len(compress_host_level(data, True, 1)) * 10 < len(compress_host_level(data, True, 0))


def test_window_and_member_edges_are_used_as_far_as_they_reach():
    from deepgrp_amd import gz
    # 2000 bytes of 64 values are 1500 bytes of literals and a few dozen as eight matches: the stretch 32 768 back is saved, the one
    # 32 769 back is not (both: above 2700)
    lz, lit = (len(compress_host_level(TEXTS["window_edge"], False, lv)) for lv in (1, 0))
    print(f"window_edge: level 0 {lit}, level 1 {lz}")
    assert 1200 <= lit - lz <= 1600
    lz, lit = (member_sizes(compress_host_level(TEXTS["match_ends_the_member"], False, lv))[0] for lv in (1, 0))
    print(f"match_ends_the_member: level 0 {lit}, level 1 {lz}")
    assert 1200 <= lit - lz <= 1600
    # the copy of the previous member's tail is out of reach: the second member is what it is on its own
    data = TEXTS["source_in_previous_member"]
    whole = compress_host_level(data, False, 1)
    assert whole[int(gz.walk_members(whole).start[1]):] == compress_host_level(data[BLOCK:], False, 1)
    alone, lit = (len(compress_host_level(data[BLOCK:], False, lv)) for lv in (1, 0))
    assert lit - alone < 400                                          # (2000 bytes from the other member would save 1400)


@pytest.mark.parametrize("name", sorted(RATIO_VS_ZLIB1))
def test_size_against_zlib_level_1(name):
    from deepgrp_amd import gz
    data = TEXTS[name]
    ours, ref = len(compress_host_level(data, True, 1)), len(gz.bgzf_compress(data, level=1))
    print(f"{name}: level 1 {ours} bytes, zlib level 1 {ref} bytes, ratio {ours / ref:.4f}, input {len(data)}")
    assert ours / ref <= RATIO_VS_ZLIB1[name] + 0.02
    if name in BEDGRAPH:
        assert RATIO_VS_ZLIB1[name] <= 1.00


# ---------------------------------------------------------------- arguments
def _buf(n):
    return (C.c_uint8 * n)()


ARG_CASES = [
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", -1, _buf(64), 64, C.byref(C.c_int64()), 1, 1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, _buf(64), -1, C.byref(C.c_int64()), 1, 1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, _buf(64), 64, None, 1, 1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (None, 3, _buf(64), 64, C.byref(C.c_int64()), 1, 1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, None, 64, C.byref(C.c_int64()), 1, 1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, _buf(64), 64, C.byref(C.c_int64()), 1, 2), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, _buf(64), 64, C.byref(C.c_int64()), 1, -1), EINVAL),
    ("dgrp_bgzf_compress_host_level", lambda: (b"abc", 3, _buf(64), 10, C.byref(C.c_int64()), 1, 1), ENOMEM),
    # the device entry refuses these before it touches the device
    ("dgrp_bgzf_compress_level", lambda: (None, -1, None, 0, C.byref(C.c_int64()), 1, 1, None, 0, None), EINVAL),
    ("dgrp_bgzf_compress_level", lambda: (None, 0, None, 0, None, 1, 1, None, 0, None), EINVAL),
    ("dgrp_bgzf_compress_level", lambda: (None, 3, None, 64, C.byref(C.c_int64()), 1, 1, None, 0, None), EINVAL),
    ("dgrp_bgzf_compress_level", lambda: (None, 0, None, 64, C.byref(C.c_int64()), 1, 1, None, 0, None), EINVAL),
    ("dgrp_bgzf_compress_level", lambda: (None, 0, None, 0, C.byref(C.c_int64()), 0, 2, None, 0, None), EINVAL),
    ("dgrp_bgzf_compress_level", lambda: (None, 0, None, 0, C.byref(C.c_int64()), 1, 1, None, 0, None), ENOMEM),
]


@pytest.mark.parametrize("k", range(len(ARG_CASES)))
def test_argument_checks(k):
    from deepgrp_amd._lib import lib
    name, args, code = ARG_CASES[k]
    assert getattr(lib(), name)(*args()) == code
    assert name.encode() in lib().dgrp_last_error()


def test_workspace_and_nothing_to_do():
    from deepgrp_amd._lib import lib
    L = lib()
    for n in (0, 1, BLOCK, BLOCK + 1, 10 * BLOCK + 5):
        nmem = (n + BLOCK - 1) // BLOCK
        assert L.dgrp_bgzf_workspace_bytes_level(n, 0) == L.dgrp_bgzf_workspace_bytes(n)
        assert L.dgrp_bgzf_workspace_bytes_level(n, 1) == L.dgrp_bgzf_workspace_bytes(n) + nmem * BLOCK * 4
    assert L.dgrp_bgzf_workspace_bytes_level(-1, 1) == 0 == L.dgrp_bgzf_workspace_bytes_level(5, 2)
    got = C.c_int64(7)
    assert L.dgrp_bgzf_compress_host_level(None, 0, None, 0, C.byref(got), 0, 1) == 0 and got.value == 0
    got = C.c_int64(7)
    assert L.dgrp_bgzf_compress_level(None, 0, None, 0, C.byref(got), 0, 1, None, 0, None) == 0 and got.value == 0


def test_host_capacity_one_byte_short():
    from deepgrp_amd._lib import lib
    L = lib()
    data = TEXTS["bedgraph_d2_bin1"][:3 * BLOCK]
    want = compress_host_level(data, True, 1)
    cap = len(want) - 1
    buf = (C.c_uint8 * (cap + 64))(*([0xA5] * (cap + 64)))
    got = C.c_int64(-1)
    assert L.dgrp_bgzf_compress_host_level(data, len(data), buf, cap, C.byref(got), 1, 1) == ENOMEM
    assert got.value == len(want) and bytes(buf[cap:]) == b"\xa5" * 64
    assert L.dgrp_bgzf_compress_host_level(data, len(data), buf, cap + 1, C.byref(got), 1, 1) == 0
    assert bytes(buf[:cap + 1]) == want and bytes(buf[cap + 1:]) == b"\xa5" * 63


# ---------------------------------------------------------------- the command line, before any device work
def _args(argv):
    from deepgrp_amd.__main__ import CommandLineParser
    return CommandLineParser().parse_args(argv).args


def test_track_gzip_and_gzip_level_parse_in_both_forms():
    a = _args(["--track_dir", "out", "--track_gzip", "--gzip_level", "0", "m.h5", "x.fa"])         # README form, the flags in front
    assert (a.command, a.track_dir, a.track_gzip, a.gzip_level, a.model, a.FASTA) == ("predict", "out", True, 0, "m.h5", ["x.fa"])
    a = _args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_gzip"])
    assert a.track_gzip and getattr(a, "gzip_level", None) is None
    a = _args(["predict", "m.h5", "x.fa", "--mask_dir", "d", "--mask_gzip", "--gzip_level", "1"])
    assert (a.mask_gzip, a.gzip_level) == (True, 1)
    a = _args(["predict", "m.h5", "x.fa", "--track_dir", "d"])
    assert not getattr(a, "track_gzip", False)


def test_plan_defaults():
    from deepgrp_amd import tracks
    level = lambda argv: tracks.plan(_args(["predict", "m.h5", "x.fa"] + argv)).gzip_level
    assert level(["--track_dir", "d"]) is None                        # plain bedGraph, as before
    assert level(["--track_dir", "d", "--track_gzip"]) == 1
    assert level(["--track_dir", "d", "--track_gzip", "--gzip_level", "0"]) == 0
    assert level(["--track_dir", "d", "--mask_dir", "m", "--mask_gzip", "--gzip_level", "1"]) is None
    spec = tracks.resolve(tracks.plan(_args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_gzip"])), 5)
    assert spec.gzip_level == 1 and spec.classes == (1, 2, 3, 4)
    assert tracks.track_path("d", "x.fa", 3, True) == os.path.join("d", "x.fa.class3.bedGraph.gz")
    assert tracks.track_path("d", "x.fa", 3) == os.path.join("d", "x.fa.class3.bedGraph")


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


def test_refusals_before_any_device_work(tmp_path, monkeypatch, no_gpu):
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGTACGTACGT\n")
    ann = tmp_path / "a.bed"
    ann.write_text("r\t0\t4\t1\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    out, tdir, mdir = str(tmp_path / "o.tsv"), str(tmp_path / "tracks"), str(tmp_path / "masked")
    _refused(["predict", model, str(fa), "--track_gzip", "--output", out], "--track_gzip needs --track_dir")
    _refused(["--track_gzip", model, str(fa), "--output", out], "--track_gzip needs --track_dir")
    _refused(["predict", model, str(fa), "--gzip_level", "1", "--output", out], "--gzip_level needs --mask_gzip or --track_gzip")
    _refused(["predict", model, str(fa), "--track_dir", tdir, "--gzip_level", "1", "--output", out], "--gzip_level needs")
    _refused(["predict", model, str(fa), "--mask_dir", mdir, "--gzip_level", "0", "--output", out], "--gzip_level needs")
    _refused(["predict", model, str(fa), "--track_dir", tdir, "--track_gzip", "--gzip_level", "2", "--output", out], "--gzip_level must be 0", "2")
    _refused(["predict", model, str(fa), "--mask_dir", mdir, "--mask_gzip", "--gzip_level", "-1", "--output", out], "--gzip_level must be 0")
    _refused(["--track_gzip", "evaluate", model, str(ann), str(fa), "--output", out], "belongs to predict")
    _refused(["--gzip_level", "1", "evaluate", model, str(ann), str(fa), "--output", out], "belongs to predict")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(["predict", model, str(fa), "--track_dir", tdir, "--track_gzip", "--output", out], "--track_dir", "WORLD_SIZE")
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not os.path.exists(tdir) and not os.path.exists(mdir) and not os.path.exists(out)


def test_mask_fasta_refuses_a_level_it_does_not_have(tmp_path, no_gpu):
    import numpy as np

    from deepgrp_amd.masking import mask_fasta
    from deepgrp_amd.pipeline import SEGMENT_DTYPE
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGT\n")
    with pytest.raises(ValueError, match="level"):
        mask_fasta(str(fa), str(tmp_path / "o.gz"), np.zeros(0, SEGMENT_DTYPE), compress=True, level=2)
