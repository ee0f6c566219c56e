"""predict --bed_gff3 without a GPU: the two escapes on all 256 byte values; gff.reference_lines against hand-written lines; the new
entry points are declared, exported and bound, their workspace queries refuse what the entries refuse and the entries refuse bad
host arguments before any device work; every refusal of the command line is a SystemExit before the model is read or torch.cuda
is touched (the name count: right after the model is read); BedFiles in GFF3 form on fake writes (text from gff.reference_lines,
members from gz.bgzf_compress, index pieces from gff.reference_index_parts) writes the header, carries the line count from write
to write, writes the payload gff.reference_index gives for the finished file under the gff preset, warns once and leaves no `.tbi`
where the input cannot be indexed, leaves no `.gff3` for an empty record name, and leaves nothing behind on abort."""
import argparse
import logging
import os
import struct
import zlib

import numpy as np
import pytest

from deepgrp_amd import bed, gff, gz, tabix
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE

ONE = 1 << 24
EINVAL = -1


# ---- the statements ------------------------------------------------------------------------------------------------------------------
def test_escapes_on_every_byte():
    keep_seqid = set(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789.:^*$@!+_?-|")
    escaped_value = set(range(0x20)) | {0x7f} | set(b"%;=&,")
    assert len(keep_seqid) == 26 + 26 + 10 + 12
    for b in range(256):
        one = bytes([b])
        assert gff.escape_seqid(one) == (one if b in keep_seqid else b"%%%02X" % b), b
        assert gff.escape_value(one) == (b"%%%02X" % b if b in escaped_value else one), b
    assert gff.escape_seqid(b"scaf;x=1") == b"scaf%3Bx%3D1" and gff.escape_seqid("chr\udcff 1") == b"chr%FF%201"
    assert gff.escape_value(b"SINE/Alu (x),y\xff") == b"SINE/Alu (x)%2Cy\xff" and gff.escape_seqid(b"") == b"" == gff.escape_value(b"")
    every = bytes(range(256))
    assert len(gff.escape_seqid(every)) == 74 + 3 * (256 - 74) and len(gff.escape_value(every)) == 256 + 2 * 38


def _rows(spans):
    rows = np.zeros(len(spans), SEGMENT_DTYPE)
    for i, r in enumerate(spans):
        rows[i] = r
    return rows


def _sc(vals):
    sc = np.zeros(len(vals), ROW_SCORE_DTYPE)
    for i, (s, b, g, m) in enumerate(vals):
        sc[i] = (s, b, g, m, 0)
    return sc


EXAMPLE_ROWS = [(99, 350, 3, 0), (1000, 1010, 1, 0), (0, 5, 4, 1)]
EXAMPLE_SCORES = [(int(0.93 * ONE) * 251, 251, 240, int(0.41 * ONE)), (ONE * 10, 10, 10, ONE), (int(0.5004 * ONE) * 5, 5, 3, ONE // 2)]
EXAMPLE = (b"chr1\tdeepgrp\trepeat_region\t100\t350\t0.9300\t.\t.\tID=r9;Name=SINE/Alu;label=3;score=930;min=0.4100;agree=0.9562\n"
           b"chr1\tdeepgrp\trepeat_region\t1001\t1010\t1.0000\t.\t.\tID=r10;Name=HSATII;label=1;score=1000;min=1.0000;agree=1.0000\n"
           b"scaf%3Bx%3D1\tdeepgrp\trepeat_region\t1\t5\t0.5004\t.\t.\tID=r11;Name=class4;label=4;score=500;min=0.5000;agree=0.6000\n")


def test_reference_lines_against_hand_written_lines():
    rows, sc = _rows(EXAMPLE_ROWS), _sc(EXAMPLE_SCORES)
    names = [b"chr1", "scaf;x=1"]
    text, lines = gff.reference_lines(names, True, rows, sc, 0, [b"HSATII", b"x", b"SINE/Alu", b"class4"], 8)
    assert (text, lines) == (EXAMPLE, 3)
    text, lines = gff.reference_lines(names, True, rows, sc, 0, None, 8)
    assert lines == 3 and text == EXAMPLE.replace(b"SINE/Alu", b"class3").replace(b"HSATII", b"class1")
    # --bed_min_score: the filtered row does not count in the ordinals; without by_contig every row has name 0
    text, lines = gff.reference_lines(names, False, rows, sc, 931, None, 0)
    assert (text, lines) == (b"chr1\tdeepgrp\trepeat_region\t1001\t1010\t1.0000\t.\t.\tID=r1;Name=class1;label=1;score=1000;min=1.0000;agree=1.0000\n", 1)
    text, lines = gff.reference_lines(names, True, rows, sc, 501, [b"a;b", b"x", b"c=d,e", b"f"], 99)
    assert lines == 2 and b"ID=r100;Name=c%3Dd%2Ce;label=3;" in text and b"ID=r101;Name=a%3Bb;label=1;" in text
    assert gff.reference_lines(names, True, rows[:0], sc[:0]) == (b"", 0)
    with pytest.raises(ValueError):
        gff.reference_lines(names, True, rows, sc, 0, [b"only", b"three", b"names"], 0)           # label 4 has no name
    with pytest.raises(ValueError):
        gff.reference_lines(names, True, rows, sc, 0, None, -1)
    assert gff.HEADER == b"##gff-version 3\n" and len(gff.HEADER) == 16


# ---- the library ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


NEW = ("dgrp_gff_text_workspace_bytes", "dgrp_gff_text_batch", "dgrp_gff_index_workspace_bytes", "dgrp_gff_index_batch")


def test_symbols_declared_exported_and_bound(L):
    from deepgrp_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "deepgrp_hip.h")).read()
    for name in NEW:
        assert name in _lib.exported_symbols() and hasattr(L, name) and name + "(" in header, name
        assert getattr(L, name).argtypes is not None


def test_workspace_queries_refuse_what_the_entries_refuse(L):
    text, index = L.dgrp_gff_text_workspace_bytes, L.dgrp_gff_index_workspace_bytes
    assert text(0, 1, 0, 0, 0) > 0 and text(5000, 3, 40, 4, 30) >= 5000 * 32 + 40 + 30 + 4 * 8 + 5 * 8
    assert text(5000, 3, 40, 4, 30) > L.dgrp_bed_text_workspace_bytes(5000, 3, 40)                 # the two columns of the ordinals
    for bad in ((-1, 1, 0, 0, 0), (10, 0, 0, 0, 0), (10, 1, -1, 0, 0), (1 << 31, 1, 0, 0, 0), (10, 1, 0, -1, 0), (10, 1, 0, 1, -1),
                (10, 1, 0, 1 << 31, 0)):
        assert text(*bad) == 0, bad
        assert index(*bad, 1) == 0, bad
    assert index(5000, 3, 40, 4, 30, 3) > text(5000, 3, 40, 4, 30)
    assert index(10, 1, 0, 0, 0, 0) == 0 and index(10, 1, 0, 0, 0, 1 << 31) == 0
    # the BED queries are what they were
    assert L.dgrp_bed_text_workspace_bytes(5000, 3, 40) == 256 + 256 + 2 * 40192 + 256
    assert L.dgrp_bed_index_workspace_bytes(5000, 3, 40, 3) == L.dgrp_gff_index_workspace_bytes(5000, 3, 40, 0, 0, 3)


def test_entries_refuse_bad_host_arguments_before_any_device_work(L):
    """NULL or descending tables, id0 below 0, NULL result pointers, a record end above 2^29, nrec > 1 without by_contig:
    DGRP_EINVAL from the host checks, with no device pointer ever read (they are NULL or made up here).  No rows: nothing to do."""
    import ctypes as C
    got, lines = C.c_int64(-7), C.c_int64(-7)
    off, coff = np.array([0, 3], np.int64), np.array([0, 2, 5], np.int64)
    bogus = 0xdead0000

    def text(names=b"abc", name_off=off, cnames=b"LTRxy", cname_off=coff, ncnames=2, nrows=0, id0=0, rows=None, h_bytes=True, h_lines=True):
        got.value = lines.value = -7
        return L.dgrp_gff_text_batch(names, name_off.ctypes.data, 1, 0, cnames, None if cname_off is None else cname_off.ctypes.data, ncnames,
                                     rows, rows, nrows, 0, id0, None, 0, C.byref(got) if h_bytes else None,
                                     C.byref(lines) if h_lines else None, None, 0, None)
    assert text() == 0 and (got.value, lines.value) == (0, 0)
    assert text(cnames=None, cname_off=None, ncnames=0) == 0 and (got.value, lines.value) == (0, 0)
    assert text(names=None) == EINVAL
    assert text(name_off=np.array([3, 0], np.int64)) == EINVAL and b"ascend" in L.dgrp_last_error()
    assert text(cname_off=np.array([0, 5, 2], np.int64)) == EINVAL and b"class-name offsets must ascend" in L.dgrp_last_error()
    assert text(cnames=None) == EINVAL and b"class names" in L.dgrp_last_error()
    assert text(cname_off=None) == EINVAL
    assert text(ncnames=-1) == EINVAL
    assert text(id0=-1) == EINVAL and b"id0" in L.dgrp_last_error()
    assert text(id0=-1, nrows=4, rows=bogus) == EINVAL and b"id0" in L.dgrp_last_error()           # before the rows are looked at
    assert text(h_bytes=False) == EINVAL and text(h_lines=False) == EINVAL
    assert text(nrows=-1) == EINVAL
    assert text(nrows=4) == EINVAL                                                                 # rows without arrays
    assert text(nrows=4, rows=bogus) != 0 and b"workspace" in L.dgrp_last_error()                   # made-up pointers are never read

    def index(ends, nrec=None, by_contig=1, nrows=0, id0=0, cname_off=coff, rows=None):
        e = np.array(ends, np.int64)
        got.value = -7
        return L.dgrp_gff_index_batch(b"abc", off.ctypes.data, 1, by_contig, b"LTRxy", None if cname_off is None else cname_off.ctypes.data,
                                      2, rows, rows, nrows, 0, id0, len(e) if nrec is None else nrec, e.ctypes.data, None, 0,
                                      C.byref(got), rows, 1 << 20, None, None, 0, None)
    assert index([1 << 29]) == 0 and got.value == 0
    assert index([(1 << 29) + 1]) == EINVAL and b"2^29" in L.dgrp_last_error()
    assert index([100, 0]) == EINVAL and b"record 1" in L.dgrp_last_error()
    assert index([100, 100], by_contig=0) == EINVAL and b"nrec must be 1" in L.dgrp_last_error()
    assert index([100], nrec=0) == EINVAL
    assert index([100], nrows=3) == EINVAL                                                         # rows without arrays
    assert index([100], id0=-1) == EINVAL and b"id0" in L.dgrp_last_error()
    assert index([100], cname_off=None) == EINVAL and b"class names" in L.dgrp_last_error()
    assert index([100], nrows=3, rows=bogus) != 0 and b"workspace" in L.dgrp_last_error()


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    import torch

    def touched(*_a, **_k):
        raise AssertionError("torch.cuda was touched before the refusal")
    for name in ("is_available", "set_device", "current_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


@pytest.fixture
def no_model(monkeypatch):
    """The model reader fails: a refusal that must come first is a SystemExit, not this error."""
    from deepgrp_amd import model as dgmodel

    def read(*_a, **_k):
        raise AssertionError("the model was read before the refusal")
    monkeypatch.setattr(dgmodel, "load_model", read)
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", read)


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_cli_refusals(no_gpu, no_model, tmp_path, monkeypatch):
    model = str(tmp_path / "no_such_model.h5")
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    out = str(tmp_path / "beds")
    base = ["predict", model, str(fa)]
    _refused(base + ["--bed_gff3"], "--bed_gff3 needs --bed_dir")
    _refused(["--bed_gff3", model, str(fa)], "--bed_gff3 needs --bed_dir")                          # the README form
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_bigbed"], "--bed_gff3 and --bed_bigbed")
    _refused(base + ["--bed_dir", out, "--bed_names", "a,b"], "--bed_names needs --bed_gff3")
    _refused(base + ["--bed_names", "a,b"], "--bed_names needs --bed_gff3")
    _refused(["--bed_names", "a,b", "--bed_dir", out, model, str(fa)], "--bed_names needs --bed_gff3")      # the README form: it takes a value
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_names", "a,,b"], "the name of label 2 is empty")
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_names", ""], "the name of label 1 is empty")
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_names", "a," + "b" * 256], "the name of label 2 has 256 bytes, above 255")
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_index"], "--bed_index needs --bed_gzip")
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--bed_min_score", "1001"], "--bed_min_score must lie in 0..1000")
    _refused(base + ["--bed_dir", out, "--bed_gff3", "--split_contigs"], "--bed_dir runs in one process")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(base + ["--bed_dir", out, "--bed_gff3"], "--bed_dir runs in one process")
    monkeypatch.delenv("WORLD_SIZE")
    (tmp_path / "sub").mkdir()
    twin = tmp_path / "sub" / "a.fa"
    twin.write_text(">r\nACGT\n")
    _refused(["predict", model, str(fa), str(twin), "--bed_dir", out, "--bed_gff3"], "have the same file name a.fa.gff3; they would collide")
    _refused(["predict", model, str(fa), str(twin), "--bed_dir", out, "--bed_gff3", "--bed_gzip"], "have the same file name a.fa.gff3.gz;")
    gzdir = tmp_path / "in"
    gzdir.mkdir()
    link = gzdir / "l.fa"                                                             # (the suffix is appended: reached through a link)
    os.symlink(gzdir / "l.fa.gff3", link)
    (gzdir / "l.fa.gff3").write_bytes(b">r\nACGT\n")
    _refused(["predict", model, str(link), "--bed_dir", str(gzdir), "--bed_gff3"], "would overwrite the input")
    _refused(["--bed_gff3", "--bed_dir", out, "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--bed_gff3 belongs to predict")
    _refused(["--bed_names", "a", "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--bed_names belongs to predict")
    assert not os.path.exists(out)                                                   # no refusal left a directory behind


def test_the_name_count_is_checked_behind_the_model(monkeypatch, tmp_path):
    """classes - 1 names: refused right after the model file is read (once, on the host), before the device model is made and
    before a record is read, with both numbers in the message."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import CommandLineParser

    read = []
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", lambda *a, **k: read.append(1) or {"ff_kernel": np.zeros((16, 5), np.float32)})

    def no_device(*_a, **_k):
        raise AssertionError("the device model was made before the refusal")
    monkeypatch.setattr(dgmodel, "device_model", no_device)
    monkeypatch.setattr(dgmodel, "load_model", no_device)

    def no_pipeline(*_a, **_k):
        raise AssertionError("the pipeline was built before the refusal")
    monkeypatch.setattr(CommandLineParser, "_pipeline", staticmethod(no_pipeline))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    _refused(["predict", "m.h5", str(fa), "--bed_dir", str(tmp_path / "o"), "--bed_gff3", "--bed_names", "a,b,c"], "gives 3 names")
    _refused(["predict", "m.h5", str(fa), "--bed_dir", str(tmp_path / "o"), "--bed_gff3", "--bed_names", "a,b,c,d,e"], "has 4 repeat classes")
    assert len(read) == 2


def test_plan(tmp_path):
    d = str(tmp_path / "out")
    ns = lambda **k: argparse.Namespace(bed_dir=d, FASTA=["-", str(tmp_path / "x.fa")], **k)
    p = bed.plan(ns(bed_gff3=True))
    assert (p.gff3, p.gzip_level, p.index, p.class_names, p.on_device) == (True, None, False, None, True)
    assert [os.path.basename(v) for v in p.paths.values()] == ["stdin.gff3", "x.fa.gff3"]
    p = bed.plan(ns(bed_gff3=True, bed_gzip=True, bed_index=True, gzip_level=0, bed_min_score=5, bed_names="LTR,SINE/Alu,a;b"))
    assert (p.gff3, p.gzip_level, p.index, p.min_score, p.class_names) == (True, 0, True, 5, (b"LTR", b"SINE/Alu", b"a;b"))
    assert [os.path.basename(v) for v in p.paths.values()] == ["stdin.gff3.gz", "x.fa.gff3.gz"]
    p = bed.plan(ns())                                                                # today's plans are what they were
    assert (p.gff3, p.class_names, p.on_device, os.path.basename(p.paths["-"])) == (False, None, False, "stdin.bed")
    assert bed.plan(ns(bed_gzip=True)).on_device and bed.BedPlan(d, 0, {}).gff3 is False
    assert bed.bed_path(d, "x.fa") == os.path.join(d, "x.fa.bed") and bed.bed_path(d, "x.fa", True, False, True) == os.path.join(d, "x.fa.gff3.gz")


# ---- BedFiles on fake writes ---------------------------------------------------------------------------------------------------------
def _spans(spans, contigs=None):
    rows = np.zeros(len(spans), SEGMENT_DTYPE)
    for i, (a, b) in enumerate(spans):
        rows[i] = (a, b, 1 + i % 4, 0 if contigs is None else contigs[i])
    return rows


def _scores(n, seed=5, low=()):
    rng = np.random.default_rng(seed)
    sc = np.zeros(n, ROW_SCORE_DTYPE)
    sc["bases"] = rng.integers(1, 5000, n)
    sc["sum"] = [int(b) * int(rng.integers(ONE // 2, ONE + 1)) for b in sc["bases"]]
    sc["agree"] = [int(rng.integers(0, b + 1)) for b in sc["bases"]]
    sc["qmin"] = rng.integers(0, ONE // 2, n)
    for i in low:
        sc["sum"][i] = 0
    return sc


def _fake_write(p, names, by_contig, rows, scores, rec_end, refused=None, texts=None):
    """A gff.GffWrite whose render states the write with gff.py's own statements; `texts` collects what it rendered."""
    raw = [nm if isinstance(nm, bytes) else nm.encode() for nm in names]

    def render(id0):
        text, lines = gff.reference_lines(names, by_contig, rows, scores, p.min_score, p.class_names, id0)
        if texts is not None:
            texts.append((id0, text))
        if p.gzip_level is None:
            return gff.GffText(text, lines)
        members = gz.bgzf_compress(text, eof=False) if text else b""
        if refused is not None or not text or not p.index:
            return gff.GffText(members, lines)
        return gff.GffText(members, lines, *gff.reference_index_parts(names, by_contig, rows, scores, p.min_score, rec_end, p.class_names, id0))
    return gff.GffWrite(raw, refused, render if len(rows) else None)


def _plan(tmp_path, gzip=True, index=True, names=None):
    final = str(tmp_path / "out" / ("in.fa.gff3" + (".gz" if gzip else "")))
    return bed.BedPlan(str(tmp_path / "out"), 500, {"in.fa": final}, 1 if gzip else None, index and gzip, False, True, names)


def _inflate(data):
    out, off = [], 0
    while off < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[off:]))
        off = len(data) - len(d.unused_data)
    return b"".join(out)


@pytest.mark.parametrize("gzip", [False, True])
def test_the_header_only_file(tmp_path, gzip):
    p = _plan(tmp_path, gzip)
    files = bed.BedFiles(p, "in.fa")
    files.write([b"r"], False, None, gff.GffWrite([b"r"]))                            # a record without a row
    files.commit()
    data = open(p.paths["in.fa"], "rb").read()
    if not gzip:
        assert data == gff.HEADER and os.listdir(p.directory) == ["in.fa.gff3"]
        return
    assert data == gff.header_member(1) + gz.BGZF_EOF and _inflate(data) == gff.HEADER
    assert sorted(os.listdir(p.directory)) == ["in.fa.gff3.gz", "in.fa.gff3.gz.tbi"]
    tbi = _inflate(open(p.paths["in.fa"] + ".tbi", "rb").read())
    assert tbi == gff.reference_index(data) == tabix.payload([], [], [], gff.PRESET)
    assert struct.unpack_from("<8i", tbi, 4) == (0, 0, 1, 4, 5, ord("#"), 0, 0)


def _three_writes(p, texts):
    """A long record of nested and wide lines on its own (several members), a batch of four records of which two consecutive ones
    share a name and one has no emitted line, and a write whose every line is filtered."""
    rng = np.random.default_rng(8)
    starts = np.sort(rng.integers(0, 40_000_000, 3000))
    spans = [(int(s), int(s) + int(w)) for s, w in zip(starts, rng.integers(1, 40_000, 3000))]
    spans[10] = (spans[10][0], 45_000_000)                                            # covers 2 700 windows; its successors are nested
    spans[-1] = (spans[-1][0], spans[-1][0] + 5)                                      # the last line ends far below the longest
    w1 = _fake_write(p, [b"chr A"], False, _spans(spans), _scores(3000, low=(0, 1, 50, 51)), [1 << 29], texts=texts)
    contigs = [0, 0, 1, 1, 1, 3, 3]
    rows2 = _spans([(5, 90), (20_000, 20_010), (0, 16_384), (16_383, 16_385), (16_385, 140_000), (7, 9), (8, 200_000)], contigs)
    w2 = _fake_write(p, [b"b1", b"twin", b"twin", b"tail"], True, rows2, _scores(7, seed=2, low=(2,)), [100_000, 200_000, 300_000, 200_000],
                     texts=texts)
    w3 = _fake_write(p, [b"tail"], False, _spans([(1, 2), (3, 4)]), _scores(2, low=(0, 1)), [50], texts=texts)
    w4 = _fake_write(p, [b"tail"], False, _spans([(10, 20), (30, 40)]), _scores(2), [50], texts=texts)
    return [w1, w2, w3, w4], spans


@pytest.mark.parametrize("gzip", [False, True])
def test_bedfiles_counts_the_lines_and_writes_the_reference_index(tmp_path, caplog, gzip):
    p = _plan(tmp_path, gzip, names=(b"LTR", b"SINE/Alu", b"a;b", b"D"))
    files = bed.BedFiles(p, "in.fa")
    texts = []
    writes, spans = _three_writes(p, texts)
    for w in writes:
        files.write(w.names, len(w.names) > 1, None, w)
    assert [t[0] for t in texts] == [0, 2996, 3002, 3002] and files.lines == 3004     # the line count travels from write to write
    assert p.paths["in.fa"] not in [os.path.join(p.directory, f) for f in os.listdir(p.directory)]      # still temporary
    with caplog.at_level(logging.WARNING):
        files.commit()
    assert not caplog.records
    want = gff.HEADER + b"".join(t for _i, t in texts)
    data = open(p.paths["in.fa"], "rb").read()
    if not gzip:
        assert data == want and os.listdir(p.directory) == ["in.fa.gff3"]
    else:
        assert sorted(os.listdir(p.directory)) == ["in.fa.gff3.gz", "in.fa.gff3.gz.tbi"]
        assert data.endswith(gz.BGZF_EOF) and _inflate(data) == want and data.startswith(gff.header_member(1))
    lines = want.split(b"\n")[1:-1]
    assert [ln.split(b"ID=r")[1].split(b";")[0] for ln in lines] == [b"%d" % j for j in range(1, 3005)]
    assert b";Name=a%3Bb;label=3;" in want and lines[0].startswith(b"chr%20A\tdeepgrp\trepeat_region\t")
    if not gzip:
        return
    payload = gff.reference_index(data)
    assert _inflate(open(p.paths["in.fa"] + ".tbi", "rb").read()) == payload
    assert struct.unpack_from("<7i", payload, 4) == (4, 0, 1, 4, 5, ord("#"), 0)
    with pytest.raises(ValueError, match="bed preset"):
        tabix.read_index(payload)                                                     # today's reader takes today's preset
    ix = gff.read_index(payload)
    assert ix["names"] == [b"chr%20A", b"b1", b"twin", b"tail"]
    assert min(c[0] for c in ix["bins"][0][min(ix["bins"][0], key=lambda b: ix["bins"][0][b][0][0])]) >> 16 == len(gff.header_member(1))
    assert len(ix["linear"][0]) == ((spans[-1][1] - 1) >> 14) + 1 < ((spans[10][1] - 1) >> 14) + 1     # the last line ends the sequence
    cols = [ln.split(b"\t") for ln in lines]
    for name, beg, end in ((b"chr%20A", 0, 1 << 29), (b"chr%20A", 35_000_000, 35_000_001), (b"twin", 16_384, 16_385), (b"tail", 0, 8),
                           (b"tail", 10, 11), (b"b1", 90, 20_000), (b"nobody", 0, 100)):
        scan = [b"\t".join(f) for f in cols if f[0] == name and int(f[3]) - 1 < end and int(f[4]) > beg]
        assert gff.query(ix, data, name, beg, end) == scan, (name, beg, end)


@pytest.mark.parametrize("case", ["above 2^29", "name reappears", "name reappears in a later write", "a write without its index"])
def test_an_input_without_an_index(tmp_path, caplog, case):
    """One warning, no `.tbi` (a stale one is removed), the `.gff3.gz` as it is without the flag."""
    p = _plan(tmp_path)
    os.makedirs(p.directory)
    stale = p.paths["in.fa"] + ".tbi"
    open(stale, "wb").write(b"left by an earlier run")
    files = bed.BedFiles(p, "in.fa")
    rows, sc = _spans([(5, 90), (100, 200), (300, 400)], [0, 1, 2]), _scores(3)
    ends, texts = [1000, 1000, 1000], []
    fw = lambda names, by_contig, rows, sc, ends, **k: _fake_write(p, names, by_contig, rows, sc, ends, texts=texts, **k)
    if case == "above 2^29":
        writes = [fw([b"a", b"b", b"c"], True, rows, sc, ends, refused="record 'b' ends at 536870913, above 2^29"), fw([b"d"], False, rows, sc, [1000])]
    elif case == "name reappears":
        writes = [fw([b"a", b"b", b"a"], True, rows, sc, ends), fw([b"d"], False, rows, sc, [1000])]
    elif case == "a write without its index":
        writes = [fw([b"a", b"b", b"c"], True, rows, sc, ends, refused="(not said to BedFiles)")._replace(refused=None)]
    else:
        writes = [fw([b"a", b"b", b"c"], True, rows, sc, ends), fw([b"c"], False, rows, sc, [1000]), fw([b"b"], False, rows, sc, [1000])]
    with caplog.at_level(logging.WARNING):
        for w in writes:
            files.write(w.names, len(w.names) > 1, None, w)
        files.commit()
    assert len(caplog.records) == 1 and "no tabix index is written (--bed_index)" in caplog.records[0].getMessage()
    assert os.listdir(p.directory) == ["in.fa.gff3.gz"]
    assert _inflate(open(p.paths["in.fa"], "rb").read()) == gff.HEADER + b"".join(t for _i, t in texts)
    assert [i for i, _t in texts] == [3 * k for k in range(len(writes))]              # the ordinals go on without the index


@pytest.mark.parametrize("gzip", [False, True])
def test_an_empty_record_name_leaves_no_file(tmp_path, caplog, gzip):
    """One warning, no `.gff3[.gz]` and no `.tbi`; what an earlier run left is removed; later writes are not rendered."""
    p = _plan(tmp_path, gzip)
    os.makedirs(p.directory)
    for left in [p.paths["in.fa"]] + ([p.paths["in.fa"] + ".tbi"] if gzip else []):
        open(left, "wb").write(b"left by an earlier run")
    files = bed.BedFiles(p, "in.fa")
    rows, sc, texts = _spans([(5, 90), (100, 200), (300, 400)], [0, 1, 2]), _scores(3), []
    with caplog.at_level(logging.WARNING):
        files.write([b"a"], False, None, _fake_write(p, [b"a"], False, rows, sc, [1000], texts=texts))
        files.write([b"a", b"", b"c"], True, None, _fake_write(p, [b"a", b"", b"c"], True, rows, sc, [1000] * 3, texts=texts))
        files.write([b"d"], False, None, _fake_write(p, [b"d"], False, rows, sc, [1000], texts=texts))
        files.write([b""], False, None, gff.GffWrite([b""]))
        files.commit()
    assert len(caplog.records) == 1 and "no GFF3 file is written (--bed_gff3): a record with an empty name" in caplog.records[0].getMessage()
    assert os.listdir(p.directory) == [] and len(texts) == 1


def test_abort_and_the_wrong_kind_of_write(tmp_path):
    p = _plan(tmp_path)
    rows, sc = _spans([(5, 90), (100, 200)]), _scores(2)
    files = bed.BedFiles(p, "in.fa")
    files.write([b"a"], False, None, _fake_write(p, [b"a"], False, rows, sc, [1000]))
    assert len(os.listdir(p.directory)) == 1
    files.abort()
    assert os.listdir(p.directory) == []
    for wrong in (sc, bed.BedWrite(b"", [b"a"])):                                     # a GFF3 file is not written from host scores
        f2 = bed.BedFiles(p, "in.fa")
        try:
            with pytest.raises(ValueError, match="GffWrite"):
                f2.write([b"a"], False, rows, wrong)
        finally:
            f2.abort()
    assert os.listdir(p.directory) == []
