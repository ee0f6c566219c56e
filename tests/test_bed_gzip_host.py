"""predict --bed_gzip, --bed_index without a GPU: the new entry points are exported and bound and their workspace queries refuse what
the entries refuse; every refusal of the command line is a SystemExit before the model is read or torch.cuda is touched; BedFiles
with gzip and index on fake writes (members from gz.bgzf_compress, chunks and linear index from bed.reference_index_parts) writes
the payload tabix.reference_index gives for the finished file, warns once and leaves no `.tbi` where the input cannot be indexed,
and leaves nothing behind on abort."""
import argparse
import logging
import os
import zlib

import numpy as np
import pytest

from deepgrp_amd import bed, gz, tabix
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE

ONE = 1 << 24
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


def test_symbols_exported_and_bound(L):
    from deepgrp_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_bed_text_workspace_bytes", "dgrp_bed_text_batch", "dgrp_bed_index_workspace_bytes", "dgrp_bed_index_batch"):
        assert name in _lib.exported_symbols() and hasattr(L, name) and name + "(" in header, name
        assert getattr(L, name).argtypes is not None


def test_workspace_queries_refuse_what_the_entries_refuse(L):
    text, index = L.dgrp_bed_text_workspace_bytes, L.dgrp_bed_index_workspace_bytes
    assert text(0, 1, 0) > 0 and text(5000, 3, 40) >= 5000 * 16 + 40 + 4 * 8
    assert text(-1, 1, 0) == 0 and text(10, 0, 0) == 0 and text(10, 1, -1) == 0 and text(1 << 31, 1, 0) == 0
    assert index(5000, 3, 40, 3) > text(5000, 3, 40)
    assert index(-1, 1, 0, 1) == 0 and index(10, 0, 0, 1) == 0 and index(10, 1, -1, 1) == 0 and index(10, 1, 0, 0) == 0
    assert index(1 << 31, 1, 0, 1) == 0 and index(10, 1, 0, 1 << 31) == 0


def test_entries_refuse_bad_host_arguments_before_any_device_work(L):
    """NULL names, descending name offsets, a record end above 2^29 or below 1, nrec > 1 without by_contig: DGRP_EINVAL from the
    host checks, with no device pointer ever read (they are NULL or bogus here).  No rows: nothing to do."""
    import ctypes as C
    got = C.c_int64(-7)
    off = np.array([0, 3], np.int64)
    assert L.dgrp_bed_text_batch(b"abc", off.ctypes.data, 1, 0, None, None, 0, 0, None, 0, C.byref(got), None, 0, None) == 0 and got.value == 0
    assert L.dgrp_bed_text_batch(None, off.ctypes.data, 1, 0, None, None, 0, 0, None, 0, C.byref(got), None, 0, None) == EINVAL
    bad = np.array([3, 0], np.int64)
    assert L.dgrp_bed_text_batch(b"abc", bad.ctypes.data, 1, 0, None, None, 0, 0, None, 0, C.byref(got), None, 0, None) == EINVAL
    assert b"ascend" in L.dgrp_last_error()
    assert L.dgrp_bed_text_batch(b"abc", off.ctypes.data, 1, 0, None, None, 4, 0, None, 0, C.byref(got), None, 0, None) == EINVAL    # rows without arrays

    def index(ends, nrec=None, by_contig=1, nrows=0):
        e = np.array(ends, np.int64)
        got.value = -7
        return L.dgrp_bed_index_batch(b"abc", off.ctypes.data, 1, by_contig, None, None, nrows, 0, len(e) if nrec is None else nrec,
                                      e.ctypes.data, None, 0, C.byref(got), None, 0, None, None, 0, None)
    assert index([1 << 29]) == 0 and got.value == 0
    assert index([(1 << 29) + 1]) == EINVAL and b"2^29" in L.dgrp_last_error()
    assert index([100, 0]) == EINVAL and b"record 1" in L.dgrp_last_error()
    assert index([100, 100], by_contig=0) == EINVAL and b"nrec must be 1" in L.dgrp_last_error()
    assert index([100], nrec=0) == EINVAL
    assert index([100], nrows=3) == EINVAL                                              # rows without arrays


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    import torch

    def touched(*_a, **_k):
        raise AssertionError("torch.cuda was touched before the refusal")
    for name in ("is_available", "set_device", "current_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_cli_refusals(no_gpu, tmp_path):
    model = str(tmp_path / "no_such_model.h5")                                       # reading it would raise, not exit
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    out = str(tmp_path / "beds")
    _refused(["predict", model, str(fa), "--bed_gzip"], "--bed_gzip needs --bed_dir")
    _refused(["--bed_gzip", model, str(fa)], "--bed_gzip needs --bed_dir")                          # the README form
    _refused(["predict", model, str(fa), "--bed_dir", out, "--bed_index"], "--bed_index needs --bed_gzip")
    _refused(["--bed_index", "--bed_dir", out, model, str(fa)], "--bed_index needs --bed_gzip")     # the README form
    _refused(["predict", model, str(fa), "--bed_index"], "--bed_index needs --bed_gzip")
    # --gzip_level: today's refusal, with the new flag's name behind it; accepted with --bed_gzip alone, where its value is checked
    _refused(["predict", model, str(fa), "--bed_dir", out, "--gzip_level", "1"], "--gzip_level needs --mask_gzip or --track_gzip")
    _refused(["predict", model, str(fa), "--bed_dir", out, "--gzip_level", "1"], "--bed_gzip")
    _refused(["predict", model, str(fa), "--bed_dir", out, "--bed_gzip", "--gzip_level", "2"], "--gzip_level must be 0 (literals only) or 1")
    (tmp_path / "sub").mkdir()
    twin = tmp_path / "sub" / "a.fa"
    twin.write_text(">r\nACGT\n")
    _refused(["predict", model, str(fa), str(twin), "--bed_dir", out, "--bed_gzip"], "have the same file name a.fa.bed.gz; they would collide")
    gzdir = tmp_path / "in"
    gzdir.mkdir()
    # the overwrite check runs on the .bed.gz name: an input DIR/x whose BED would be DIR/x itself cannot exist (the suffix is
    # appended), so the check is reached through a link
    link = gzdir / "l.fa"
    os.symlink(gzdir / "l.fa.bed.gz", link)
    (gzdir / "l.fa.bed.gz").write_bytes(gz.bgzf_compress(b">r\nACGT\n"))
    _refused(["predict", model, str(link), "--bed_dir", str(gzdir), "--bed_gzip"], "would overwrite the input")
    _refused(["--bed_gzip", "--bed_dir", out, "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--bed_dir belongs to predict")
    assert not os.path.exists(out)                                                   # no refusal left a directory behind


def test_plan(tmp_path):
    d = str(tmp_path / "out")
    ns = lambda **k: argparse.Namespace(bed_dir=d, FASTA=["-", str(tmp_path / "x.fa")], **k)
    p = bed.plan(ns(bed_gzip=True))
    assert (p.gzip_level, p.index) == (1, False) and [os.path.basename(v) for v in p.paths.values()] == ["stdin.bed.gz", "x.fa.bed.gz"]
    p = bed.plan(ns(bed_gzip=True, bed_index=True, gzip_level=0, bed_min_score=5))
    assert (p.gzip_level, p.index, p.min_score) == (0, True, 5)
    p = bed.plan(ns())
    assert (p.gzip_level, p.index) == (None, False) and os.path.basename(p.paths["-"]) == "stdin.bed"


# ---- BedFiles on fake writes ---------------------------------------------------------------------------------------------------------
def _rows(spans, contigs=None):
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


def _fake_write(names, by_contig, rows, scores, min_score, rec_end, level=6, refused=None):
    text = bed.reference_lines(names, by_contig, rows, scores, min_score)
    members = gz.bgzf_compress(text, level=level, eof=False) if text else b""
    raw = [nm if isinstance(nm, bytes) else nm.encode() for nm in names]
    if refused is not None or not text:
        return bed.BedWrite(members, raw, refused), text
    return bed.BedWrite(members, raw, None, *bed.reference_index_parts(names, by_contig, rows, scores, min_score, rec_end)), text


def _plan(tmp_path, index=True):
    return bed.BedPlan(str(tmp_path / "out"), 500, {"in.fa": str(tmp_path / "out" / "in.fa.bed.gz")}, 1, index)


def _inflate(data):
    out, off = [], 0
    while off < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[off:]))
        off = len(data) - len(d.unused_data)
    return b"".join(out)


def test_bedfiles_writes_the_reference_index(tmp_path, caplog):
    """Three writes: a long record of nested and wide lines on its own (several members), a batch of four records of which two
    consecutive ones share a name and one has no emitted line, and a write whose every line is filtered."""
    p = _plan(tmp_path)
    files = bed.BedFiles(p, "in.fa")
    rng = np.random.default_rng(8)
    starts = np.sort(rng.integers(0, 40_000_000, 3000))
    spans = [(int(s), int(s) + int(w)) for s, w in zip(starts, rng.integers(1, 40_000, 3000))]
    spans[10] = (spans[10][0], 45_000_000)                                            # covers 2 700 windows; its successors are nested
    spans[-1] = (spans[-1][0], spans[-1][0] + 5)                                      # the last line ends far below the longest
    rows1, sc1 = _rows(spans), _scores(3000, low=(0, 1, 50, 51))
    w1, t1 = _fake_write([b"chrA"], False, rows1, sc1, p.min_score, [1 << 29])
    contigs = [0, 0, 1, 1, 1, 3, 3]
    rows2 = _rows([(5, 90), (20_000, 20_010), (0, 16_384), (16_383, 16_385), (16_385, 140_000), (7, 9), (8, 200_000)], contigs)
    sc2 = _scores(7, seed=2, low=(2,))
    names2 = [b"b1", b"twin", b"twin", b"tail"]                                       # record 2 (the second twin) has no row at all
    w2, t2 = _fake_write(names2, True, rows2, sc2, p.min_score, [100_000, 200_000, 300_000, 200_000])
    rows3, sc3 = _rows([(1, 2), (3, 4)]), _scores(2, low=(0, 1))
    w3, t3 = _fake_write([b"tail"], False, rows3, sc3, p.min_score, [50])
    assert t1.count(b"\n") == 2996 and len(tabix.member_sizes(w1.members)[0]) > 1 and t3 == b"" and t2.count(b"\n") == 6
    for w in (w1, w2, w3):
        files.write(w.names, len(w.names) > 1, None, w)
    assert sorted(os.listdir(tmp_path / "out")) != ["in.fa.bed.gz"]                   # still temporary
    with caplog.at_level(logging.WARNING):
        files.commit()
    assert not caplog.records
    assert sorted(os.listdir(tmp_path / "out")) == ["in.fa.bed.gz", "in.fa.bed.gz.tbi"]
    data = open(p.paths["in.fa"], "rb").read()
    assert data.endswith(gz.BGZF_EOF) and _inflate(data) == t1 + t2
    want = tabix.reference_index(data)
    assert _inflate(open(p.paths["in.fa"] + ".tbi", "rb").read()) == want
    ix = tabix.read_index(want)
    assert ix["names"] == [b"chrA", b"b1", b"twin", b"tail"]
    assert len(ix["linear"][0]) == ((spans[-1][1] - 1) >> 14) + 1 < ((spans[10][1] - 1) >> 14) + 1     # the last line ends the sequence
    lines = (t1 + t2).split(b"\n")[:-1]
    for name, beg, end in ((b"chrA", 0, 1 << 29), (b"chrA", 35_000_000, 35_000_001), (b"twin", 16_384, 16_385), (b"tail", 0, 8),
                           (b"b1", 90, 20_000), (b"nobody", 0, 100)):
        scan = [ln for ln in lines if ln.split(b"\t")[0] == name and int(ln.split(b"\t")[1]) < end and int(ln.split(b"\t")[2]) > beg]
        assert tabix.query(ix, data, name, beg, end) == scan, (name, beg, end)


@pytest.mark.parametrize("case", ["above 2^29", "empty name", "name reappears", "name reappears in a later write"])
def test_an_input_without_an_index(tmp_path, caplog, case):
    """One warning, no `.tbi` (a stale one is removed), the `.bed.gz` as it is without the flag."""
    p = _plan(tmp_path)
    os.makedirs(p.directory)
    stale = p.paths["in.fa"] + ".tbi"
    open(stale, "wb").write(b"left by an earlier run")
    files = bed.BedFiles(p, "in.fa")
    rows, sc = _rows([(5, 90), (100, 200), (300, 400)], [0, 1, 2]), _scores(3)
    ends = [1000, 1000, 1000]
    if case == "above 2^29":
        writes = [_fake_write([b"a", b"b", b"c"], True, rows, sc, 0, ends, refused="record 'b' ends at 536870913, above 2^29"),
                  _fake_write([b"d"], False, rows, sc, 0, [1000])]
    elif case == "empty name":
        writes = [_fake_write([b"a", b"", b"c"], True, rows, sc, 0, ends), _fake_write([b"d"], False, rows, sc, 0, [1000])]
    elif case == "name reappears":
        writes = [_fake_write([b"a", b"b", b"a"], True, rows, sc, 0, ends), _fake_write([b"d"], False, rows, sc, 0, [1000])]
    else:
        writes = [_fake_write([b"a", b"b", b"c"], True, rows, sc, 0, ends), _fake_write([b"c"], False, rows, sc, 0, [1000]),
                  _fake_write([b"b"], False, rows, sc, 0, [1000])]
    with caplog.at_level(logging.WARNING):
        for w, _t in writes:
            files.write(w.names, len(w.names) > 1, None, w)
        files.commit()
    assert len(caplog.records) == 1 and "no tabix index is written (--bed_index)" in caplog.records[0].getMessage()
    assert os.listdir(p.directory) == ["in.fa.bed.gz"]
    assert _inflate(open(p.paths["in.fa"], "rb").read()) == b"".join(t for _w, t in writes)


def test_abort_and_plain_gzip(tmp_path):
    p = _plan(tmp_path)
    rows, sc = _rows([(5, 90), (100, 200)]), _scores(2)
    w, text = _fake_write([b"a"], False, rows, sc, 0, [1000])
    files = bed.BedFiles(p, "in.fa")
    files.write(w.names, False, None, w)
    files.abort()
    assert os.listdir(p.directory) == []
    with pytest.raises(ValueError):                                                   # a BGZF BED is not written from host scores
        f2 = bed.BedFiles(p, "in.fa")
        try:
            f2.write([b"a"], False, rows, sc)
        finally:
            f2.abort()
    # --bed_gzip without --bed_index: the members and the EOF member, no index, and a `.tbi` beside it is not this run's to touch
    q = _plan(tmp_path, index=False)
    files = bed.BedFiles(q, "in.fa")
    files.write(w.names, False, None, bed.BedWrite(w.members, w.names))
    files.commit()
    assert os.listdir(q.directory) == ["in.fa.bed.gz"]
    assert open(q.paths["in.fa"], "rb").read() == w.members + gz.BGZF_EOF and _inflate(w.members) == text


def test_a_commit_that_fails_leaves_the_earlier_run(tmp_path, monkeypatch):
    """The `.tbi` cannot be written: commit raises, no temporary file remains, no file of this run appears and the earlier run's
    files are what they were; abort has nothing left to do."""
    p = _plan(tmp_path)
    os.makedirs(p.directory)
    before = {"in.fa.bed.gz": b"the earlier run's BED", "in.fa.bed.gz.tbi": b"the earlier run's index"}
    for name, data in before.items():
        open(os.path.join(p.directory, name), "wb").write(data)
    listing = lambda: {name: open(os.path.join(p.directory, name), "rb").read() for name in sorted(os.listdir(p.directory))}
    files = bed.BedFiles(p, "in.fa")
    rows, sc = _rows([(5, 90), (100, 200), (300, 400)], [0, 1, 1]), _scores(3)
    for w, _t in (_fake_write([b"a", b"b"], True, rows, sc, 0, [1000, 1000]), _fake_write([b"c"], False, rows[:2], sc[:2], 0, [1000])):
        files.write(w.names, len(w.names) > 1, None, w)
    assert len(os.listdir(p.directory)) == 3                                          # the temporary file

    def full_disk(_payload):
        raise OSError(28, "No space left on device")
    monkeypatch.setattr(tabix, "index_file", full_disk)
    with pytest.raises(OSError, match="No space left"):
        files.commit()
    assert listing() == before
    files.abort()
    assert listing() == before
