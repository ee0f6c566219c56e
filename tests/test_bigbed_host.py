"""bigbed.py without a GPU: the reference statements on hand-written cases, the container BigBedBuilder writes read back by the
independent reader (bigbed_reader.py), the host-side refusals of the two entries' ABI, of the command line and of BedFiles, and the
bytes of a bigWig, which the shared builder must not change."""
import ctypes as C
import hashlib
import io
import logging
import os
import struct
import zlib

import numpy as np
import pytest

from bigbed_cases import host_write, ladder, rows_scores
from bigbed_reader import BigBed
from conftest import GOLDEN

EINVAL, ENOMEM = -1, -3
TOP = (1 << 32) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


def _err(L):
    return L.dgrp_last_error().decode("utf-8", "replace")


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_the_symbols_are_declared_exported_and_bound(L):
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_bed_blocks_workspace_bytes", "dgrp_bed_blocks_batch", "dgrp_bed_zoom_workspace_bytes", "dgrp_bed_zoom_batch"):
        assert name + "(" in header and name in _lib.exported_symbols() and hasattr(L, name), name
    assert "dgrp_bed_block;" in header and L.dgrp_abi_version() == 1


def test_workspace_queries_return_zero_on_refused_arguments(L):
    def ends(*e):
        return np.array(e, np.int64)
    for q in (L.dgrp_bed_blocks_workspace_bytes, L.dgrp_bed_zoom_workspace_bytes):
        good = ends(5000, TOP)
        assert q(1000, 2, good.ctypes.data) > 0 and q(0, 2, good.ctypes.data) > 0
        assert q(2000, 2, good.ctypes.data) > q(1000, 2, good.ctypes.data)
        assert q(-1, 2, good.ctypes.data) == 0 and q(1 << 31, 2, good.ctypes.data) == 0
        assert q(1000, 0, good.ctypes.data) == 0 and q(1000, 1 << 31, good.ctypes.data) == 0 and q(1000, 2, None) == 0
        for bad in (ends(5000, 0), ends(-3, 10), ends(5000, TOP + 1)):
            assert q(1000, 2, bad.ctypes.data) == 0, bad
    # the zoom workspace grows with the level-0 windows, the blocks workspace does not
    small, large = ends(1 << 20), ends(1 << 30)
    assert L.dgrp_bed_zoom_workspace_bytes(10, 1, large.ctypes.data) > L.dgrp_bed_zoom_workspace_bytes(10, 1, small.ctypes.data) + (1 << 20) * 12
    assert L.dgrp_bed_blocks_workspace_bytes(10, 1, large.ctypes.data) == L.dgrp_bed_blocks_workspace_bytes(10, 1, small.ctypes.data)


def _call(L, entry, by_contig=1, nrows=4, nrec=2, rec_end=(100, 200), chrom0=0, cap=0, tcap=0, heads=True, rows=0x1000, out=None, table=None,
          work=0x1000, work_bytes=1 << 40):
    """An entry with host tables only (every device pointer is a dummy that a host-side refusal never touches): -> (rc, the host
    outputs as one int64 array, -7 where the entry did not write)."""
    ends = np.array(rec_end, np.int64) if rec_end is not None else None
    pe = ends.ctypes.data if ends is not None else None
    host = np.full(64, -7, np.int64)
    p = lambda k: C.cast(host.ctypes.data + 8 * k, C.POINTER(C.c_int64)) if heads else None
    if entry == "blocks":
        rc = L.dgrp_bed_blocks_batch(by_contig, rows, rows, nrows, 0, nrec, pe, chrom0, out, cap, p(0), table, tcap, p(1), p(2), work, work_bytes, None)
    else:
        q = lambda k: host.ctypes.data + 8 * k if heads else None
        rc = L.dgrp_bed_zoom_batch(by_contig, rows, rows, nrows, 0, nrec, pe, chrom0, out, cap, q(0), table, tcap, q(11), q(22), work, work_bytes, None)
    return rc, host


@pytest.mark.parametrize("entry", ["blocks", "zoom"])
@pytest.mark.parametrize("kw,words", [
    (dict(heads=False), ("NULL h_",)),
    (dict(nrows=-1), ("bad nrows -1",)),
    (dict(nrows=1 << 31), ("bad nrows",)),
    (dict(nrec=0), ("bad nrec 0",)),
    (dict(rec_end=None), ("no record ends",)),
    (dict(by_contig=0), ("without by_contig", "nrec must be 1, not 2")),
    (dict(rec_end=(100, 0)), ("record 1", "ends at 0", "outside 1..2^32 - 1")),
    (dict(rec_end=(TOP + 1, 5)), ("record 0", "ends at 4294967296", "largest coordinate of a bigBed")),
    (dict(chrom0=-1), ("bad first chromId -1",)),
    (dict(chrom0=TOP - 1), ("bad first chromId",)),
    (dict(cap=-1), ("bad cap",)),
    (dict(tcap=-1), ("bad cap/table_cap",)),
    (dict(rows=None), ("NULL rows",)),
    (dict(cap=64), ("NULL rows, scores, output or table",)),            # d_out may be NULL only with cap 0
    (dict(tcap=5), ("NULL rows, scores, output or table",)),
    (dict(tcap=5, table=0x1004), ("aligned",)),
])
def test_host_side_refusals_name_the_entry(L, entry, kw, words):
    rc, host = _call(L, entry, **kw)
    msg = _err(L)
    assert rc == EINVAL, (kw, rc, msg)
    assert msg.startswith(f"dgrp_bed_{entry}_batch: "), msg
    for w in words:
        assert w in msg, (kw, msg)
    if kw.get("heads", True):
        nfill = 3 if entry == "blocks" else 27                          # the counts (zoom: 11 + 11 offsets, 5 totals), zeroed in front
        assert (host[:nfill] == 0).all() and (host[nfill:] == -7).all()


def test_zoom_alignment_a_short_workspace_and_an_empty_call(L):
    rc, _h = _call(L, "zoom", cap=64, out=0x1008, tcap=5, table=0x1000)
    assert rc == EINVAL and _err(L).startswith("dgrp_bed_zoom_batch: ") and "16-byte" in _err(L)
    for entry in ("blocks", "zoom"):
        rc, _h = _call(L, entry, work_bytes=16)
        assert rc == ENOMEM and _err(L).startswith(f"dgrp_bed_{entry}_batch: workspace too small"), _err(L)
        rc, _h = _call(L, entry, work=None)
        assert rc == ENOMEM, _err(L)
        rc, host = _call(L, entry, nrows=0, rows=None, work=None)       # no rows: no device work, every count 0
        nfill = 3 if entry == "blocks" else 27
        assert rc == 0 and (host[:nfill] == 0).all() and (host[nfill:] == -7).all(), _err(L)


# ------------------------------------------------------------------------------------------------------- the reference statements
def test_reference_items_blocks_and_totals_on_a_hand_written_case():
    from deepgrp_amd import bed, bigbed as bb
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE
    one = 1 << 24
    rows = np.array([(10, 20, 3, 0), (20, 1030, 12, 0), (5, 7, 1, 2)], SEGMENT_DTYPE)
    scores = np.array([(int(0.8123 * one) * 10, 10, 9, int(0.4 * one), 0), (0, 1010, 0, 0, 0), (2 * one, 2, 2, one, 0)], ROW_SCORE_DTYPE)
    items = bb.reference_items(True, rows, scores, 0, 7)
    assert items[0] == (0, 10, 20, b"\x07\0\0\0" + b"\x0a\0\0\0" + b"\x14\0\0\0" + b"class3\t812\t.\t0.8123\t0.4000\t0.9000\0")
    assert items[1][3] == struct.pack("<III", 7, 20, 1030) + b"class12\t0\t.\t0.0000\t0.0000\t0.0000\0"
    assert items[2] == (2, 5, 7, struct.pack("<III", 9, 5, 7) + b"class1\t1000\t.\t1.0000\t1.0000\t1.0000\0")
    lines = bed.reference_lines([b"a", b"b", b"c"], True, rows, scores)
    assert lines == b"".join((b"a", b"a", b"c")[i] + b"\t%d\t%d\t" % (s, e) + raw[12:-1] + b"\n" for i, (_r, s, e, raw) in enumerate(items))
    data, table = bb.reference_blocks(True, rows, scores, 0, 7)
    assert data == b"".join(it[3] for it in items)
    n0 = len(items[0][3]) + len(items[1][3])
    assert table.tolist() == [(0, n0, 0, 10, 1030, 2), (n0, len(items[2][3]), 2, 5, 7, 1)]
    assert bb.reference_totals(True, rows, scores) == (1022, 1, 1, 1022, 1022)
    # min_score filters items, blocks and coverage alike
    assert [it[0] for it in bb.reference_items(True, rows, scores, 500, 7)] == [0, 2]
    assert bb.reference_totals(True, rows, scores, 500) == (12, 1, 1, 12, 12)
    assert bb.reference_totals(True, rows, scores, 1001) == (0, 0, 0, 0, 0) and bb.reference_blocks(True, rows, scores, 1001)[0] == b""


def test_reference_zoom_on_a_hand_written_case():
    from deepgrp_amd import bigbed as bb
    rows, scores = rows_scores([(1000, 1030), (1040, 5000), (1 << 20, (1 << 20) + 1)], contigs=[0, 0, 1])
    zdata, roff, ztable, boff = bb.reference_zoom(True, rows, scores, 0, 3)
    one = struct.pack("<f", 1.0)
    rec = lambda c, a, b, n: struct.pack("<IIII", c, a, b, n) + one + one + struct.pack("<ff", n, n)
    level0 = (rec(3, 1000, 1024, 24) + rec(3, 1024, 2048, 6 + 1008) + rec(3, 2048, 3072, 1024) + rec(3, 3072, 4096, 1024) + rec(3, 4096, 5000, 904)
              + rec(4, 1 << 20, (1 << 20) + 1, 1))
    level1 = rec(3, 1000, 4096, 24 + 1014 + 2048) + rec(3, 4096, 5000, 904) + rec(4, 1 << 20, (1 << 20) + 1, 1)
    level2 = rec(3, 1000, 5000, 3990) + rec(4, 1 << 20, (1 << 20) + 1, 1)
    assert zdata == level0 + level1 + level2 * 8
    assert roff.tolist() == [0, 6, 9] + [9 + 2 * k for k in range(1, 9)] and boff.tolist() == list(range(11))
    assert ztable[0].tolist() == (0, 192, 0, 0, 0, 1, 1000, (1 << 20) + 1) and ztable[9].tolist() == (32 * 23, 64, 0, 9, 0, 1, 1000, (1 << 20) + 1)


def test_a_block_is_512_items_of_one_record():
    from deepgrp_amd import bigbed as bb
    counts = [0, 3, 512, 0, 700]
    spans, contigs = [], []
    for r, n in enumerate(counts):
        spans += ladder(n)
        contigs += [r] * n
    rows, scores = rows_scores(spans, contigs)
    data, table = bb.reference_blocks(True, rows, scores, 0, 7)
    assert table["rec"].tolist() == [1, 2, 4, 4] and table["items"].tolist() == [3, 512, 512, 188]
    assert (table["off"] == np.r_[0, np.cumsum(table["bytes"])[:-1]]).all() and int(table["bytes"].sum()) == len(data)
    assert int(table["bytes"].max()) <= 512 * 60 < 0xff00               # the bound the header states


# ------------------------------------------------------------------------------------------------------------- the whole file
def _file(tmp_path, writes):
    from deepgrp_amd import bigbed as bb
    path = tmp_path / "t.bb"
    with open(path, "w+b") as fh:
        b = bb.BigBedBuilder(fh, str(tmp_path))
        for names, sizes, w in writes:
            b.add(names, sizes, w)
        b.finish()
    assert sorted(os.listdir(tmp_path)) == ["t.bb"]                      # the spool is gone
    return path.read_bytes()


@pytest.mark.parametrize("level,min_score", [(1, 0), (0, 300)])
def test_a_whole_file_read_back_by_the_independent_reader(tmp_path, level, min_score):
    from deepgrp_amd import bed, bigbed as bb
    # write 1: a batch of three records (1100 rows: three blocks; none; 4 rows), write 2: one record with a row over 3000 windows
    spans = ladder(1100) + [(0, 1), (1, 9), (2000, 3024), (4000, 4001)]
    contigs = [0] * 1100 + [2] * 4
    rows1, scores1 = rows_scores(spans, contigs, low=(0, 511, 512, 1099, 1101))
    rows2, scores2 = rows_scores([(7, 19), (1024, 1024 + 3_000_000), (3_500_000, 3_500_001)], low=(2,))
    names, sizes = [b"chrA", b"none", b"chrB", b"big"], [50_000, 123, 4001, 3_600_000]
    data = _file(tmp_path, [(names[:3], sizes[:3], host_write(names[:3], sizes[:3], True, rows1, scores1, min_score, 0, level)),
                            ([b"nobase"], [77], None),
                            (names[3:], sizes[3:], host_write(names[3:], sizes[3:], False, rows2, scores2, min_score, 4, level))])
    r = BigBed(data)
    assert (r.field_count, r.defined_fields, r.autosql_at) == (9, 6, 304) and r.autosql + b"\0" == bb.AUTOSQL
    for word in (b"table ", b"string chrom;", b"uint   chromStart;", b"uint   chromEnd;", b"string name;", b"uint   score;", b"char[1] strand;",
                 b"float  mean;", b"float  minProb;", b"float  agree;"):
        assert word in r.autosql, word
    assert r.autosql.count(b";") == 9
    assert r.chroms == sorted([(b"chrA", 0, 50_000), (b"none", 1, 123), (b"chrB", 2, 4001), (b"nobase", 3, 77), (b"big", 4, 3_600_000)])
    items, zooms = r.check_all()                                         # zoom levels, summary and uncompressBufSize from the items
    want = bed.reference_lines(names[:3], True, rows1, scores1, min_score) + bed.reference_lines(names[3:], False, rows2, scores2, min_score)
    assert r.lines() == want and want.count(b"\n") == r.item_count == len(items)
    assert len(items) == 1107 if min_score == 0 else 512 < len(items) < 1100     # (means that print 0 and 7 go with the LOW rows)
    assert r.nzoom == 6 and [len(z[1]) for z in zooms][-1] >= 2         # 1024 * 4^5 < 3.6 Mbp <= 1024 * 4^6
    assert len(r._data_leaves()[0]) == (5 if min_score == 0 else 3)      # blocks: 512 + 512 + rest (512 + rest) of chrA, chrB, big (none: all its rows are below 300)
    # R-tree queries against scans: inside a block, across a block edge, across nothing, beyond the records
    edge = items[511][1]
    for q in ((0, 0, 50_000), (0, edge - 100, edge + 100), (0, items[511][2], items[512][1]), (0, 45_000, 50_000), (1, 0, 123), (2, 1, 2),
              (2, 9, 2000), (4, 2000, 2001), (4, 3_400_000, 3_500_000), (4, 0, TOP), (3, 0, 77), (9, 0, 10)):
        assert r.query(*q) == [it for it in items if it[0] == q[0] and it[1] < q[2] and it[2] > q[1]], q
    assert r.query(0, edge - 100, edge + 100) != [] and r.query(0, items[511][2], items[512][1]) == []
    for block in r._data_leaves()[0]:                                    # Python's zlib inflates every block (the reader used it too)
        assert len(zlib.decompress(data[block[4]:block[4] + block[5]])) <= r.buf_size


def test_an_empty_file_is_valid(tmp_path):
    for writes in ([], [([b"a", b"b"], [10, 5000], None)]):
        r = BigBed(_file(tmp_path, writes))
        assert r.check_all() == ([], []) and r.item_count == 0 and r.nzoom == 0 and r.summary == (0, 0.0, 0.0, 0.0, 0.0) and r.buf_size == 0
        assert r.query(0, 0, 100) == [] and len(r.chroms) == (2 if writes else 0)
    rows, scores = rows_scores(ladder(3), low=(0, 1, 2))                 # a write whose rows are all filtered
    r = BigBed(_file(tmp_path, [([b"a"], [5000], host_write([b"a"], [5000], False, rows, scores, 300))]))
    assert r.check_all() == ([], []) and r.chroms == [(b"a", 0, 5000)]


def test_the_bytes_of_a_bigwig_are_what_they_were():
    """A small bigWig through BigWigBuilder (stored zlib blocks: the same bytes from every zlib) has the SHA-256 the builder gave
    before it learnt to carry a bigBed, and cir_tree's new parameter defaults to the 1 a bigWig states."""
    from deepgrp_amd import bigwig as bw
    fh = io.BytesIO()
    b = bw.BigWigBuilder(fh, 2, 1, None)
    blocks, table = [], np.zeros(300, bw.SECTION_DTYPE)
    for j in range(300):
        start = np.array([0, 10, 30], np.int64) + 100 * j
        end = start + np.array([5, 20, 7])
        (raw,) = bw.section_bytes(1, start, end, np.array([1, 50, 100], np.int64), 2)
        blocks.append(raw)
        table[j] = (0, len(raw), 1, start[0], end[-1], 0)
    streams = [zlib.compress(x, 0) for x in blocks]
    ztab, z = np.zeros(2, bw.ZOOM_BLOCK_DTYPE), []
    for k in range(2):
        z.append(zlib.compress(struct.pack("<IIIIffff", 1, 0, 29937, 9600, 0.01, 1.0, 5.0, 6.0), 0))
        ztab[k] = (0, 32, 0, k, 1, 1, 0, 29937)
    b.add([b"empty", b"chrA"], [7, 40000],
          bw.ClassWrite(b"".join(streams), np.array([len(s) for s in streams], np.int64), table, b"".join(z), np.array([len(s) for s in z], np.int64),
                        ztab, (9600, 1, 100, 500, 600)))
    b.finish()
    data = fh.getvalue()
    assert len(data) == 31688 and hashlib.sha256(data).hexdigest() == "6dada413d7a9de2b8f308c96a8883a6b7850e0ad23a08f33b421727b80a8c215"
    leaves = np.zeros(300, bw.LEAF_DTYPE)
    leaves["sb"], leaves["eb"], leaves["off"], leaves["size"] = table["start"], table["end"], 1000 + 50 * np.arange(300), 50
    for lv in (leaves, leaves[:0]):
        assert bw.cir_tree(lv, 777, 888) == bw.cir_tree(lv, 777, 888, 1)
        other = bw.cir_tree(lv, 777, 888, 512)
        assert other[:40] + struct.pack("<I", 1) + other[44:] == bw.cir_tree(lv, 777, 888) and struct.unpack_from("<I", other, 40)[0] == 512


# ------------------------------------------------------------------------------------------ the command line and BedFiles
def test_command_line_refusals_before_any_device_work(tmp_path, monkeypatch):
    from deepgrp_amd import bed
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import pipeline
    from deepgrp_amd.__main__ import CommandLineParser, main

    def touched(*_a, **_k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(pipeline, "require_gpu", touched)
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGTACGTACGT\n")
    sub = tmp_path / "sub"
    sub.mkdir()
    (sub / "a.fa").write_bytes(b">r\nACGT\n")
    ann = tmp_path / "a.bed"
    ann.write_text("r\t0\t4\t1\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    out, bdir = str(tmp_path / "o.tsv"), str(tmp_path / "beds")
    for argv, words in ((["predict", model, str(fa), "--bed_bigbed", "--output", out], ("--bed_bigbed needs --bed_dir",)),
                        (["--bed_bigbed", model, str(fa), "--output", out], ("--bed_bigbed needs --bed_dir",)),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--bed_gzip", "--output", out],
                         ("--bed_bigbed", "writes a bigBed file instead of BED text", "--bed_gzip")),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--bed_gzip", "--bed_index", "--output", out],
                         ("--bed_bigbed", "writes a bigBed file instead of BED text", "--bed_index")),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--bed_index", "--output", out], ("--bed_",)),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--gzip_level", "2", "--output", out],
                         ("--gzip_level must be 0",)),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--bed_min_score", "1001", "--output", out],
                         ("--bed_min_score must lie in 0..1000",)),
                        (["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--split_contigs", "--output", out],
                         ("--bed_dir runs in one process",)),
                        (["predict", model, str(fa), str(sub / "a.fa"), "--bed_dir", bdir, "--bed_bigbed", "--output", out],
                         ("a.fa.bb", "collide")),
                        (["--bed_bigbed", "--bed_dir", bdir, "evaluate", model, str(ann), str(fa), "--output", out],
                         ("--bed_bigbed belongs to predict",)),
                        (["--bed_bigbed", "evaluate", model, str(ann), str(fa), "--output", out], ("--bed_bigbed belongs to predict",))):
        with pytest.raises(SystemExit) as e:
            main(argv)
        for word in words:
            assert word in str(e.value.code), (argv, e.value.code)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        main(["predict", model, str(fa), "--bed_dir", bdir, "--bed_bigbed", "--output", out])
    assert "--bed_dir runs in one process" in str(e.value.code)
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(bdir) and not os.path.exists(out)
    args = lambda argv: CommandLineParser().parse_args(argv).args
    p = bed.plan(args(["predict", "m.h5", "x.fa", "--bed_dir", "d", "--bed_bigbed"]))
    assert p.bigbed and p.gzip_level == 1 and not p.index and p.min_score == 0 and p.paths == {"x.fa": os.path.join("d", "x.fa.bb")}
    p = bed.plan(args(["predict", "m.h5", "x.fa", "--bed_dir", "d", "--bed_bigbed", "--gzip_level", "0", "--bed_min_score", "600"]))
    assert p.bigbed and p.gzip_level == 0 and p.min_score == 600       # --gzip_level with --bed_bigbed alone is accepted
    p = bed.plan(args(["predict", "m.h5", "x.fa", "--bed_dir", "d"]))
    assert not p.bigbed and p.gzip_level is None and p.paths == {"x.fa": os.path.join("d", "x.fa.bed")}
    assert bed.BedPlan("d", 0, {}) == bed.BedPlan("d", 0, {}, None, False, False)          # appended last: earlier constructions hold
    assert bed.bed_path("d", "-", bigbed=True) == os.path.join("d", "stdin.bb")
    with pytest.raises(SystemExit) as e:                                # one input twice: one .bb for both
        bed.plan(args(["predict", "m.h5", str(fa), str(fa), "--bed_dir", bdir, "--bed_bigbed"]))
    assert "an input file is given twice" in str(e.value.code)


@pytest.mark.parametrize("case,word", [("ok", None), ("empty", "empty name"), ("dup", "two records have the name 'a'"),
                                       ("dup_in_one_write", "two records have the name 'a'"), ("over", "above 2^32 - 1")])
def test_bed_files_writes_a_bigbed_or_warns_once_and_leaves_none(tmp_path, caplog, case, word):
    from deepgrp_amd import bed, bigbed as bb
    plan = bed.BedPlan(str(tmp_path), 0, {"in.fa": str(tmp_path / "in.fa.bb")}, 1, False, True)
    (tmp_path / "in.fa.bb").write_bytes(b"left by an earlier run")
    files = bed.BedFiles(plan, "in.fa")

    def fake(names, sizes, chrom):
        rows, scores = rows_scores(ladder(2), [0, 0])
        return host_write(names, sizes, True, rows, scores, 0, chrom)
    with caplog.at_level(logging.WARNING):
        files.write([b"a", b"b"], True, None, fake([b"a", b"b"], [500, 40], 0))
        if case == "empty":
            files.write([b""], True, None, fake([b""], [500], 2))
        elif case == "dup":
            files.write([b"c"], True, None, fake([b"c"], [500], 2))
            files.write([b"a"], True, None, fake([b"a"], [500], 3))
        elif case == "dup_in_one_write":
            files.write([b"c", b"a"], True, None, fake([b"c", b"a"], [500, 500], 2))
        elif case == "over":
            assert "largest coordinate of a bigBed" in bb.end_refusal([b"c"], [1 << 32])
            files.write([b"c"], False, None, bb.BigBedWrite([b"c"], [1 << 32], bb.end_refusal([b"c"], [1 << 32])))
        files.write([b"nothing"], False, None, bed.empty_write(plan, b"nothing", 12, 2))
        files.write([b"z"], True, None, fake([b"z"], [900], 3))          # (after a refusal: ignored, no second warning)
        files.commit()
    warned = [r.getMessage() for r in caplog.records if "no bigBed" in r.getMessage()]
    if word is None:
        assert warned == [] and sorted(os.listdir(tmp_path)) == ["in.fa.bb"]
        r = BigBed((tmp_path / "in.fa.bb").read_bytes())
        items, _z = r.check_all()
        assert r.chroms == [(b"a", 0, 500), (b"b", 1, 40), (b"nothing", 2, 12), (b"z", 3, 900)]
        assert [(c, s) for c, s, _e, _r in items] == [(0, 5), (0, 45), (3, 5), (3, 45)]
    else:
        assert len(warned) == 1 and word in warned[0] and "in.fa" in warned[0] and "--bed_bigbed" in warned[0]
        assert os.listdir(tmp_path) == []                                # no file, no temporary file, and the stale one is gone


def test_bed_files_abort_a_wrong_chrom_and_scores_on_the_host(tmp_path):
    from deepgrp_amd import bed
    plan = bed.BedPlan(str(tmp_path), 0, {"in.fa": str(tmp_path / "in.fa.bb")}, 1, False, True)
    rows, scores = rows_scores(ladder(2))
    files = bed.BedFiles(plan, "in.fa")
    files.write([b"a"], False, rows, host_write([b"a"], [500], False, rows, scores))
    with pytest.raises(ValueError, match="arrived as record 1"):
        files.write([b"b"], False, rows, host_write([b"b"], [500], False, rows, scores, 0, 5))
    with pytest.raises(ValueError, match="BigBedWrite"):
        files.write([b"b"], False, rows, scores)
    files.abort()
    assert os.listdir(tmp_path) == []
