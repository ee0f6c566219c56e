"""bigwig.py without a GPU: the container BigWigBuilder writes, read back by the independent reader (bigwig_reader.py); the host zlib
entry against zlib.decompress; the refusals of the three entries' ABI, of the command line and of TrackFiles."""
import logging
import os
import struct
import zlib

import numpy as np
import pytest

from bigwig_reader import BigWig
from conftest import GOLDEN
from deflate_corpus import corpus as deflate_corpus
from deflate_lz_corpus import corpus as deflate_lz_corpus

EINVAL = -1


def _compress(blocks, level=1):
    """Python's zlib in place of the library's (the builder takes any zlib streams): -> (blob, sizes)."""
    streams = [zlib.compress(b, level) for b in blocks]
    return b"".join(streams), np.array([len(s) for s in streams], np.int64)


def _write(bw, nsec, rec=0, start0=0, digits=2, zoom=True, chrom=None):
    """A ClassWrite of `nsec` hand-made sections of record `rec` of the write, chromId `chrom` of the file (3 items each), and one
    zoom record per level."""
    chrom = rec if chrom is None else chrom
    blocks, table = [], np.zeros(nsec, bw.SECTION_DTYPE)
    s1 = s2 = covered = 0
    for j in range(nsec):
        start = np.array([0, 10, 30], np.int64) + start0 + 100 * j
        end = start + np.array([5, 20, 7])
        q = np.array([1, 50, 100], np.int64)
        (raw,) = bw.section_bytes(chrom, start, end, q, digits)
        blocks.append(raw)
        table[j] = (0, len(raw), rec, start[0], end[-1], 0)
        s1 += int((q * (end - start)).sum())
        s2 += int((q * q * (end - start)).sum())
        covered += int((end - start).sum())
    blob, sizes = _compress(blocks)
    ztab, zblocks = np.zeros(0, bw.ZOOM_BLOCK_DTYPE), []
    if zoom and nsec:
        ztab = np.zeros(bw.ZOOM_LEVELS, bw.ZOOM_BLOCK_DTYPE)
        lo, hi = start0, start0 + 100 * (nsec - 1) + 37
        for k in range(bw.ZOOM_LEVELS):
            zblocks.append(struct.pack("<IIIIffff", chrom, lo, hi, covered, 0.01, 1.0, s1 / 100, s2 / 10000))
            ztab[k] = (0, 32, 0, k, rec, rec, lo, hi)
    zblob, zsizes = _compress(zblocks)
    return bw.ClassWrite(blob, sizes, table, zblob, zsizes, ztab, (covered, 1, 100, s1, s2) if nsec else (0, 0, 0, 0, 0))


def _build(tmp_path, writes, digits=2, bin=1):
    """[(names, sizes, ClassWrite or None)] through a builder: -> the reader on the file."""
    from deepgrp_amd import bigwig as bw
    path = tmp_path / "t.bw"
    with open(path, "w+b") as fh:
        b = bw.BigWigBuilder(fh, digits, bin, str(tmp_path))
        for names, sizes, w in writes:
            b.add(names, sizes, w)
        b.finish()
    assert sorted(os.listdir(tmp_path)) == ["t.bw"]                  # the spool is gone
    return BigWig(path.read_bytes())


@pytest.mark.parametrize("nchrom", [0, 1, 257, 70_000])
def test_chromosome_tree_of_one_leaf_two_and_three_levels(tmp_path, nchrom):
    rng = np.random.default_rng(nchrom)
    names = [b"chr%d_%s" % (i, b"x" * int(rng.integers(0, 9))) for i in range(nchrom)]
    order = rng.permutation(nchrom)
    names = [names[i] for i in order]
    sizes = [int(x) for x in rng.integers(1, 1 << 32, nchrom)]
    r = _build(tmp_path, [(names, sizes, None)] if nchrom else [])
    assert [(k, i) for k, i, _s in r.chroms] == sorted((nm, i) for i, nm in enumerate(names))
    assert {i: s for _k, i, s in r.chroms} == dict(enumerate(sizes))
    bs, ks, n = r._bpt_head()
    assert n == nchrom and bs == min(256, max(1, nchrom)) and ks == max([1] + [len(x) for x in names])
    for i in list(range(min(nchrom, 5))) + ([nchrom - 1, nchrom // 2] if nchrom else []):
        assert r.find_chrom(names[i]) == (i, sizes[i])
    assert r.find_chrom(b"absent") is None and r.find_chrom(b"zzzz") is None
    assert r.nzoom == 0 and r.section_count == 0 and r.summary == (0, 0.0, 0.0, 0.0, 0.0) and r.check_all() == ([], [])


@pytest.mark.parametrize("nsec", [0, 1, 256, 257])
def test_cirtree_of_one_leaf_and_of_two_levels(tmp_path, nsec):
    from deepgrp_amd import bigwig as bw
    half = nsec // 2
    writes = [([b"a", b"empty"], [100 * nsec + 50, 7], _write(bw, half, rec=0)),
              ([b"b"], [100 * nsec + 1000], _write(bw, nsec - half, rec=0, start0=900, chrom=2))]
    r = _build(tmp_path, writes)
    items, zooms = r.check_all()
    assert r.section_count == nsec and len(items) == 3 * nsec
    want = [(0, 100 * j + s, 100 * j + e) for j in range(half) for s, e in ((0, 5), (10, 30), (30, 37))]
    want += [(2, 900 + 100 * j + s, 900 + 100 * j + e) for j in range(nsec - half) for s, e in ((0, 5), (10, 30), (30, 37))]
    assert [(c, s, e) for c, s, e, _v in items] == want
    assert {v for _c, _s, _e, v in items} <= {np.float32(0.01), np.float32(0.5), np.float32(1.0)}
    if nsec >= 2:
        assert r.query(2, 900 + 12, 900 + 31) == [x for x in items if x[0] == 2 and x[1] < 931 and x[2] > 912] != []
        assert r.query(1, 0, 1 << 31) == [] and r.query(0, 5, 10) == []
    covered = 32 * nsec
    assert r.summary[0] == covered
    if nsec:
        assert r.summary[1:3] == (0.01, 1.0) and r.summary[3] == nsec * (5 + 20 * 50 + 7 * 100) / 100
        # R_k < the largest chromSize, and every level has a record of each write
        nz = sum(1 for k in range(10) if 16 * 4 ** k < 100 * nsec + 1000)
        assert r.nzoom == nz and [z[0] for z in zooms] == [16 * 4 ** k for k in range(nz)]
        assert all(len(recs) == (1 if half == 0 else 2) for _red, recs in zooms)
    else:
        assert r.nzoom == 0


def test_reference_items_are_the_lines_of_reference_text():
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd import tracks
    rng = np.random.default_rng(4)
    for digits, width, sp, n in ((2, 1, 0, 300), (3, 7, 13, 1000), (1, 50, 49, 777), (4, 65, 5, 131)):
        v = np.round(rng.random(n) * 1.2 - 0.1, 2).astype(np.float32).clip(0, 1)
        v[40:90] = 0
        v[100:160] = 0.5
        s, e, q = bw.reference_items(v, sp, digits, width)
        val = bw.item_values(q, digits)
        lines = tracks.reference_text(v, sp, b"n", digits, width).split(b"\n")[:-1]
        assert len(lines) == len(s) > 0
        for line, a, b, x in zip(lines, s, e, val):
            _nm, ls, le, lv = line.split(b"\t")
            assert (int(ls), int(le)) == (a, b) and np.float32(float(lv)) == x


# ------------------------------------------------------------------------------------------ zlib on the host
def _zlib_inputs():
    out = [("empty", b""), ("one", b"\x07"), ("ff_full", b"\xff" * 0xff00), ("zeros_full", bytes(0xff00))]
    for name, data in list(deflate_corpus().items()) + list(deflate_lz_corpus().items()):
        out.append((name, bytes(data)[:0xff00]))
    return out


@pytest.mark.parametrize("level", [0, 1])
def test_zlib_compress_host_inflates_to_its_input(level):
    from deepgrp_amd import bigwig as bw
    inputs = _zlib_inputs()
    data = b"".join(d for _n, d in inputs)
    offs = np.cumsum([0] + [len(d) for _n, d in inputs])[:-1]
    blob, sizes = bw.zlib_compress_host(data, offs, [len(d) for _n, d in inputs], level)
    assert len(blob) == sizes.sum()
    at = 0
    for (name, d), s in zip(inputs, sizes):
        stream = blob[at:at + s]
        assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == d, name
        assert struct.unpack(">I", stream[-4:])[0] == zlib.adler32(d), name
        assert s <= len(d) + 11, name                                   # never more than a stored block's overhead
        at += s
    assert sizes[0] == 11 and blob[:11] == bytes.fromhex("7801010000ffff00000001")
    if level == 1:
        assert sizes[2] < 200 and sizes[3] < 200                        # a run is matches


# ------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


def _err(L):
    return L.dgrp_last_error().decode("utf-8", "replace")


def _call(L, entry, C_=5, nrec=2, row0=(0, 64), n=(10, 20), spos=(0, 3), cls=(1, 2), ncls=None, digits=2, bin=1, cap=0, tcap=0, off=True,
          out=None, chrom0=0):
    """A track entry with host tables only (every device pointer is a dummy that a refusal never touches)."""
    r0, nn, sp = (np.array(x, np.int64) for x in (row0, n, spos))
    cl = np.array(cls, np.int32)
    ncls = len(cls) if ncls is None else ncls
    a, b = np.full(700, -7, np.int64), np.full(700, -7, np.int64)
    if entry == "sections":
        rc = L.dgrp_track_sections_batch(0x1000, C_, nrec, r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, cl.ctypes.data, ncls, digits, bin,
                                         chrom0, out, cap, a.ctypes.data if off else None, None, tcap, b.ctypes.data, 0x1000, 1 << 40, None)
    else:
        tot = np.zeros(5 * 64, np.uint64)
        rc = L.dgrp_track_zoom_batch(0x1000, C_, nrec, r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, cl.ctypes.data, ncls, digits, bin,
                                     chrom0, out, cap, a.ctypes.data if off else None, None, tcap, b.ctypes.data, tot.ctypes.data, 0x1000, 1 << 40,
                                     None)
    return rc, a, b


def test_the_symbols_are_exported_and_bound(L):
    from deepgrp_amd import _lib
    for name in ("dgrp_track_sections_workspace_bytes", "dgrp_track_sections_batch", "dgrp_track_zoom_workspace_bytes", "dgrp_track_zoom_batch",
                 "dgrp_zlib_bound", "dgrp_zlib_workspace_bytes", "dgrp_zlib_compress_batch", "dgrp_zlib_compress_host"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    assert L.dgrp_abi_version() == 1


@pytest.mark.parametrize("entry", ["sections", "zoom"])
@pytest.mark.parametrize("kw,words", [
    (dict(nrec=-1), ("bad nrec", "-1")),
    (dict(C_=0), ("bad C",)),
    (dict(cls=(), ncls=0), ("ncls must lie in 1..C",)),
    (dict(cls=(1, 5)), ("class 5", "0..4")),
    (dict(digits=5), ("digits must lie in 1..4", "5")),
    (dict(bin=0), ("bad bin 0",)),
    (dict(chrom0=-1), ("bad first chromId -1",)),
    (dict(chrom0=(1 << 32) - 2), ("bad first chromId",)),
    (dict(cap=-1), ("bad cap",)),
    (dict(tcap=-1), ("bad cap/table_cap",)),
    (dict(n=(10, 0)), ("record 1", "bad n 0")),
    (dict(spos=(0, -2)), ("record 1", "bad offset -2")),
    (dict(row0=(0, -64)), ("record 1", "bad first row")),
    (dict(off=False), ("NULL h_",)),
    (dict(cap=64), ("NULL pointer",)),                                 # d_out may be NULL only with cap 0
    (dict(tcap=5), ("NULL pointer",)),
    (dict(cap=64, out=0x1002), ("aligned",)),
    (dict(n=(10, 20_001), spos=(0, (1 << 32) - 20_001)), ("record 1", "ends at 4294967296", "2^32 - 1")),
    (dict(n=(10, 1), spos=(0, (1 << 32) - 1)), ("record 1", "largest coordinate of a bigWig")),
])
def test_refusals_name_the_entry_and_the_record(L, entry, kw, words):
    rc, a, b = _call(L, entry, **kw)
    msg = _err(L)
    assert rc == EINVAL, (kw, rc, msg)
    assert msg.startswith(f"dgrp_track_{entry}_batch: "), msg
    for w in words:
        assert w in msg, (kw, msg)
    if kw.get("off", True) and "C_" not in kw and "ncls" not in kw:
        nfill = 3 if entry == "sections" else 21
        for t in (a, b):
            assert (t[:nfill] == 0).all() and (t[nfill:] == -7).all()    # filled in full in front of the refusal


def test_an_empty_batch_the_workspaces_and_the_zlib_refusals(L):
    for entry, nfill in (("sections", 4), ("zoom", 31)):
        rc, a, b = _call(L, entry, nrec=0, cls=(3, 1, 0))
        assert rc == 0 and (a[:nfill] == 0).all() and (a[nfill:] == -7).all() and (b[:nfill] == 0).all(), _err(L)

    def wb(query, n=(1000, 2000), spos=(0, 5), bin=1, ncls=2):
        nn, sp = np.array(n, np.int64), np.array(spos, np.int64)
        return query(len(n), nn.ctypes.data, sp.ctypes.data, bin, ncls)
    nn, sp = np.array((1000, 2000), np.int64), np.array((0, 5), np.int64)
    text = L.dgrp_track_batch_workspace_bytes(2, nn.ctypes.data, sp.ctypes.data, 1, 2, 0)
    sec, zoom = L.dgrp_track_sections_workspace_bytes, L.dgrp_track_zoom_workspace_bytes
    assert wb(sec) > text > 0 and wb(zoom) > text
    top = (1 << 32) - 1
    for q in (sec, zoom):
        assert wb(q, n=(1000, 20_000), spos=(0, top - 20_000)) > 0 and wb(q, n=(1000, 20_001), spos=(0, top - 20_000)) == 0
        for bad in (dict(bin=0), dict(ncls=0), dict(n=(1000, 0)), dict(spos=(0, -1))):
            assert wb(q, **bad) == 0, bad
    assert L.dgrp_zlib_bound(3, 100) == 133 and L.dgrp_zlib_bound(-1, 0) == 0
    assert L.dgrp_zlib_workspace_bytes(4, 1) > L.dgrp_zlib_workspace_bytes(4, 0) > 4 * 0xff00 and L.dgrp_zlib_workspace_bytes(4, 2) == 0
    got = np.zeros(1, np.int64)
    import ctypes as C
    p = C.cast(got.ctypes.data, C.POINTER(C.c_int64))
    for args, word in (((0x1000, 10, 0x1000, 8, 1, 0, 0x1000, 100, 0x1000, p, 0x1000, 1 << 30, None), "stride 8"),
                       ((0x1000, 10, 0x1000, 16, 1, 2, 0x1000, 100, 0x1000, p, 0x1000, 1 << 30, None), "level 2"),
                       ((0x1000, 10, None, 16, 1, 0, 0x1000, 100, 0x1000, p, 0x1000, 1 << 30, None), "NULL pointer"),
                       ((0x1000, 10, 0x1000, 16, 1, 0, 0x1000, 100, 0x1000, p, 0x1000, 16, None), "workspace too small"),
                       ((0x1000, 10, 0x1000, 16, 1, 0, 0x1000, 100, 0x1000, p, 0x1008, 1 << 30, None), "aligned")):
        rc = L.dgrp_zlib_compress_batch(*args)
        assert rc != 0 and _err(L).startswith("dgrp_zlib_compress_batch: ") and word in _err(L), (args, _err(L))
    rows = np.array([[0, 0xff01]], np.int64)
    data = bytes(0xff01)
    out = (C.c_uint8 * 70000)()
    sizes = np.zeros(1, np.int64)
    rc = L.dgrp_zlib_compress_host(data, len(data), rows.ctypes.data, 16, 1, 0, out, 70000, sizes.ctypes.data, p)
    assert rc == EINVAL and "row 0" in _err(L) and "65280" in _err(L)
    rows[0] = (5, 0xff00)
    rc = L.dgrp_zlib_compress_host(data, len(data), rows.ctypes.data, 16, 1, 0, out, 70000, sizes.ctypes.data, p)
    assert rc == EINVAL and "does not lie in the input" in _err(L)
    rows[0] = (0, 100)
    rc = L.dgrp_zlib_compress_host(data, len(data), rows.ctypes.data, 16, 1, 1, out, 10, sizes.ctypes.data, p)
    assert rc != 0 and got[0] > 10 and "needed" in _err(L)              # the size is reported, nothing past the capacity is written


# ------------------------------------------------------------------------------------------ the command line and TrackFiles
def test_command_line_refusals_before_any_device_work(tmp_path, monkeypatch):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import pipeline, tracks
    from deepgrp_amd.__main__ import CommandLineParser, main

    def touched(*_a, **_k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(pipeline, "require_gpu", touched)
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was loaded")))
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGTACGTACGT\n")
    ann = tmp_path / "a.bed"
    ann.write_text("r\t0\t4\t1\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    out, tdir = str(tmp_path / "o.tsv"), str(tmp_path / "tracks")
    for argv, word in ((["predict", model, str(fa), "--track_bigwig", "--output", out], "--track_bigwig needs --track_dir"),
                       (["--track_bigwig", model, str(fa), "--output", out], "--track_bigwig needs --track_dir"),
                       (["predict", model, str(fa), "--track_dir", tdir, "--track_bigwig", "--track_gzip", "--output", out], "does not go with"),
                       (["predict", model, str(fa), "--track_dir", tdir, "--track_bigwig", "--track_gzip", "--track_index", "--output", out],
                        "does not go with"),
                       (["predict", model, str(fa), "--track_dir", tdir, "--track_bigwig", "--gzip_level", "2", "--output", out],
                        "--gzip_level must be 0"),
                       (["predict", model, str(fa), "--gzip_level", "1", "--output", out], "--gzip_level needs --mask_gzip or --track_gzip"),
                       (["--track_bigwig", "--track_dir", tdir, "evaluate", model, str(ann), str(fa), "--output", out], "belongs to predict"),
                       (["--track_bigwig", "evaluate", model, str(ann), str(fa), "--output", out], "belongs to predict")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert word in str(e.value.code), argv
    assert not os.path.exists(tdir) and not os.path.exists(out)
    args = lambda argv: CommandLineParser().parse_args(argv).args
    plan = tracks.plan(args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_bigwig"]))
    spec = tracks.resolve(plan, 5)
    assert plan.bigwig and spec.bigwig and spec.gzip_level == 1 and not spec.index
    assert tracks.resolve(tracks.plan(args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_bigwig", "--gzip_level", "0"])), 5).gzip_level == 0
    plan = tracks.plan(args(["predict", "m.h5", "x.fa", "--track_dir", "d"]))
    assert not plan.bigwig and not tracks.resolve(plan, 5).bigwig and tracks.resolve(plan, 5).gzip_level is None
    assert tracks.track_path("d", "x.fa", 3, bigwig=True) == os.path.join("d", "x.fa.class3.bw")


def _fake(tracks, bw, names, sizes, nsec=1, refused=None, chrom=0):
    t = tracks.TrackTexts([b"x", b"x"])
    t.bigwig = tracks.BigWigWrite(list(names), list(sizes), refused, None if refused else [_write(bw, nsec, chrom=chrom), _write(bw, 0)],
                                  chrom)
    return t


@pytest.mark.parametrize("case,word", [("ok", None), ("empty", "empty name"), ("dup", "two records have the name 'a'"),
                                       ("dup_in_one_write", "two records have the name 'a'"), ("over", "above 2^32 - 1")])
def test_track_files_writes_bigwig_or_warns_once_and_leaves_none(tmp_path, caplog, case, word):
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd import tracks
    plan = tracks.TrackPlan(str(tmp_path), (1, 2), 2, 1, {"in.fa": "in.fa"}, 1, False, True)
    spec = tracks.resolve(plan, 5)
    finals = ["in.fa.class1.bw", "in.fa.class2.bw"]
    (tmp_path / finals[0]).write_bytes(b"left by an earlier run")
    files = tracks.TrackFiles(plan, spec, "in.fa")
    with caplog.at_level(logging.WARNING):
        files.write([b"", b""])                                        # a record without bases: nothing, and no complaint
        files.write(_fake(tracks, bw, [b"a", b"b"], [500, 40]))
        if case == "empty":
            files.write(_fake(tracks, bw, [b""], [500]))
        elif case == "dup":
            files.write(_fake(tracks, bw, [b"c"], [500], chrom=2))
            files.write(_fake(tracks, bw, [b"a"], [500], chrom=3))
        elif case == "dup_in_one_write":
            files.write(_fake(tracks, bw, [b"c", b"a"], [500, 500], chrom=2))
        elif case == "over":
            files.write(_fake(tracks, bw, [b"c"], [1 << 32], refused="record 'c' ends at 4294967296, above 2^32 - 1 = 4294967295, the largest"))
        files.write(tracks.empty_texts(spec, b"nothing", 12))
        files.write(_fake(tracks, bw, [b"z"], [900], chrom=3))          # (after a refusal: ignored, no second warning)
        files.commit()
    warned = [r.getMessage() for r in caplog.records if "no bigWig" in r.getMessage()]
    if word is None:
        assert warned == [] and sorted(os.listdir(tmp_path)) == finals
        r = BigWig((tmp_path / finals[0]).read_bytes())
        items, _z = r.check_all()
        assert r.chroms == [(b"a", 0, 500), (b"b", 1, 40), (b"nothing", 2, 12), (b"z", 3, 900)]
        assert [(c, s) for c, s, _e, _v in items[::3]] == [(0, 0), (3, 0)]
        assert BigWig((tmp_path / finals[1]).read_bytes()).check_all() == ([], [])
    else:
        assert len(warned) == 1 and word in warned[0] and "in.fa" in warned[0] and "--track_bigwig" in warned[0]
        assert os.listdir(tmp_path) == []                                # no file, no temporary file, and the stale one is gone


def test_track_files_abort_removes_everything(tmp_path):
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd import tracks
    plan = tracks.TrackPlan(str(tmp_path), (1, 2), 2, 1, {"in.fa": "in.fa"}, 1, False, True)
    files = tracks.TrackFiles(plan, tracks.resolve(plan, 5), "in.fa")
    files.write(_fake(tracks, bw, [b"a"], [500]))
    files.abort()
    assert os.listdir(tmp_path) == []


def test_track_files_commit_that_fails_leaves_the_earlier_run(tmp_path, monkeypatch):
    """The second class's bigWig cannot be finished: commit raises, no temporary file and no spool remains, no file of this run
    appears and the earlier run's files are what they were; abort has nothing left to do."""
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd import tracks
    plan = tracks.TrackPlan(str(tmp_path), (1, 2), 2, 1, {"in.fa": "in.fa"}, 1, False, True)
    before = {f"in.fa.class{c}.bw": b"left by an earlier run: %d" % c for c in (1, 2)}
    for name, data in before.items():
        (tmp_path / name).write_bytes(data)
    listing = lambda: {name: (tmp_path / name).read_bytes() for name in sorted(os.listdir(tmp_path))}
    files = tracks.TrackFiles(plan, tracks.resolve(plan, 5), "in.fa")
    files.write(_fake(tracks, bw, [b"a", b"b"], [500, 40]))
    files.write(_fake(tracks, bw, [b"c"], [700], chrom=2))
    assert len(os.listdir(tmp_path)) == 4                                  # the two temporary files (the spools have no name)
    real, calls = bw.BigWigBuilder.finish, []

    def full_disk(self):
        calls.append(self)
        if len(calls) == 2:
            raise OSError(28, "No space left on device")
        return real(self)
    monkeypatch.setattr(bw.BigWigBuilder, "finish", full_disk)
    with pytest.raises(OSError, match="No space left"):
        files.commit()
    assert len(calls) == 2 and listing() == before
    files.abort()
    assert listing() == before
