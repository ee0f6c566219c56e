"""The tabix index without a GPU: reg2bin at every level boundary, reference_index against a payload written out by hand, the reader
(read_index, query) against a brute-force overlap filter on a corpus of BGZF bedGraph files, IndexBuilder on what the device entry
hands out (restated in Python), the ABI refusals of dgrp_track_index_batch and the refusals of the command line."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from tabix_corpus import BLOCK, brute, device_like, noisy, parse, regions

EINVAL = -1


# ------------------------------------------------------------------------------------------ bins
def test_reg2bin_at_and_across_every_level_boundary():
    from deepgrp_amd.tabix import IndexRefused, reg2bin, reg2bins
    first = {14: 4681, 17: 585, 20: 73, 23: 9, 26: 1}
    assert reg2bin(0, 1) == 4681 and reg2bin(0, 1 << 14) == 4681 and reg2bin(0, (1 << 14) + 1) == 585
    for shift, above in ((14, 17), (17, 20), (20, 23), (23, 26), (26, None)):
        e = 1 << shift
        for k in (1, 3):                                              # the first boundary of the level and a later one
            if k * e >= 1 << (above or 29):
                continue
            assert reg2bin(k * e - 1, k * e) == 4681 + ((k * e - 1) >> 14)                 # ends at the boundary: a leaf
            assert reg2bin(k * e, k * e + 1) == 4681 + ((k * e) >> 14)                     # starts at it
            assert reg2bin((k - 1) * e, k * e) == first[shift] + k - 1                     # fills the level's bin exactly
            want = 0 if above is None else first[above] + ((k * e) >> above)               # straddles it: one level up
            if above is not None and (k * e - 1) >> above != (k * e) >> above:
                want = None
            if want is not None:
                assert reg2bin(k * e - 1, k * e + 1) == want, (shift, k)
    assert reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73 and reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    top = 1 << 29
    assert reg2bin(top - 1, top) == 4681 + 32767 == 37448 and reg2bin(top - (1 << 26), top) == 8 and reg2bin(0, top) == 0
    assert reg2bin(top - (1 << 14), top) == 37448 and reg2bin(top - (1 << 14) - 1, top) == 585 + 4095
    for bad in ((0, 0), (-1, 5), (5, 4), (top - 1, top + 1)):
        with pytest.raises(IndexRefused):
            reg2bin(*bad)
    for beg, end in ((0, 1), (16383, 16385), (131071, 131073), (top - 1, top), (12345, 9_000_000)):
        assert reg2bin(beg, end) in reg2bins(beg, end) and reg2bin(beg, beg + 1) in reg2bins(beg, end)
    assert reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681]


# ------------------------------------------------------------------------------------------ the payload by hand
TEN = [(b"chrA", 0, 100), (b"chrA", 100, 16384), (b"chrA", 16384, 16400), (b"chrA", 16400, 40000), (b"chrA", 40000, 40010),
       (b"chrA", 40010, 40020), (b"chrA", 131071, 131073), (b"chrB", 5, 10), (b"chrB", 300000, 300010), (b"chrB", 300010, 300020)]


def test_reference_index_of_ten_lines_by_hand():
    from deepgrp_amd import gz, tabix
    lines = [b"%s\t%d\t%d\t0.%02d\n" % (nm, s, e, 10 + i) for i, (nm, s, e) in enumerate(TEN)]
    text = b"".join(lines)
    comp = gz.bgzf_compress_host(text, level=1)
    assert comp.endswith(gz.BGZF_EOF) and len(gz.walk_members(comp).start) == 2
    o = np.cumsum([0] + [len(l) for l in lines]).tolist()             # one member at file offset 0: a virtual offset is a text offset
    end = (len(comp) - len(gz.BGZF_EOF)) << 16                        # ... but the end of the text is the EOF member's begin
    p = struct.pack
    want = b"".join([
        b"TBI\1", p("<8i", 2, 0x10000, 1, 2, 3, ord("#"), 0, 10), b"chrA\0chrB\0",
        p("<i", 5),                                                   # chrA: five bins, ascending
        p("<Ii2Q", 73, 1, o[6], o[7]),                                # 131071-131073 straddles 2^17
        p("<Ii2Q", 585, 1, o[3], o[4]),                               # 16400-40000 straddles a 16 kb window
        p("<Ii2Q", 4681, 1, o[0], o[2]),                              # 0-100 and 100-16384: one chunk
        p("<Ii2Q", 4682, 1, o[2], o[3]),
        p("<Ii2Q", 4683, 1, o[4], o[6]),                              # 40000-40010 and 40010-40020
        p("<i9Q", 9, o[0], o[2], o[3], o[6], o[6], o[6], o[6], o[6], o[6]),
        p("<i", 2),                                                   # chrB
        p("<Ii2Q", 4681, 1, o[7], o[8]),
        p("<Ii2Q", 4681 + 18, 1, o[8], end),
        p("<i", 19), p("<19Q", o[7], *([o[8]] * 18)),
        p("<Q", 0)])
    got = tabix.reference_index(comp)
    assert got == want
    ix = tabix.read_index(got)
    assert ix["names"] == [b"chrA", b"chrB"] and ix["bins"][1] == {4681: [(o[7], o[8])], 4699: [(o[8], end)]}
    assert tabix.query(ix, comp, b"chrA", 16383, 16385) == [lines[1][:-1], lines[2][:-1]]
    assert tabix.query(ix, comp, b"chrB", 0, 1 << 29) == [l[:-1] for l in lines[7:]] and tabix.query(ix, comp, b"chrC", 0, 100) == []
    tbi = tabix.index_file(got)
    assert tbi.endswith(gz.BGZF_EOF) and gz.inflate_host(tbi, "tbi", 1 << 20) == got
    for bad in (b"chrA\t0\t5\t0.1\nchrB\t0\t5\t0.1\nchrA\t9\t12\t0.1\n", b"\t0\t5\t0.1\n", b"chrA\t0\t%d\t0.1\n" % ((1 << 29) + 1)):
        with pytest.raises(tabix.IndexRefused):
            tabix.reference_index(gz.bgzf_compress_host(bad))
    assert tabix.read_index(tabix.reference_index(gz.BGZF_EOF))["names"] == []


# ------------------------------------------------------------------------------------------ the reader on a corpus
def _corpus():
    """name -> [record texts] of the five files."""
    from deepgrp_amd.tracks import reference_text
    several = [reference_text(noisy(3000, 1), 0, b"chr1"), reference_text(noisy(30_000, 2), 15_000, b"chr2", 2, 50),
               reference_text(noisy(2000, 3), 70_000, b"chr3", 3)]
    head = reference_text(noisy(9000, 4), 100, b"chr1")
    assert BLOCK - len(head) - 11 > 1
    filler = b"%s\t0\t10\t0.50\n" % (b"x" * (BLOCK - len(head) - 11))
    boundary = [head, filler, reference_text(noisy(5000, 5), 16_000, b"chr3")]
    assert len(head + filler) == BLOCK
    long_name = [reference_text(noisy(21, 6), 16_380, b"L" * 140_000), reference_text(noisy(500, 7), 0, b"chr2")]
    gap = np.r_[noisy(10_000, 8), np.zeros(300_000, np.float32), noisy(10_000, 9)]
    one = np.r_[noisy(3000, 10), np.full(300_000, 0.5, np.float32), noisy(3000, 11)]
    return {"several": several, "boundary": boundary, "long_name": long_name, "gap": [reference_text(gap, 5000, b"chrG")],
            "one_line": [reference_text(one, 1000, b"chr1"), reference_text(noisy(800, 12), 0, b"chr2")]}


@pytest.fixture(scope="module")
def corpus():
    from deepgrp_amd import gz
    return {k: (recs, gz.bgzf_compress_host(b"".join(recs), level=1)) for k, recs in _corpus().items()}


def test_the_corpus_holds_what_it_is_for(corpus):
    from deepgrp_amd import gz
    lines = {k: parse(b"".join(recs)) for k, (recs, _c) in corpus.items()}
    assert len({nm for _l, nm, _s, _e in lines["several"]}) == 3
    ends = np.cumsum([len(l) + 1 for l, *_ in lines["boundary"]])
    assert BLOCK in ends.tolist()                                                       # a line ends exactly at a member boundary
    assert max(len(l) for l, *_ in lines["long_name"]) > 2 * BLOCK                      # a line in three members
    starts = np.array([s for _l, _n, s, _e in lines["gap"]])
    assert np.diff(starts).max() >= 300_000
    assert max(e - s for _l, _n, s, e in lines["one_line"]) == 300_000
    for k, (_recs, comp) in corpus.items():
        assert gz.walk_members(comp).kind == "bgzf", k


@pytest.mark.parametrize("name", ["several", "boundary", "long_name", "gap", "one_line"])
def test_query_returns_what_a_brute_force_filter_returns(corpus, name):
    from deepgrp_amd import tabix
    recs, comp = corpus[name]
    lines = parse(b"".join(recs))
    ix = tabix.read_index(tabix.reference_index(comp))
    assert ix["names"] == list(dict.fromkeys(nm for _l, nm, _s, _e in lines))
    hits = 0
    for nm, beg, end in regions(lines, seed=len(name)):
        got = tabix.query(ix, comp, nm, beg, end)
        assert got == brute(lines, nm, beg, end), (name, nm[:10], beg, end)
        hits += len(got)
    assert hits >= 50                                                                   # (the queries do find lines)


# ------------------------------------------------------------------------------------------ text offsets to a payload
def _build(writes, level=1):
    """The file and the IndexBuilder's payload of a sequence of writes, each [(name, text), ...]: what TrackFiles does."""
    from deepgrp_amd import gz, tabix
    b, comp = tabix.IndexBuilder(), b""
    for recs in writes:
        chunks, linear, text = device_like([t for _nm, t in recs])
        if not text:
            continue
        members = b"".join(gz.bgzf_compress_host(text[o:o + 3 * BLOCK], eof=False, level=level) for o in range(0, len(text), 3 * BLOCK))
        sizes, text_len = tabix.member_sizes(members)
        assert text_len == len(text)
        wpref = np.cumsum([0] + [len(l) + 2 for l in linear])                           # two windows behind every record's last line
        lin = np.full(wpref[-1], -1, np.int64)
        for r, l in enumerate(linear):
            lin[wpref[r]:wpref[r] + len(l)] = l
        arr = np.array([tuple(c) for c in chunks], tabix.CHUNK_DTYPE)
        b.add(len(comp), sizes, text_len, [nm for nm, _t in recs], arr, lin, wpref)
        comp += members
    return comp + gz.BGZF_EOF, b.payload()


@pytest.mark.parametrize("name", ["several", "boundary", "long_name", "gap", "one_line"])
def test_index_builder_gives_the_reference_payload(corpus, name):
    from deepgrp_amd import tabix
    recs = [(parse(t)[0][1], t) for t in corpus[name][0]]
    for writes in ([recs], [[r] for r in recs]):                                        # one batch; record by record
        comp, got = _build(writes)
        assert got == tabix.reference_index(comp), name
    assert comp != corpus[name][1] or len(recs) == 1                                    # (a write ends in a short member)


def test_index_builder_joins_records_of_one_name_and_refuses_a_returning_name():
    from deepgrp_amd import tabix
    from deepgrp_amd.tracks import reference_text
    a1, a2 = reference_text(noisy(3000, 21), 100, b"a"), reference_text(noisy(3000, 22), 2000, b"a")          # same leaf bin at the seam
    a3, none, c = reference_text(noisy(40_000, 23), 0, b"a"), b"", reference_text(noisy(900, 24), 50_000, b"c")
    recs = [(b"a", a1), (b"a", a2), (b"b", none), (b"a", a3), (b"c", c), (b"c", reference_text(noisy(900, 25), 10, b"c")),
            (b"c", reference_text(noisy(900, 27), 40_000, b"c"))]                       # the middle record of c ends two windows early
    for writes in ([recs], [recs[:1], recs[1:4], recs[4:]], [[r] for r in recs]):
        comp, got = _build(writes)
        assert got == tabix.reference_index(comp)
        assert tabix.read_index(got)["names"] == [b"a", b"c"]                           # b has no line: absent
    with pytest.raises(tabix.IndexRefused, match="reappears"):
        _build([[(b"a", a1), (b"c", c), (b"a", a2)]])
    with pytest.raises(tabix.IndexRefused, match="empty"):
        _build([[(b"", reference_text(noisy(100, 26), 0, b""))]])


# ------------------------------------------------------------------------------------------ TrackFiles on fake writes
def _track_write(names, class_texts):
    """One write as the device path hands it to TrackFiles: class_texts[k][r] is the text of record r of class k; the members are
    the host encoder's, chunks and linear index device_like's, two windows behind every record's last line."""
    from deepgrp_amd import gz, tabix, tracks
    parts = [device_like(ts) for ts in class_texts]
    wpref = np.cumsum([0] + [max(len(lin[r]) for _c, lin, _t in parts) + 2 for r in range(len(names))])
    linear = np.full((len(parts), wpref[-1]), -1, np.int64)
    chunks, coff = [], [0]
    for k, (ch, lin, _text) in enumerate(parts):
        for r, l in enumerate(lin):
            linear[k, wpref[r]:wpref[r] + len(l)] = l
        chunks += [tuple(c) for c in ch]
        coff.append(len(chunks))
    texts = tracks.TrackTexts(gz.bgzf_compress_host(text, eof=False, level=1) if text else b"" for _c, _l, text in parts)
    texts.index = tracks.WriteIndex(list(names), None, np.array(chunks, tabix.CHUNK_DTYPE), np.array(coff, np.int64), linear, wpref)
    return texts


def _track_files(tmp_path, classes, index=True):
    from deepgrp_amd import tracks
    plan = tracks.TrackPlan(str(tmp_path), classes, 2, 1, {"in.fa": "in.fa"}, 1, index)
    return tracks.TrackFiles(plan, tracks.resolve(plan, 5), "in.fa")


def _listing(path):
    return {name: (path / name).read_bytes() for name in sorted(os.listdir(path))}


def _class_texts(names, nclasses, seed):
    from deepgrp_amd.tracks import reference_text
    return [[reference_text(noisy(3000 + 500 * k, seed + 10 * k + r), 100 * r, nm) for r, nm in enumerate(names)] for k in range(nclasses)]


def test_track_files_commit_that_fails_leaves_the_earlier_run(tmp_path, monkeypatch):
    """The `.tbi` of the second class cannot be written: commit raises, no temporary file remains (not the first class's staged
    `.tbi` either), no file of this run appears, and the earlier run's files are what they were; abort has nothing left to do."""
    from deepgrp_amd import tabix
    finals = [f"in.fa.class{c}.bedGraph.gz" + ext for c in (1, 2) for ext in ("", ".tbi")]
    for name in finals:
        (tmp_path / name).write_bytes(b"left by an earlier run: " + name.encode())
    before = _listing(tmp_path)
    files = _track_files(tmp_path, (1, 2))
    files.write(_track_write([b"a", b"b"], _class_texts([b"a", b"b"], 2, 1)))
    files.write(_track_write([b"c"], _class_texts([b"c"], 2, 2)))
    assert len(os.listdir(tmp_path)) == len(finals) + 2                                 # the two temporary files
    real, calls = tabix.index_file, []

    def full_disk(payload):
        calls.append(len(payload))
        if len(calls) == 2:
            raise OSError(28, "No space left on device")
        return real(payload)
    monkeypatch.setattr(tabix, "index_file", full_disk)
    with pytest.raises(OSError, match="No space left"):
        files.commit()
    assert len(calls) == 2 and sorted(before) == sorted(finals) and _listing(tmp_path) == before
    files.abort()
    assert _listing(tmp_path) == before


def test_track_files_one_warning_drops_the_index_of_every_class(tmp_path, caplog):
    """Three classes, and a name that comes back in a later write: one warning for the input, no `.tbi`, the stale `.tbi` of every
    class removed, and the `.gz` files those of a run without --track_index."""
    import logging
    classes = (1, 2, 3)
    writes = [_track_write(nms, _class_texts(nms, 3, seed)) for seed, nms in enumerate([[b"a", b"b"], [b"b", b"c"], [b"a"], [b"d"]])]
    with_index, without = tmp_path / "with", tmp_path / "without"
    with_index.mkdir()
    gz_names = [f"in.fa.class{c}.bedGraph.gz" for c in classes]
    for name in gz_names:
        (with_index / (name + ".tbi")).write_bytes(b"left by an earlier run")
    with caplog.at_level(logging.WARNING):
        for directory, index in ((with_index, True), (without, False)):
            files = _track_files(directory, classes, index)
            for w in writes:
                files.write(w)
            files.commit()
    warned = [r.getMessage() for r in caplog.records]
    assert len(warned) == 1 and "in.fa: no tabix index is written (--track_index)" in warned[0] and "'a' reappears after another name" in warned[0]
    assert sorted(os.listdir(with_index)) == gz_names
    assert _listing(with_index) == _listing(without)
    assert all(len(data) > 28 for data in _listing(without).values())                   # (more than the EOF member)


# ------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


def _err(L):
    return L.dgrp_last_error().decode("utf-8", "replace")


def _call(L, C_=5, nrec=2, row0=(0, 64), n=(10, 20), spos=(0, 3), names=b"abcd", name_off=(0, 2, 4), cls=(1, 2), ncls=None, digits=2,
          bin=1, cap=0, lcap=1 << 20, chunk_off=True, linear=0x1000):
    """dgrp_track_index_batch with host tables only (every device pointer is a dummy that a refusal never touches)."""
    r0, nn, sp = (np.array(x, np.int64) for x in (row0, n, spos))
    no = np.array(name_off, np.int64)
    cl = np.array(cls, np.int32)
    ncls = len(cls) if ncls is None else ncls
    off = np.full(max(ncls, 0) + 1 + 64, -7, np.int64)
    rc = L.dgrp_track_index_batch(0x1000, C_, nrec, r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, names, no.ctypes.data, cl.ctypes.data, ncls,
                                  digits, bin, None, cap, off.ctypes.data if chunk_off else None, linear, lcap, 0x1000, 1 << 40, None)
    return rc, off


def test_the_two_symbols_are_exported_and_bound(L):
    from deepgrp_amd import _lib
    for name in ("dgrp_track_index_workspace_bytes", "dgrp_track_index_batch"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name


@pytest.mark.parametrize("kw,words", [
    (dict(nrec=-1), ("bad nrec", "-1")),
    (dict(C_=0), ("bad C",)),
    (dict(cls=(), ncls=0), ("ncls must lie in 1..C",)),
    (dict(cls=(1, 5)), ("class 5", "0..4")),
    (dict(digits=5), ("digits must lie in 1..4", "5")),
    (dict(bin=0), ("bad bin 0",)),
    (dict(cap=-1), ("bad chunk_cap",)),
    (dict(lcap=-1), ("bad chunk_cap/linear_cap",)),
    (dict(n=(10, 0)), ("record 1", "bad n 0")),
    (dict(spos=(0, -2)), ("record 1", "bad offset -2")),
    (dict(row0=(0, -64)), ("record 1", "bad first row")),
    (dict(name_off=(0, 3, 2)), ("record 1", "descending name offsets")),
    (dict(chunk_off=False), ("NULL h_chunk_off",)),
    (dict(names=None), ("NULL pointer",)),
    (dict(linear=None), ("NULL pointer",)),
    (dict(cap=5), ("NULL pointer",)),                                  # d_chunks may be NULL only with chunk_cap 0
    (dict(lcap=3), ("linear_cap 3 < 4",)),                             # two records of one window, two classes
    (dict(n=(10, 20_001), spos=(0, (1 << 29) - 20_000)), ("record 1", "ends at 536870913", "2^29")),
    (dict(n=(10, 1), spos=(0, 1 << 29)), ("record 1", "above 2^29")),
])
def test_refusals_name_the_entry_and_the_record(L, kw, words):
    rc, off = _call(L, **kw)
    msg = _err(L)
    assert rc == EINVAL, (kw, rc, msg)
    assert msg.startswith("dgrp_track_index_batch: "), msg
    for w in words:
        assert w in msg, (kw, msg)
    if kw.get("chunk_off", True) and "C_" not in kw and "ncls" not in kw:
        assert off[:3].tolist() == [0, 0, 0] and (off[3:] == -7).all()                 # filled in full in front of the refusal


def test_an_empty_batch_and_the_workspace(L):
    rc, off = _call(L, nrec=0, cls=(3, 1, 0), linear=None, lcap=0)
    assert rc == 0 and off[:4].tolist() == [0, 0, 0, 0] and (off[4:] == -7).all(), _err(L)

    def wb(query, n=(1000, 2000), spos=(0, 5), bin=1, ncls=2, names=10):
        nn, sp = np.array(n, np.int64), np.array(spos, np.int64)
        return query(len(n), nn.ctypes.data, sp.ctypes.data, bin, ncls, names)
    text, index = L.dgrp_track_batch_workspace_bytes, L.dgrp_track_index_workspace_bytes
    assert wb(index) > wb(text) > 0                                                    # the text chain's workspace and the index's parts
    assert wb(index, n=(100_000, 2000)) - wb(text, n=(100_000, 2000)) < 100_000 * 2 * 4 // 10      # per tile, not per bin
    top = 1 << 29
    assert wb(index, n=(1000, 20_000), spos=(0, top - 20_000)) > 0 and wb(index, n=(1000, 20_001), spos=(0, top - 20_000)) == 0
    assert wb(text, n=(1000, 20_001), spos=(0, top - 20_000)) > 0                      # the text has no such limit
    for bad in (dict(bin=0), dict(ncls=0), dict(names=-1), dict(n=(1000, 0)), dict(spos=(0, -1))):
        assert wb(index, **bad) == 0, bad


# ------------------------------------------------------------------------------------------ the command line
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
    for argv in (["predict", model, str(fa), "--track_dir", tdir, "--track_index", "--output", out],
                 ["predict", model, str(fa), "--track_index", "--output", out],
                 ["--track_index", "--track_dir", tdir, model, str(fa), "--output", out]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert "--track_index needs --track_gzip" in str(e.value.code), argv
    with pytest.raises(SystemExit) as e:
        main(["--track_index", "evaluate", model, str(ann), str(fa), "--output", out])
    assert "belongs to predict" in str(e.value.code)
    assert not os.path.exists(tdir) and not os.path.exists(out)
    args = lambda argv: CommandLineParser().parse_args(argv).args
    plan = tracks.plan(args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_gzip", "--track_index"]))
    assert plan.index and tracks.resolve(plan, 5).index and tracks.resolve(plan, 5).gzip_level == 1
    plan = tracks.plan(args(["predict", "m.h5", "x.fa", "--track_dir", "d", "--track_gzip"]))
    assert not plan.index and not tracks.resolve(plan, 5).index
