"""The CSI index without a GPU: the binning scheme at depth 6 and its tie to the `.tbi` scheme, csi_payload / read_csi, the loffset
rule against the `.tbi` statement's linear index, csi_query against a brute-force filter (with the offsets and with the bins alone),
IndexBuilder(fmt="csi") on pieces computed in Python, the refusals of --index_format before the model is read, the three new
symbols, and BgzfSink's handling of the `.csi` file and of a stale index of the other format."""
import os
import struct
import zlib

import numpy as np
import pytest

from csi_cases import FIRST5, FIRST6, MIN_SCORE, NBINS6, REFUSED_SPAN, SPANS, T29, T31, T32, corpus, scan, track_like, writes
from deepgrp_amd import bed, gff, gz, outfiles, tabix


def test_constants_and_bins_of_the_hand_written_spans():
    assert tabix.CSI_DEPTH == 6 and tabix.csi_max_end(6) == T32 and tabix.csi_max_end(5) == T29 == tabix.MAX_END
    assert tuple(((1 << 3 * l) - 1) // 7 for l in range(7)) == FIRST6 and FIRST6[6] + (1 << 18) == NBINS6
    for beg, end, b6, b5 in SPANS:
        assert tabix.csi_reg2bin(beg, end, 6) == b6, (beg, end)
        assert b6 in tabix.csi_reg2bins(beg, end, 6) and 0 <= b6 < NBINS6
        if b5 is not None:
            assert tabix.csi_reg2bin(beg, end, 5) == b5 == tabix.reg2bin(beg, end), (beg, end)
        else:
            with pytest.raises(tabix.IndexRefused):
                tabix.csi_reg2bin(beg, end, 5)
    with pytest.raises(tabix.IndexRefused, match=r"2\^32"):
        tabix.csi_reg2bin(*REFUSED_SPAN, 6)
    assert tabix.csi_reg2bin(0, T32) == 0                               # depth 6 is the default


def test_depth_5_is_reg2bin_and_depth_6_renumbers_it_below_2_29():
    rng = np.random.default_rng(11)
    for _ in range(2000):
        beg = int(rng.integers(0, T29))
        end = min(T29, beg + 1 + int(2 ** rng.uniform(0, 29)))
        b5 = tabix.reg2bin(beg, end)
        assert tabix.csi_reg2bin(beg, end, 5) == b5
        level = max(l for l in range(6) if FIRST5[l] <= b5)
        assert tabix.csi_reg2bin(beg, end, 6) == FIRST6[level + 1] + (b5 - FIRST5[level])
        assert tabix.csi_reg2bins(beg, end, 5) == tabix.reg2bins(beg, end)
    assert tabix.csi_bottom_window(0) == 0 and tabix.csi_bottom_window(2) == 1 << 15 and tabix.csi_bottom_window(NBINS6 - 1) == (1 << 18) - 1
    assert tabix.csi_bottom_window(4681 + 3) == 24 and tabix.csi_bottom_window(4681 + 3, 5) == 3


def _renumber(b5):
    level = max(l for l in range(6) if FIRST5[l] <= b5)
    return FIRST6[level + 1] + (b5 - FIRST5[level])


def _small_file(seed=3, names=(b"chrA", b"chrB"), lines_per=150, top=6_000_000):
    rng = np.random.default_rng(seed)
    out = []
    for nm in names:
        starts = np.sort(rng.integers(0, top, lines_per))
        for s in starts.tolist():
            width = int(rng.choice([1, 30, 900, 20_000, 400_000]))
            out.append(b"%s\t%d\t%d\t0.5\n" % (nm, s, s + width))
    text = b"".join(out)
    return text, gz.bgzf_compress(text, block=2048)                    # many members: virtual offsets cross them


def test_the_same_chunks_per_renumbered_bin_and_loffset_is_ioff_of_the_bottom_window():
    text, data = _small_file()
    tbi = tabix.read_index(tabix.reference_index(data))
    pl = tabix.csi_reference_index(data)
    csi = tabix.read_csi(pl)
    assert csi["names"] == tbi["names"] == [b"chrA", b"chrB"] and csi["depth"] == 6 and csi["preset"] == tabix.PRESET_BED
    for b5, b6, lin in zip(tbi["bins"], csi["bins"], tbi["linear"]):
        assert {_renumber(k): v for k, v in b5.items()} == {k: v[1] for k, v in b6.items()}
        assert len(b6) > 20
        for k, (loff, _chunks) in b6.items():
            w = tabix.csi_bottom_window(k, 6)
            assert w < len(lin) and loff == int(lin[w]), k
    # at depth 5 the bins are the .tbi's own
    five = tabix.read_csi(tabix.csi_reference_index(data, tabix.PRESET_BED, 5))
    assert [{k: v[1] for k, v in b.items()} for b in five["bins"]] == tbi["bins"] and five["depth"] == 5


def test_payload_bytes_and_round_trip():
    bins = [{0: [(5, 9)], 37449: [(1 << 16, 2 << 16), (3 << 16 | 7, 9 << 16)]}, {299592: [(10 << 16, 11 << 16)]}]
    loffs = [{0: 5, 37449: 1 << 16}, {299592: 77}]
    pl = tabix.csi_payload([b"a", b"bc"], bins, loffs, tabix.PRESET_GFF, 6)
    want = b"CSI\1" + struct.pack("<3i", 14, 6, 28 + 5) + struct.pack("<7i", 0, 1, 4, 5, ord("#"), 0, 5) + b"a\0bc\0" + struct.pack("<i", 2)
    want += struct.pack("<i", 2) + struct.pack("<IQi", 0, 5, 1) + struct.pack("<2Q", 5, 9)
    want += struct.pack("<IQi", 37449, 1 << 16, 2) + struct.pack("<4Q", 1 << 16, 2 << 16, 3 << 16 | 7, 9 << 16)
    want += struct.pack("<i", 1) + struct.pack("<IQi", 299592, 77, 1) + struct.pack("<2Q", 10 << 16, 11 << 16) + struct.pack("<Q", 0)
    assert pl == want
    got = tabix.read_csi(pl)
    assert got == {"names": [b"a", b"bc"], "depth": 6, "preset": tabix.PRESET_GFF,
                   "bins": [{k: (loffs[s][k], v) for k, v in b.items()} for s, b in enumerate(bins)]}
    with pytest.raises(ValueError):
        tabix.read_csi(pl[:-9])
    with pytest.raises(ValueError):
        tabix.read_csi(b"TBI\1" + pl[4:])
    assert zlib.decompress(tabix.index_file(pl), 31) == pl


def test_csi_query_agrees_with_a_scan_with_and_without_the_offsets():
    rng = np.random.default_rng(7)
    out = []
    for nm, base in ((b"low", 0), (b"mid", T29 - 3_000_000), (b"high", T31 - 3_000_000), (b"top", T32 - 6_100_000)):
        for s in np.sort(rng.integers(40_000, 6_000_000, 120)).tolist():              # (the first window is empty)
            out.append(b"%s\t%d\t%d\tx\n" % (nm, base + s, base + s + int(rng.choice([1, 30, 900, 20_000, 90_000]))))
    text = b"".join(out)
    data = gz.bgzf_compress(text, block=4096)
    ix = tabix.read_csi(tabix.csi_reference_index(data))
    lines = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    regions = [(b"low", 0, 1), (b"low", 0, 50_000), (b"low", 16_000, 16_500), (b"low", 7_000_000, 7_000_001), (b"top", T32 - 5, T32),
               (b"mid", T29 - 1, T29 + 1), (b"high", T31 - 1, T31 + 1), (b"mid", 0, T32), (b"high", T32 - 1, T32), (b"none", 0, T32)]
    for _ in range(200):
        nm, base = [(b"low", 0), (b"mid", T29 - 3_000_000), (b"high", T31 - 3_000_000), (b"top", T32 - 6_100_000)][int(rng.integers(0, 4))]
        beg = base + int(rng.integers(0, 6_200_000))
        regions.append((nm, beg, beg + int(rng.choice([1, 10, 500, 20_000, 200_000, 3_000_000]))))
    found = 0
    for nm, beg, end in regions:
        want = scan(lines, nm, beg, end)
        assert tabix.csi_query(ix, data, nm, beg, end) == want, (nm, beg, end)         # the offsets lose no line
        assert tabix.csi_query(ix, data, nm, beg, end, use_loffset=False) == want      # the bins alone lose none
        found += len(want)
    assert found > 100
    # the offsets do cut: a region far up a sequence starts reading behind the lines in front of it
    bins = ix["bins"][0]
    assert tabix.csi_min_off(bins, 5_900_000, 6) > tabix.csi_min_off(bins, 100_000, 6) >= 0 == tabix.csi_min_off(bins, 0, 6)


def _python_pieces(names, rows, scores, rec_end, depth, gff3=False, id0=0):
    if gff3:
        text, n = gff.reference_lines(names, True, rows, scores, MIN_SCORE, None, id0)
        return text, n, gff.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, None, id0, depth)
    text = bed.reference_lines(names, True, rows, scores, MIN_SCORE)
    return text, text.count(b"\n"), bed.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, depth)


@pytest.mark.parametrize("gff3", [False, True])
@pytest.mark.parametrize("split", [False, True])
def test_index_builder_csi_on_python_pieces_is_the_reference_of_the_file(gff3, split):
    names, rows, scores, rec_end = corpus()
    preset = gff.PRESET if gff3 else tabix.PRESET_BED
    builder = tabix.IndexBuilder(preset, "csi", 6)
    data = gz.bgzf_compress(gff.HEADER, eof=False, block=4096) if gff3 else b""
    done = 0
    for nm, r, s, e in (writes(names, rows, scores, rec_end) if split else [(names, rows, scores, rec_end)]):
        text, n, (chunks, linear, wpref, last) = _python_pieces(nm, r, s, e, 6, gff3, done)
        done += n
        members = gz.bgzf_compress(text, eof=False, block=tabix.BLOCK)
        sizes, text_len = tabix.member_sizes(members)
        builder.add(len(data), sizes, text_len, nm, chunks, linear, wpref, last)
        data += members
    data += gz.BGZF_EOF
    pl = builder.payload()
    assert pl == tabix.csi_reference_index(data, preset)
    ix = tabix.read_csi(pl)
    assert ix["names"] == [b"chrBig", b"twin", b"tail"] and ix["preset"] == preset
    assert {0, 1, 299592, 37449 + 32767, 37449 + 32768, 37449 + 131071, 37449 + 131072} <= set(ix["bins"][0])
    lines = [ln.split(b"\t") for ln in b"".join(_members(data)).split(b"\n")[:-1] if not ln.startswith(b"#")]
    cols = (0, 3, 4) if gff3 else (0, 1, 2)
    found = 0
    for nm, beg, end in [(b"chrBig", 0, T32), (b"chrBig", 35, 75), (b"chrBig", T29 - 1, T29), (b"chrBig", T29, T29 + 1), (b"chrBig", T31 - 2, T31 - 1),
                         (b"chrBig", T31 + 1, T31 + 2), (b"chrBig", T32 - 1, T32), (b"chrBig", 2_999_999_999, 3_000_000_001),
                         (b"chrBig", 3_500_000_000, 3_500_000_001), (b"twin", 0, 10), (b"twin", T29 + 15, T29 + 16), (b"twin", T31, T31 + 5),
                         (b"twin", 16_384, 16_385), (b"tail", 0, 10), (b"quiet", 0, 1000)]:
        want = scan(lines, nm, beg, end, cols, one_based=gff3)
        assert tabix.csi_query(ix, data, nm, beg, end) == want, (nm, beg, end)
        assert tabix.csi_query(ix, data, nm, beg, end, use_loffset=False) == want
        found += len(want)
    assert found > 30


def _members(data):
    off = 0
    while off < len(data):
        d = zlib.decompressobj(31)
        yield d.decompress(data[off:])
        off = len(data) - len(d.unused_data)


def test_index_builder_defaults_and_refusals():
    names, rows, scores, rec_end = corpus()
    with pytest.raises(ValueError):
        tabix.IndexBuilder(tabix.PRESET_BED, "bai")
    with pytest.raises(ValueError):
        tabix.IndexBuilder(tabix.PRESET_BED, "tbi", 6)
    assert tabix.IndexBuilder().fmt == "tbi" and tabix.IndexBuilder().payload() == tabix.payload([], [], [])
    assert tabix.IndexBuilder(fmt="csi", depth=6).payload() == tabix.csi_payload([], [], [])
    # the refusal texts: today's at depth 5, the CSI limit at depth 6
    assert tabix.end_refusal([T29 + 1]) == tabix.end_refusal([T29 + 1], None, 5) \
        == f"record 0 ends at {T29 + 1}, above 2^29, the largest coordinate of a tabix index"
    assert tabix.end_refusal([5, T32], [b"a", b"b"], 6) is None and tabix.end_refusal([T29 + 1], None, 6) is None
    assert tabix.end_refusal([5, T32 + 1], [b"a", b"b"], 6) \
        == f"record 'b' ends at {T32 + 1}, above 2^32 = {T32}, the largest coordinate of a CSI index of depth 6"
    with pytest.raises(tabix.IndexRefused, match="a CSI index"):
        tabix.window_prefix([T32 + 1], 6)
    assert tabix.window_prefix([T32, 1], 6).tolist() == [0, 1 << 18, (1 << 18) + 1]
    with pytest.raises(tabix.IndexRefused, match="tabix index"):
        tabix.window_prefix([T29 + 1])
    # a name that comes back is refused as for a .tbi
    bad = [b"chrBig", b"quiet", b"norows", b"twin", b"chrBig", b"tail"]
    text = bed.reference_lines(bad, True, rows, scores, MIN_SCORE)
    with pytest.raises(tabix.IndexRefused, match="reappears"):
        tabix.csi_reference_index(gz.bgzf_compress(text))


def test_track_like_pieces_through_the_builder():
    """A bedGraph write of three records (two of one name, one without a line between them) at coordinates around 2^29 and 2^31."""
    recs = [b"a\t%d\t%d\t0.10\na\t%d\t%d\t0.20\n" % (T29 - 300, T29 - 2, T29 - 2, T29 + 300), b"",
            b"a\t%d\t%d\t0.30\n" % (T31 - 300, T31 + 300), b"b\t%d\t%d\t0.40\nb\t%d\t%d\t0.50\n" % (T32 - 600, T32 - 300, T32 - 300, T32)]
    chunks, linear = track_like(recs, 6)
    assert [c[3] for c in chunks] == [37449 + 32767, 0, 0, 299592]     # (records never share a chunk on the device)
    ends = [T29 + 300, T29 + 400, T31 + 300, T32]
    wpref = tabix.window_prefix(ends, 6)
    lin = np.full(int(wpref[-1]), -1, np.int64)
    for r, l in enumerate(linear):
        lin[wpref[r]:wpref[r] + len(l)] = l
    c = np.zeros(len(chunks), tabix.CHUNK_DTYPE)
    for i, ch in enumerate(chunks):
        c[i] = tuple(ch)
    text = b"".join(recs)
    members = gz.bgzf_compress(text, eof=False, block=tabix.BLOCK)
    b = tabix.IndexBuilder(tabix.PRESET_BED, "csi", 6)
    b.add(0, *tabix.member_sizes(members), [b"a", b"a", b"a", b"b"], c, lin, wpref)
    data = members + gz.BGZF_EOF
    assert b.payload() == tabix.csi_reference_index(data)
    ix = tabix.read_csi(b.payload())
    assert len(ix["bins"][0][0][1]) == 1                                # the two bin-0 lines of "a", a record apart: one chunk
    assert tabix.csi_query(ix, data, b"a", T29, T29 + 1) == [recs[0].split(b"\n")[1]]
    assert tabix.csi_query(ix, data, b"b", T32 - 1, T32) == [recs[3].split(b"\n")[1]]


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_model(monkeypatch):
    import torch
    from deepgrp_amd import model as dgmodel

    def touched(*_a, **_k):
        raise AssertionError("the model was read or torch.cuda was touched before the refusal")
    for name in ("is_available", "set_device", "current_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(dgmodel, "load_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_flag_refusals_before_the_model_is_read(no_model, tmp_path):
    model = str(tmp_path / "no_such_model.h5")
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    out = str(tmp_path / "out")
    need = "--index_format needs --track_index or --bed_index"
    _refused(["predict", model, str(fa), "--index_format", "csi"], need)
    _refused(["--index_format", "csi", model, str(fa)], need)                                      # the README form
    _refused(["predict", model, str(fa), "--index_format", "tbi"], need)                            # given is given
    _refused(["predict", model, str(fa), "--track_dir", out, "--track_gzip", "--index_format", "csi"], need)
    _refused(["predict", model, str(fa), "--bed_dir", out, "--bed_gzip", "--index_format", "csi"], need)
    _refused(["predict", model, str(fa), "--bed_dir", out, "--bed_index", "--index_format", "csi"], "--bed_index needs --bed_gzip")
    _refused(["--index_format", "csi", "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--index_format belongs to predict, not evaluate")
    with pytest.raises(SystemExit) as e:                                                            # argparse's own refusal of another value
        from deepgrp_amd.__main__ import main
        main(["predict", model, str(fa), "--bed_dir", out, "--bed_gzip", "--bed_index", "--index_format", "bai"])
    assert e.value.code == 2
    assert not os.path.exists(out)


def test_the_flag_reaches_the_plans(no_model, tmp_path):
    import argparse
    from deepgrp_amd import tracks
    ns = lambda **kw: argparse.Namespace(FASTA=[str(tmp_path / "a.fa")], **kw)
    p = bed.plan(ns(bed_dir=str(tmp_path / "b"), bed_gzip=True, bed_index=True, index_format="csi"))
    assert p.index and p.index_format == "csi"
    assert bed.plan(ns(bed_dir=str(tmp_path / "b"), bed_gzip=True, bed_index=True)).index_format == "tbi"
    assert bed.BedPlan("d", 0, {}) == bed.BedPlan("d", 0, {}, index_format="tbi")                  # appended last: earlier constructions hold
    t = tracks.plan(ns(track_dir=str(tmp_path / "t"), track_gzip=True, track_index=True, index_format="csi"))
    assert t.index and t.index_format == "csi" and tracks.resolve(t, 5).index_format == "csi"
    t = tracks.plan(ns(track_dir=str(tmp_path / "t"), track_gzip=True, track_index=True))
    assert t.index_format == "tbi" and tracks.resolve(t, 5) == tracks.TrackSpec((1, 2, 3, 4), 2, 1, 1, True, False)
    assert tracks.index_depth("csi") == 6 and tracks.index_depth("tbi") == 5


def test_symbols_declared_bound_and_exported():
    from deepgrp_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_track_csi_batch", "dgrp_bed_csi_batch", "dgrp_gff_csi_batch"):
        for sym in (name, name.replace("_batch", "_workspace_bytes")):
            assert sym in _lib.exported_symbols() and hasattr(L, sym) and sym + "(" in header, sym
            assert getattr(L, sym).argtypes is not None
    # the workspace twins take the depth: the .tbi entries' figures at 5 and 6, 0 at any other
    assert L.dgrp_bed_csi_workspace_bytes(50, 2, 9, 2, 6) == L.dgrp_bed_csi_workspace_bytes(50, 2, 9, 2, 5) \
        == L.dgrp_bed_index_workspace_bytes(50, 2, 9, 2) > 0
    assert L.dgrp_gff_csi_workspace_bytes(50, 2, 9, 3, 12, 2, 6) == L.dgrp_gff_index_workspace_bytes(50, 2, 9, 3, 12, 2) > 0
    assert L.dgrp_bed_csi_workspace_bytes(50, 2, 9, 2, 4) == 0 == L.dgrp_gff_csi_workspace_bytes(50, 2, 9, 3, 12, 2, 7)
    n, sp = np.array([600], np.int64), np.array([T32 - 600], np.int64)
    track = lambda depth: L.dgrp_track_csi_workspace_bytes(1, n.ctypes.data, sp.ctypes.data, 1, 2, 4, depth)
    assert track(6) > 0 and track(5) == 0 == track(7) == L.dgrp_track_index_workspace_bytes(1, n.ctypes.data, sp.ctypes.data, 1, 2, 4)
    sp[0] += 1
    assert track(6) == 0                                                # one base above 2^32


def test_entries_refuse_depth_and_end_on_the_host():
    """A depth other than 5 or 6 and a record end above 2^(14 + 3 depth): DGRP_EINVAL from the host checks, no device pointer read."""
    import ctypes as C
    from deepgrp_amd._lib import lib
    L = lib()
    got = C.c_int64(-7)
    off = np.array([0, 3], np.int64)

    def index(end, depth, entry="bed"):
        e = np.array([end], np.int64)
        if entry == "bed":
            return L.dgrp_bed_csi_batch(b"abc", off.ctypes.data, 1, 1, None, None, 0, 0, 1, e.ctypes.data, depth, None, 0, C.byref(got), None, 0,
                                        None, None, 0, None)
        return L.dgrp_gff_csi_batch(b"abc", off.ctypes.data, 1, 1, None, None, 0, None, None, 0, 0, 0, 1, e.ctypes.data, depth, None, 0,
                                    C.byref(got), None, 0, None, None, 0, None)
    for entry in ("bed", "gff"):
        assert index(T32, 6, entry) == 0 and got.value == 0             # no rows: nothing to do
        assert index(T29, 5, entry) == 0
        assert index(T32 + 1, 6, entry) == -1
        msg = L.dgrp_last_error().decode()
        assert f"dgrp_{entry}_csi_batch" in msg and "a CSI index" in msg and "2^32 = 4294967296" in msg and str(T32 + 1) in msg, msg
        assert index(T29 + 1, 5, entry) == -1 and "2^29 = 536870912" in L.dgrp_last_error().decode() and "a CSI index" in L.dgrp_last_error().decode()
        assert index(100, 7, entry) == -1 and "depth must be 5 or 6" in L.dgrp_last_error().decode()
        assert index(100, 0, entry) == -1
    # the old entry keeps its words
    e = np.array([T29 + 1], np.int64)
    assert L.dgrp_bed_index_batch(b"abc", off.ctypes.data, 1, 1, None, None, 0, 0, 1, e.ctypes.data, None, 0, C.byref(got), None, 0, None, None, 0,
                                  None) == -1
    assert b"outside 1..2^29 (the largest coordinate of a tabix index)" in L.dgrp_last_error()


# ---- BgzfSink ------------------------------------------------------------------------------------------------------------------------
def _sink_write(sink):
    text = b"a\t5\t9\tx\n"
    members = gz.bgzf_compress(text, eof=False)
    b = 37449 if sink.fmt == "csi" else 4681
    chunks = np.array([(0, len(text), 0, b)], tabix.CHUNK_DTYPE)
    sink.append(members, [b"a"], chunks, np.array([0], np.int64), np.array([0, 1], np.int64))
    return members + gz.BGZF_EOF


@pytest.mark.parametrize("fmt,other", [("csi", "tbi"), ("tbi", "csi")])
def test_sink_stages_commits_and_removes_the_stale_sibling(tmp_path, fmt, other):
    final = str(tmp_path / "x.bed.gz")
    stale = final + "." + other
    with open(stale, "wb") as fh:
        fh.write(b"an index of an earlier run")
    sink = outfiles.BgzfSink(final, True, fmt=fmt)
    data = _sink_write(sink)
    sink.finish()
    assert sorted(f for f in os.listdir(tmp_path) if not f.startswith(".")) == ["x.bed.gz." + other]       # staged: nothing in place yet
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".tmp")]) == 2
    sink.commit()
    assert sorted(os.listdir(tmp_path)) == ["x.bed.gz", "x.bed.gz." + fmt]                                 # the stale sibling is gone
    assert open(final, "rb").read() == data
    pl = zlib.decompress(open(final + "." + fmt, "rb").read(), 31)
    assert pl == (tabix.csi_reference_index(data) if fmt == "csi" else tabix.reference_index(data))


@pytest.mark.parametrize("fmt", ["csi", "tbi"])
def test_sink_abort_dropped_index_and_no_index_flag(tmp_path, fmt):
    final = str(tmp_path / "x.bed.gz")
    for suffix in (".tbi", ".csi"):
        with open(final + suffix, "wb") as fh:
            fh.write(b"earlier")
    # abort: no temporary file, and what an earlier run left is untouched
    sink = outfiles.BgzfSink(final, True, fmt=fmt)
    _sink_write(sink)
    sink.finish()
    sink.abort()
    assert sorted(os.listdir(tmp_path)) == ["x.bed.gz.csi", "x.bed.gz.tbi"]
    # without the index flag nothing beside the file is touched
    sink = outfiles.BgzfSink(final, False, fmt=fmt)
    _sink_write(sink)
    sink.finish()
    sink.commit()
    assert sorted(os.listdir(tmp_path)) == ["x.bed.gz", "x.bed.gz.csi", "x.bed.gz.tbi"]
    assert open(final + ".csi", "rb").read() == open(final + ".tbi", "rb").read() == b"earlier"
    # the index dropped on the way (a refused input): both files of an earlier run go, the data file stays
    sink = outfiles.BgzfSink(final, True, fmt=fmt)
    _sink_write(sink)
    sink.builder = None
    sink.finish()
    sink.commit()
    assert sorted(os.listdir(tmp_path)) == ["x.bed.gz"]


# ---- consecutive records of one name whose starts begin again ------------------------------------------------------------------------
def _descending_writes(kind, depth):
    """Two records named "x", one write each: the first has its lines at 50 kb (window 3), the second at 100 bp, so the sequence's
    last line starts in front of an earlier one and n_intv is 1 -> [(names, text, chunks, linear, wpref, last_end or None)]"""
    if kind == "track":
        recs = [b"x\t50000\t50100\t0.10\nx\t50100\t50200\t0.20\n", b"x\t100\t200\t0.30\n"]
        out = []
        for t, end in zip(recs, (50_200, 200)):
            chunks, linear = track_like([t], depth)
            c = np.zeros(len(chunks), tabix.CHUNK_DTYPE)
            for i, ch in enumerate(chunks):
                c[i] = tuple(ch)
            wpref = tabix.window_prefix([end], depth)
            lin = np.full(int(wpref[-1]), -1, np.int64)
            lin[:len(linear[0])] = linear[0]
            out.append(([b"x"], t, c, lin, wpref, None))
        return out
    from csi_cases import _rows_and_scores
    out = []
    for rows, end in (([(50_000, 50_100, 1, 0), (50_100, 66_000, 2, 0)], 70_000), ([(100, 200, 1, 0)], 300)):
        seg, sc = _rows_and_scores(rows, [False] * len(rows))
        text = bed.reference_lines([b"x"], True, seg, sc, MIN_SCORE)
        c, lin, wpref, last = bed.reference_index_parts([b"x"], True, seg, sc, MIN_SCORE, [end], depth)
        out.append(([b"x"], text, c, lin, wpref, last))
    return out


@pytest.mark.parametrize("kind", ["track", "bed"])
@pytest.mark.parametrize("fmt", ["tbi", "csi"])
def test_one_name_whose_starts_begin_again_is_indexed_in_both_formats(tmp_path, caplog, fmt, kind):
    import logging
    final = str(tmp_path / "x.gz")
    files = outfiles.StagedOutputs(logging.getLogger("csi_test"), "in.fa", "--bed_index", True, [outfiles.BgzfSink(final, True, fmt=fmt)])
    lines = []
    with caplog.at_level(logging.WARNING):
        for names, text, chunks, lin, wpref, last in _descending_writes(kind, 6 if fmt == "csi" else 5):
            assert files.name_order(names) is None                     # the same name twice in a row is one sequence
            files.append(0, gz.bgzf_compress(text, eof=False), names, chunks, lin, wpref, last)
            lines += [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
        files.commit()
    assert not caplog.records and files.indexed
    assert sorted(os.listdir(tmp_path)) == ["x.gz", "x.gz." + fmt]
    data = open(final, "rb").read()
    pl = zlib.decompress(open(final + "." + fmt, "rb").read(), 31)
    regions = [(0, 1), (0, 1000), (150, 151), (16_384, 16_385), (49_000, 50_001), (50_050, 50_150), (65_999, 66_000), (70_000, 80_000), (0, T32)]
    if fmt == "tbi":
        assert pl == tabix.reference_index(data) and len(tabix.read_index(pl)["linear"][0]) == 1
        return
    assert pl == tabix.csi_reference_index(data)
    ix = tabix.read_csi(pl)
    assert ix["names"] == [b"x"] and 37449 + 3 in ix["bins"][0]          # a bin whose bottom window lies behind n_intv = 1 ...
    first = min(c[0] for _l, cs in ix["bins"][0].values() for c in cs)
    assert ix["bins"][0][37449 + 3][0] == first                           # ... has the begin of the first line that ends above it
    for beg, end in regions:
        want = scan(lines, b"x", beg, end)
        assert tabix.csi_query(ix, data, b"x", beg, end) == want, (beg, end)
        assert tabix.csi_query(ix, data, b"x", beg, end, use_loffset=False) == want
