"""dgrp_track_csi_batch, dgrp_bed_csi_batch and dgrp_gff_csi_batch on the GPU.  At depth 5 their outputs are those of the `.tbi`
entries bit for bit, on the case shapes of tests/test_gpu_track_index.py and the corpora of tests/test_gpu_bed_index.py and
tests/test_gpu_gff_index.py.  At depth 6 the chunks and linear arrays equal restatements in Python integers at coordinates on both
sides of 2^29 and 2^31 and up to 2^32 (the shapes are small: the large numbers are start positions and row coordinates); through
tabix.IndexBuilder(fmt="csi"), with members from a real deflate of the device's text, they give tabix.csi_reference_index of the
finished file, and tabix.csi_query answers what a scan of the lines answers.  Refusals, a chunk capacity too small and the bytes
behind the exact capacities are checked on poisoned buffers."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bed_device as bd  # noqa: E402
import gff_device as gd  # noqa: E402
from csi_cases import MIN_SCORE, T29, T31, T32, corpus, scan, tbi_corpus, track_like, writes  # noqa: E402
from deepgrp_amd import bed, gff, gz, tabix  # noqa: E402
from deepgrp_amd._lib import lib, name_blob  # noqa: E402
from deepgrp_amd.pipeline import stream_ptr  # noqa: E402
from tabix_corpus import noisy  # noqa: E402

C5, DIGITS = 5, 2
GUARD = 0x5a
EINVAL = -1


# ---- tracks --------------------------------------------------------------------------------------------------------------------------
def _tables(n, spos, names, cls):
    nn, sp = (np.ascontiguousarray(x, np.int64) for x in (n, spos))
    noff = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(x) for x in names], out=noff[1:])
    return nn, sp, noff, b"".join(names), np.ascontiguousarray(cls, np.int32)


def _track_text(d_probs, row0, n, spos, names, cls, bin):
    """dgrp_track_text_batch -> (text, class offsets)"""
    L = lib()
    nn, sp, noff, blob, cl = _tables(n, spos, names, cls)
    r0 = np.ascontiguousarray(row0, np.int64)
    wb = L.dgrp_track_batch_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=d_probs.device)
    off = np.full(len(cl) + 1, -1, np.int64)
    text = None
    for _ in range(2):
        cap = max(int(off[-1]), 0)
        text = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_probs.device)
        assert L.dgrp_track_text_batch(d_probs.data_ptr(), C5, len(nn), r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data,
                                       cl.ctypes.data, len(cl), DIGITS, bin, text.data_ptr(), cap, off.ctypes.data, work.data_ptr(), wb,
                                       stream_ptr()) == 0, L.dgrp_last_error()
    return text.cpu().numpy().tobytes()[:int(off[-1])], off


def _track_index(depth, d_probs, row0, n, spos, names, cls, bin, short=0):
    """depth None: dgrp_track_index_batch; else dgrp_track_csi_batch at that depth.  Three calls on poisoned buffers: chunk_cap 0
    (counts only), `short` below the count where asked (nothing written), the exact capacities (nothing behind them)
    -> (chunks, chunk offsets, linear [classes, windows], window prefix)"""
    L = lib()
    nn, sp, noff, blob, cl = _tables(n, spos, names, cls)
    r0 = np.ascontiguousarray(row0, np.int64)
    dev = d_probs.device
    wpref = np.zeros(len(nn) + 1, np.int64)
    np.cumsum(((sp + nn - 1) >> 14) + 1, out=wpref[1:])
    nwin = int(wpref[-1]) * len(cl)
    if depth is None:
        wb = L.dgrp_track_index_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob))
    else:
        wb = L.dgrp_track_csi_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob), depth)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    linear = torch.full((nwin + 16,), GUARD, dtype=torch.int64, device=dev)
    off = np.full(len(cl) + 1, -1, np.int64)

    def call(chunks, cap):
        head = (d_probs.data_ptr(), C5, len(nn), r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data, cl.ctypes.data, len(cl),
                DIGITS, bin)
        tail = (chunks.data_ptr(), cap, off.ctypes.data, linear.data_ptr(), nwin, work.data_ptr(), wb, stream_ptr())
        rc = L.dgrp_track_index_batch(*head, *tail) if depth is None else L.dgrp_track_csi_batch(*head, depth, *tail)
        assert rc == 0, L.dgrp_last_error()
    size = tabix.CHUNK_DTYPE.itemsize
    probe = torch.full((64 * size,), GUARD, dtype=torch.uint8, device=dev)
    call(probe, 0)
    total = int(off[-1])
    counts = off.copy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and total > 0
    assert (probe.cpu().numpy() == GUARD).all() and (linear.cpu().numpy() == GUARD).all()          # the counts alone: nothing written
    if short:
        call(probe, total - short)                                      # too small: nothing written
        assert (off == counts).all() and (probe.cpu().numpy() == GUARD).all() and (linear.cpu().numpy() == GUARD).all()
    chunks = torch.full(((total + 4) * size,), GUARD, dtype=torch.uint8, device=dev)
    call(chunks, total)
    assert (off == counts).all()
    host, lin = chunks.cpu().numpy(), linear.cpu().numpy()
    assert (host[total * size:] == GUARD).all() and (lin[nwin:] == GUARD).all()                  # nothing behind the exact capacities
    return host[:total * size].view(tabix.CHUNK_DTYPE).copy(), off.copy(), lin[:nwin].reshape(len(cl), -1).copy(), wpref


def _noisy_probs(n, seed, step=4):
    p = np.zeros((n, C5), np.float32)
    for c in range(1, C5):
        p[:, c] = noisy(n, seed * 10 + c, step)
    return p


def _batch(nrec=300, seed=5):
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 3001, size=nrec)
    n[:3] = (1, 3000, 2)
    spos = rng.integers(0, 70_001, size=nrec)
    row0 = np.zeros(nrec, np.int64)
    np.cumsum((n[:-1] + 63) // 64 * 64, out=row0[1:])
    probs = np.zeros((int(row0[-1] + n[-1]), C5), np.float32)
    names, k = [], 0
    for r in range(nrec):
        k += 0 if r % 5 in (1, 2) else 1
        names.append(b"contig_%d" % k)
        if r != 204:
            probs[row0[r]:row0[r] + n[r]] = _noisy_probs(int(n[r]), 100 + r, 3 + r % 5)
    return probs, row0, n, spos, names


def _old_shapes():
    """The case shapes of tests/test_gpu_track_index.py: (id, probs, row0, n, startpos, names, bin)."""
    name = b"NC_000001.11"
    for bin in (1, 50, 128):
        yield "noisy-bin%d" % bin, _noisy_probs(40_000, 1), [0], [40_000], [16_000], [name], bin
    p = _noisy_probs(40_000, 2)
    p[:, 1], p[:, 3] = 0.37, 0
    yield "one-line-over-twenty-tiles", p, [0], [40_000], [16_000], [name], 1
    n = 140_000
    p = np.zeros((n, C5), np.float32)
    for edge in (16_384, 131_072):
        p[edge - 300:edge, 1], p[edge:edge + 200, 1] = 0.3, 0.4
        p[edge - 50:edge + 70, 2] = 0.5
    p[:, 3], p[:, 4] = noisy(n, 33, 5), noisy(n, 34, 9)
    yield "window-edges", p, [0], [n], [0], [b"chr7"], 1
    yield ("batch-of-300",) + _batch() + (1,)
    p = _noisy_probs(20_000, 7)
    p[:, 4] = 0.99
    yield "ends-at-2^29", p, [0], [20_000], [T29 - 20_000], [b"chrT"], 1


@pytest.mark.parametrize("case", list(_old_shapes()), ids=lambda c: c[0])
def test_tracks_depth_5_is_the_tbi_entry_bit_for_bit(case):
    _id, probs, row0, n, spos, names, bin = case
    d_probs = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).cuda()
    old = _track_index(None, d_probs, row0, n, spos, names, (1, 2, 3, 4), bin)
    new = _track_index(5, d_probs, row0, n, spos, names, (1, 2, 3, 4), bin)
    for a, b in zip(old, new):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert len(old[0]) > 0


def _records(startposes, seed):
    """Records of 600 bases at `startposes`: two noisy classes, and in class 1 one value over rows 290..309 (a line across the
    middle of the record, where 2^29 and 2^31 fall)."""
    nrec = len(startposes)
    row0 = [640 * r for r in range(nrec)]
    probs = np.zeros((640 * nrec, C5), np.float32)
    for r in range(nrec):
        probs[row0[r]:row0[r] + 600] = _noisy_probs(600, seed + r, 3)
        probs[row0[r] + 290:row0[r] + 310, 1] = 0.37
    return probs, row0, [600] * nrec


def _check_tracks_depth_6(startposes, names, bin, seed):
    """-> per class (text, chunks, linear rows, wpref) after the comparison with the restatement over the text"""
    cls = (1, 2)
    probs, row0, n = _records(startposes, seed)
    d_probs = torch.from_numpy(probs).cuda()
    text, toff = _track_text(d_probs, row0, n, startposes, names, cls, bin)
    chunks, coff, linear, wpref = _track_index(6, d_probs, row0, n, startposes, names, cls, bin, short=1)
    assert wpref.tolist() == tabix.window_prefix([s + 600 for s in startposes], 6).tolist()
    out = []
    for k in range(len(cls)):
        t = text[toff[k]:toff[k + 1]]
        lines = t.split(b"\n")[:-1]
        rec_texts = [b"".join(ln + b"\n" for ln in lines if s <= int(ln.split(b"\t")[1]) < s + 600) for s in startposes]
        assert b"".join(rec_texts) == t and all(rec_texts)
        want_c, want_l = track_like(rec_texts, 6)
        got = chunks[coff[k]:coff[k + 1]]
        assert [list(map(int, c)) for c in got.tolist()] == want_c, (k, bin)
        for r, lin in enumerate(want_l):
            row = linear[k, wpref[r]:wpref[r + 1]]
            assert row[:len(lin)].tolist() == lin and (row[len(lin):] == -1).all(), (k, r)
        out.append((t, got, linear[k], wpref))
    return out


@pytest.mark.parametrize("bin", [1, 50])
@pytest.mark.parametrize("startpos", [0, T29 - 300, T31 - 300, T32 - 600], ids=["0", "2^29-300", "2^31-300", "2^32-600"])
def test_tracks_depth_6_one_record(startpos, bin):
    out = _check_tracks_depth_6([startpos], [b"chrZ"], bin, 3)
    bins = set(out[0][1]["bin"].tolist())
    if startpos in (T29 - 300, T31 - 300):
        assert 0 in bins                                                # the line across 2^29 / 2^31: the root at depth 6
    else:
        assert 0 not in bins and min(bins) >= 37449 + (startpos >> 14)
    if startpos == T32 - 600:
        assert max(bins) == 299592 and len(out[0][2]) == 1 << 18        # the record's first line owns all 262 144 windows
        assert len(set(out[0][2].tolist())) == 1


@pytest.mark.parametrize("bin", [1, 50])
def test_tracks_depth_6_three_records_through_the_builder(bin):
    """Three records in one call, two of one name; the device's pieces through IndexBuilder(fmt="csi") are the reference of the file."""
    startposes, names = [T29 - 300, T31 - 300, T32 - 600], [b"one", b"one", b"two"]
    for k, (text, chunks, linear, wpref) in enumerate(_check_tracks_depth_6(startposes, names, bin, 20)):
        members = gz.bgzf_compress(text, eof=False)
        b = tabix.IndexBuilder(tabix.PRESET_BED, "csi", 6)
        b.add(0, *tabix.member_sizes(members), names, chunks, linear, wpref)       # (offsets inside the class's slice: it is the write)
        data = members + gz.BGZF_EOF
        pl = b.payload()
        assert pl == tabix.csi_reference_index(data), (k, bin)
        ix = tabix.read_csi(pl)
        assert ix["names"] == [b"one", b"two"]
        lines = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
        found = 0
        for nm, beg, end in [(b"one", T29 - 5, T29 - 1), (b"one", T29, T29 + 5), (b"one", T29 - 1, T29 + 1), (b"one", T31 - 5, T31 - 1),
                             (b"one", T31 + 1, T31 + 200), (b"one", 0, T32), (b"two", T32 - 1, T32), (b"two", T32 - 600, T32 - 500),
                             (b"two", 0, 100), (b"one", T29 + 1000, T31 - 1000)]:
            want = scan(lines, nm, beg, end)
            assert tabix.csi_query(ix, data, nm, beg, end) == want, (nm, beg, end)
            found += len(want)
        assert found > 10


def test_tracks_a_record_one_base_above_the_limit_is_refused_with_nothing_touched():
    L = lib()
    probs, row0, n = _records([T32 - 600], 9)
    d_probs = torch.from_numpy(np.vstack([probs, probs[:1]])).cuda()
    for depth, sp, nn, words in ((6, T32 - 600, 601, ("record 0 ends at 4294967297", "2^32 = 4294967296", "a CSI index")),
                                 (5, T29 - 600, 601, ("record 0 ends at 536870913", "2^29 = 536870912", "a CSI index")),
                                 (7, 0, 600, ("depth must be 5 or 6",)), (4, 0, 600, ("depth must be 5 or 6",))):
        t_n, t_sp, noff, blob, cl = _tables([nn], [sp], [b"chrT"], (1, 2))
        r0, off = np.zeros(1, np.int64), np.full(3, -1, np.int64)
        buf = torch.full((1 << 16,), GUARD, dtype=torch.int64, device=d_probs.device)
        assert L.dgrp_track_csi_workspace_bytes(1, t_n.ctypes.data, t_sp.ctypes.data, 1, 2, 4, depth) == 0
        rc = L.dgrp_track_csi_batch(d_probs.data_ptr(), C5, 1, r0.ctypes.data, t_n.ctypes.data, t_sp.ctypes.data, blob, noff.ctypes.data,
                                    cl.ctypes.data, 2, DIGITS, 1, depth, buf.data_ptr(), 16, off.ctypes.data, buf.data_ptr(), 1 << 16,
                                    buf.data_ptr(), 1 << 19, stream_ptr())
        msg = L.dgrp_last_error().decode()
        assert rc == EINVAL and all(w in msg for w in words) and "dgrp_track_csi_batch" in msg, msg
        assert (buf.cpu().numpy() == GUARD).all()
    # the old entry keeps its words
    t_n, t_sp, noff, blob, cl = _tables([601], [T29 - 600], [b"chrT"], (1, 2))
    rc = L.dgrp_track_index_batch(d_probs.data_ptr(), C5, 1, r0.ctypes.data, t_n.ctypes.data, t_sp.ctypes.data, blob, noff.ctypes.data,
                                  cl.ctypes.data, 2, DIGITS, 1, buf.data_ptr(), 16, off.ctypes.data, buf.data_ptr(), 1 << 16, buf.data_ptr(),
                                  1 << 19, stream_ptr())
    assert rc == EINVAL and "above 2^29 = 536870912, the largest coordinate of a tabix index" in L.dgrp_last_error().decode()


def test_tracks_pipeline_method_takes_the_depth():
    from deepgrp_amd.pipeline import ContigPipeline
    probs, row0, n = _records([T31 - 300, T32 - 600], 4)
    d_probs = torch.from_numpy(probs).cuda()
    pipe = ContigPipeline.__new__(ContigPipeline)                       # the method needs no model
    got = pipe.track_index_batch_device(d_probs, row0, n, [T31 - 300, T32 - 600], [b"a", "b"], (1, 2), DIGITS, 1, depth=6)
    want = _track_index(6, d_probs, row0, n, [T31 - 300, T32 - 600], [b"a", b"b"], (1, 2), 1)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all()
    with pytest.raises(tabix.IndexRefused, match="record 1 ends at"):   # the default is the .tbi's limit
        pipe.track_index_batch_device(d_probs, row0, n, [0, T29], [b"a", b"b"], (1, 2), DIGITS, 1)
    with pytest.raises(tabix.IndexRefused, match="a CSI index"):
        pipe.track_index_batch_device(d_probs, row0, n, [0, T32 - 599], [b"a", b"b"], (1, 2), DIGITS, 1, depth=6)


# ---- BED and GFF3 --------------------------------------------------------------------------------------------------------------------
def _csi_call(kind, names, by_contig, rows, scores, min_score, rec_end, depth, chunk_cap=None, class_names=None, id0=0):
    """dgrp_bed_csi_batch / dgrp_gff_csi_batch on guarded arenas -> (rc, *h_nchunks, chunks, linear, last ends, workspace, wpref)"""
    L = lib()
    n, nrec = len(rows), len(rec_end)
    ends = np.ascontiguousarray(rec_end, np.int64)
    wpref = bd.window_prefix([min(max(int(e), 1), T32) for e in rec_end])
    nwin = int(wpref[-1])
    if chunk_cap is None:
        chunk_cap = max(n, 1)
    if kind == "bed":
        raw, blob, off = name_blob(names)
        wb = int(L.dgrp_bed_csi_workspace_bytes(n, len(raw), len(blob), nrec, 6 if depth not in (5, 6) else depth))
    else:
        raw, blob, off, cblob, coff, nc = gd.tables(names, class_names)
        wb = int(L.dgrp_gff_csi_workspace_bytes(n, len(raw), len(blob), nc, len(cblob or b""), nrec, 6 if depth not in (5, 6) else depth))
    assert wb > 0
    chunks, linear, last, work = bd.Arena(chunk_cap * tabix.CHUNK_DTYPE.itemsize), bd.Arena(nwin * 8), bd.Arena(nrec * 8), bd.Arena(wb)
    keep_r, p_rows = bd._upload(rows)
    keep_s, p_scores = bd._upload(scores)
    got = C.c_int64(-7)
    tail = (nrec, ends.ctypes.data, depth, chunks.ptr, chunk_cap, C.byref(got), linear.ptr, nwin, last.ptr, work.ptr, work.n, stream_ptr())
    if kind == "bed":
        rc = L.dgrp_bed_csi_batch(blob, off.ctypes.data, len(raw), int(by_contig), p_rows, p_scores, n, int(min_score), *tail)
    else:
        rc = L.dgrp_gff_csi_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, None if coff is None else coff.ctypes.data, nc,
                                  p_rows, p_scores, n, int(min_score), int(id0), *tail)
    torch.cuda.current_stream().synchronize()
    del keep_r, keep_s
    return rc, got.value, chunks, linear, last, work, wpref


def _reference_parts(kind, names, rows, scores, rec_end, depth, id0=0):
    if kind == "bed":
        return bed.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, depth)
    return gff.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, None, id0, depth)


def _device_text(kind, names, rows, scores, id0=0):
    if kind == "bed":
        want = bed.reference_lines(names, True, rows, scores, MIN_SCORE)
        rc, n, text, _work = bd.text_call(names, True, rows, scores, MIN_SCORE)
        lines = want.count(b"\n")
    else:
        want, lines = gff.reference_lines(names, True, rows, scores, MIN_SCORE, None, id0)
        rc, n, got_lines, text, _work = gd.text_call(names, True, rows, scores, MIN_SCORE, None, id0)
        assert got_lines == lines
    assert rc == 0 and n == len(want)
    got = text.body(n).cpu().numpy().tobytes()
    assert got == want                                                  # coordinates of ten digits in the device's text
    return got, lines


def _device_parts(kind, names, rows, scores, rec_end, depth, id0=0):
    """The entry's outputs after the comparison with the restatement."""
    rc, nchunks, chunks, linear, last, work, wpref = _csi_call(kind, names, True, rows, scores, MIN_SCORE, rec_end, depth, id0=id0)
    assert rc == 0, lib().dgrp_last_error()
    assert all(a.guards_intact() for a in (chunks, linear, last, work))
    c, lin, le = bd.index_parts(chunks, nchunks, linear, last)
    want_c, want_lin, want_wpref, want_le = _reference_parts(kind, names, rows, scores, rec_end, depth, id0)
    assert np.array_equal(wpref, want_wpref)
    assert nchunks == len(want_c) and np.array_equal(c, want_c)
    bad = np.flatnonzero(lin != want_lin)
    assert bad.size == 0, (bad[:5], lin[bad[:5]], want_lin[bad[:5]])
    assert np.array_equal(le, want_le)
    return c.copy(), lin.copy(), wpref, le.copy()


@pytest.mark.parametrize("split", [False, True], ids=["one-write", "two-writes"])
@pytest.mark.parametrize("kind", ["bed", "gff"])
def test_corpus_up_to_2_32_is_the_statement_and_the_reference_of_the_file(kind, split):
    names, rows, scores, rec_end = corpus()
    preset = gff.PRESET if kind == "gff" else tabix.PRESET_BED
    builder = tabix.IndexBuilder(preset, "csi", 6)
    data = gff.header_member(1) if kind == "gff" else b""
    whole, done = b"", 0
    for nm, r, s, e in (writes(names, rows, scores, rec_end) if split else [(names, rows, scores, rec_end)]):
        text, n = _device_text(kind, nm, r, s, done)
        c, lin, wpref, le = _device_parts(kind, nm, r, s, e, 6, done)
        done += n
        members = gz.bgzf_compress(text, eof=False)
        builder.add(len(data), *tabix.member_sizes(members), nm, c, lin, wpref, le)
        data += members
        whole += text
    data += gz.BGZF_EOF
    pl = builder.payload()
    assert pl == tabix.csi_reference_index(data, preset)
    ix = tabix.read_csi(pl)
    assert ix["names"] == [b"chrBig", b"twin", b"tail"] and ix["depth"] == 6
    assert {0, 1, 299592, 37449 + 32767, 37449 + 32768, 37449 + 131071, 37449 + 131072} <= set(ix["bins"][0])
    lines = [ln.split(b"\t") for ln in whole.split(b"\n")[:-1]]
    cols = (0, 3, 4) if kind == "gff" else (0, 1, 2)
    found = 0
    for nm, beg, end in [(b"chrBig", 0, T32), (b"chrBig", 35, 75), (b"chrBig", T29 - 1, T29), (b"chrBig", T29, T29 + 1), (b"chrBig", T29 + 1, T29 + 2),
                         (b"chrBig", T31 - 2, T31 - 1), (b"chrBig", T31 + 1, T31 + 2), (b"chrBig", T32 - 1, T32), (b"chrBig", 2_999_999_999, 3_000_000_001),
                         (b"chrBig", 3_500_000_000, 3_500_000_001), (b"twin", 0, 10), (b"twin", T29 + 15, T29 + 16), (b"twin", T31, T31 + 5),
                         (b"twin", 16_384, 16_385), (b"tail", 0, 10), (b"quiet", 0, 1000)]:
        want = scan(lines, nm, beg, end, cols, one_based=kind == "gff")
        assert tabix.csi_query(ix, data, nm, beg, end) == want, (nm, beg, end)
        assert tabix.csi_query(ix, data, nm, beg, end, use_loffset=False) == want
        found += len(want)
    assert found > 30


def _same(a, b):
    """Two index calls gave the same bytes in every output."""
    assert a[0] == b[0] == 0 and a[1] == b[1] > 0
    n = a[1] * tabix.CHUNK_DTYPE.itemsize
    assert a[2].body(n).cpu().numpy().tobytes() == b[2].body(n).cpu().numpy().tobytes()
    for i in (3, 4):
        assert a[i].body().cpu().numpy().tobytes() == b[i].body().cpu().numpy().tobytes()
    assert np.array_equal(a[6], b[6])


def test_bed_and_gff_depth_5_are_the_tbi_entries_bit_for_bit():
    names, rows, scores, rec_end = tbi_corpus()                         # inside 2^29: every level, a row ending at 2^29
    LOW = MIN_SCORE
    _same(bd.index_call(names, True, rows, scores, LOW, rec_end), _csi_call("bed", names, True, rows, scores, LOW, rec_end, 5))
    _same(gd.index_call(names, True, rows, scores, LOW, rec_end, None, 7), _csi_call("gff", names, True, rows, scores, LOW, rec_end, 5, id0=7))
    cn = [b"LTR", b"a;b", b"SINE", b"D", b"E"]
    _same(gd.index_call(names, True, rows, scores, 0, rec_end, cn, 0), _csi_call("gff", names, True, rows, scores, 0, rec_end, 5, class_names=cn))
    # below 2^29 the depth-6 chunks are those of depth 5 under other bin numbers, and the linear index is the same
    five, six = _csi_call("bed", names, True, rows, scores, LOW, rec_end, 5), _csi_call("bed", names, True, rows, scores, LOW, rec_end, 6)
    c5, l5, e5 = bd.index_parts(five[2], five[1], five[3], five[4])
    c6, l6, e6 = bd.index_parts(six[2], six[1], six[3], six[4])
    assert five[1] == six[1] and np.array_equal(l5, l6) and np.array_equal(e5, e6)
    for k in ("beg", "end", "rec"):
        assert np.array_equal(c5[k], c6[k])
    first5, first6 = (0, 1, 9, 73, 585, 4681), (0, 1, 9, 73, 585, 4681, 37449)
    for b5, b6 in zip(c5["bin"].tolist(), c6["bin"].tolist()):
        level = max(l for l in range(6) if first5[l] <= b5)
        assert b6 == first6[level + 1] + (b5 - first5[level])


def _untouched(out):
    rc, _n, chunks, linear, last, work, _w = out
    return chunks.untouched() and linear.untouched() and last.untouched() and work.guards_intact()


@pytest.mark.parametrize("kind", ["bed", "gff"])
def test_refusals_and_a_capacity_too_small_leave_the_outputs_untouched(kind):
    names, rows, scores, rec_end = corpus()

    def refused(words, depth=6, **kw):
        args = dict(rows=rows, scores=scores, rec_end=rec_end)
        args.update(kw)
        out = _csi_call(kind, names, True, args["rows"], args["scores"], MIN_SCORE, args["rec_end"], depth)
        msg = lib().dgrp_last_error()
        assert out[0] == EINVAL and all(w in msg for w in words) and _untouched(out), (words, msg)

    refused([b"a CSI index", b"2^32 = 4294967296", b"ends at 4294967297", b"dgrp_%s_csi_batch" % kind.encode()], rec_end=[T32 + 1] + rec_end[1:])
    refused([b"a CSI index", b"2^29 = 536870912"], depth=5)                               # the corpus at depth 5: above that limit
    refused([b"depth must be 5 or 6"], depth=7)
    refused([b"depth must be 5 or 6"], depth=0)
    refused([b"ends behind its record"], rec_end=[T32 - 1] + rec_end[1:])                 # a row ends at 2^32
    bad = rows.copy()
    bad["end"][-1] = bad["start"][-1]
    refused([b"start < 0 or start >= end"], rows=bad)
    bad = rows.copy()
    bad[[2, 3]] = bad[[3, 2]]
    refused([b"starts descend"], rows=bad)
    want = len(_reference_parts(kind, names, rows, scores, rec_end, 6)[0])
    assert want > 15
    out = _csi_call(kind, names, True, rows, scores, MIN_SCORE, rec_end, 6, chunk_cap=want - 1)
    assert out[0] == 0 and out[1] == want and _untouched(out)
    out = _csi_call(kind, names, True, rows, scores, MIN_SCORE, rec_end, 6, chunk_cap=want)           # the exact capacity is enough
    assert out[0] == 0 and out[1] == want and out[2].guards_intact()


def test_pipeline_methods_take_the_depth():
    from deepgrp_amd.pipeline import ContigPipeline
    names, rows, scores, rec_end = corpus()
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
    for g, w in zip(ContigPipeline.bed_index_batch(names, True, d_rows, d_scores, MIN_SCORE, rec_end, 6),
                    bed.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, 6)):
        assert np.array_equal(g, w)
    for g, w in zip(ContigPipeline.gff_index_batch(names, True, d_rows, d_scores, MIN_SCORE, rec_end, None, 3, depth=6),
                    gff.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, None, 3, 6)):
        assert np.array_equal(g, w)
    with pytest.raises(tabix.IndexRefused, match="tabix index"):        # the default is the .tbi's limit
        ContigPipeline.bed_index_batch(names, True, d_rows, d_scores, MIN_SCORE, rec_end)
    with pytest.raises(tabix.IndexRefused, match="a CSI index"):
        ContigPipeline.gff_index_batch(names, True, d_rows, d_scores, MIN_SCORE, [T32 + 1] + rec_end[1:], depth=6)
