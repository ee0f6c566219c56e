"""dgrp_track_index_batch on the GPU: for every case the text comes from dgrp_track_text_batch and the index from the new entry for
the same arguments; the text is compressed on the host, tracks.TrackFiles (the code the command line uses) maps the text offsets to
virtual offsets and writes the files, and the `.tbi` must inflate to tabix.reference_index of the `.gz`, byte for byte.  Every call
is made twice: with chunk_cap 0 (counts only, nothing written) and with the exact capacities and guard values behind the buffers."""
import gzip

import numpy as np
import pytest

from tabix_corpus import BLOCK, noisy, parse

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C5, DIGITS, CLASSES = 5, 2, (1, 2, 3, 4)
GUARD = 0x5a


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


def _tables(n, spos, names, cls):
    nn, sp = (np.ascontiguousarray(x, np.int64) for x in (n, spos))
    noff = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(x) for x in names], out=noff[1:])
    return nn, sp, noff, b"".join(names), np.ascontiguousarray(cls, np.int32)


def _text(L, d_probs, row0, n, spos, names, cls, bin):
    """dgrp_track_text_batch -> (text as bytes, class offsets)"""
    from deepgrp_amd.pipeline import stream_ptr
    nn, sp, noff, blob, cl = _tables(n, spos, names, cls)
    r0 = np.ascontiguousarray(row0, np.int64)
    wb = L.dgrp_track_batch_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=d_probs.device)
    off = np.full(len(cl) + 1, -1, np.int64)
    text = torch.empty(1, dtype=torch.uint8, device=d_probs.device)
    for _ in range(2):
        cap = max(int(off[-1]), 0)
        text = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_probs.device)
        assert L.dgrp_track_text_batch(d_probs.data_ptr(), C5, len(nn), r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data,
                                       cl.ctypes.data, len(cl), DIGITS, bin, text.data_ptr(), cap, off.ctypes.data, work.data_ptr(), wb,
                                       stream_ptr()) == 0
    return text.cpu().numpy().tobytes()[:int(off[-1])], off


def _index(L, d_probs, row0, n, spos, names, cls, bin):
    """dgrp_track_index_batch, first with chunk_cap 0, then with exactly the room reported and guards -> (chunks, chunk offsets,
    linear [classes, windows], window prefix)"""
    from deepgrp_amd.pipeline import stream_ptr
    from deepgrp_amd.tabix import CHUNK_DTYPE
    nn, sp, noff, blob, cl = _tables(n, spos, names, cls)
    r0 = np.ascontiguousarray(row0, np.int64)
    dev = d_probs.device
    wpref = np.zeros(len(nn) + 1, np.int64)
    np.cumsum(((sp + nn - 1) >> 14) + 1, out=wpref[1:])
    nwin = int(wpref[-1]) * len(cl)
    wb = L.dgrp_track_index_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    linear = torch.full((nwin + 16,), GUARD, dtype=torch.int64, device=dev)
    off = np.full(len(cl) + 1, -1, np.int64)

    def call(chunks, cap):
        rc = L.dgrp_track_index_batch(d_probs.data_ptr(), C5, len(nn), r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data,
                                      cl.ctypes.data, len(cl), DIGITS, bin, chunks.data_ptr(), cap, off.ctypes.data, linear.data_ptr(), nwin,
                                      work.data_ptr(), wb, stream_ptr())
        assert rc == 0, L.dgrp_last_error()
    probe = torch.full((64,), GUARD, dtype=torch.uint8, device=dev)
    call(probe, 0)
    total = int(off[-1])
    assert off[0] == 0 and (np.diff(off) >= 0).all()
    if total > 0:                                                       # the counts alone: nothing was written
        assert (probe.cpu().numpy() == GUARD).all() and (linear.cpu().numpy() == GUARD).all()
    counts = off.copy()
    size = CHUNK_DTYPE.itemsize
    chunks = torch.full(((total + 4) * size,), GUARD, dtype=torch.uint8, device=dev)
    call(chunks, total)
    assert (off == counts).all()
    host, lin = chunks.cpu().numpy(), linear.cpu().numpy()
    assert (host[total * size:] == GUARD).all() and (lin[nwin:] == GUARD).all()          # nothing behind the exact capacities
    return host[:total * size].view(CHUNK_DTYPE).copy(), off, lin[:nwin].reshape(len(cl), -1).copy(), wpref


def _files(tmp_path, writes, bin):
    """The writes through tracks.TrackFiles, as the command line drives it -> [(gz bytes, tbi bytes or None)] per class"""
    from deepgrp_amd import gz, tracks
    plan = tracks.TrackPlan(str(tmp_path / "T"), CLASSES, DIGITS, bin, {"x.fa": "x.fa"}, 1, True)
    spec = tracks.TrackSpec(CLASSES, DIGITS, bin, 1, True)
    files = tracks.TrackFiles(plan, spec, "x.fa")
    for names, text, toff, chunks, coff, linear, wpref in writes:
        texts = tracks.TrackTexts(gz.bgzf_compress_host(text[toff[k]:toff[k + 1]], eof=False, level=1) for k in range(len(CLASSES)))
        texts.index = tracks.WriteIndex(list(names), None, chunks, coff, linear, wpref)
        files.write(texts)
    files.commit()
    out = []
    for c in CLASSES:
        path = tmp_path / "T" / f"x.fa.class{c}.bedGraph.gz"
        tbi = tmp_path / "T" / f"x.fa.class{c}.bedGraph.gz.tbi"
        out.append((path.read_bytes(), tbi.read_bytes() if tbi.exists() else None))
    return out


def _check(L, tmp_path, probs, row0, n, spos, names, bin, splits=None):
    """The case's records in one write (or split at `splits`): text, index, files; every .tbi is reference_index of its .gz.
    -> per class (text, payload)"""
    from deepgrp_amd import tabix
    from deepgrp_amd.tracks import reference_text
    d_probs = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).cuda()
    cuts = [0] + list(splits or []) + [len(n)]
    writes, whole = [], [b""] * len(CLASSES)
    for a, b in zip(cuts[:-1], cuts[1:]):
        args = (d_probs, row0[a:b], n[a:b], spos[a:b], names[a:b], CLASSES, bin)
        text, toff = _text(L, *args)
        chunks, coff, linear, wpref = _index(L, *args)
        assert (chunks["beg"] < chunks["end"]).all()
        for k in range(len(CLASSES)):
            sl = chunks[coff[k]:coff[k + 1]]
            assert (sl["beg"][1:] == sl["end"][:-1]).all()              # the text holds nothing but lines: chunks tile the slice
            if len(sl):
                assert sl["beg"][0] == 0 and sl["end"][-1] == toff[k + 1] - toff[k]
            whole[k] += text[toff[k]:toff[k + 1]]
        writes.append((names[a:b], text, toff, chunks, coff, linear, wpref))
    out = []
    for k, (comp, tbi) in enumerate(_files(tmp_path, writes, bin)):
        assert gzip.decompress(comp) == whole[k]
        want = b"".join(reference_text(probs[row0[r]:row0[r] + n[r], CLASSES[k]], spos[r], names[r], DIGITS, bin) for r in range(len(n)))
        assert whole[k] == want                                         # (the text is the statement's: the index is of the real thing)
        assert tbi is not None and gzip.decompress(tbi) == tabix.reference_index(comp), (k, bin)
        out.append((whole[k], gzip.decompress(tbi)))
    return out


def _noisy_probs(n, seed, step=4):
    p = np.zeros((n, C5), np.float32)
    for c in range(1, C5):
        p[:, c] = noisy(n, seed * 10 + c, step)
    return p


NAME = b"NC_000001.11"


@pytest.mark.parametrize("bin", [1, 50, 128])
def test_one_noisy_record(L, tmp_path, bin):
    """Tile edges, three windows (16 000 .. 56 000), several members at bin 1; bin 128 takes the wave bin pass."""
    from deepgrp_amd import tabix
    out = _check(L, tmp_path, _noisy_probs(40_000, 1), [0], [40_000], [16_000], [NAME], bin)
    for text, pl in out:
        ix = tabix.read_index(pl)
        assert ix["names"] == [NAME] and len(ix["linear"][0]) == 4
        if bin == 1:
            assert len(text) > 3 * BLOCK and len(ix["bins"][0]) >= 4    # leaves of three windows and a line across a window edge


def test_one_line_over_twenty_tiles_and_a_class_without_a_line(L, tmp_path):
    from deepgrp_amd import tabix
    p = _noisy_probs(40_000, 2)
    p[:, 1] = 0.37                                                      # one line, its first and last bin 20 tiles apart
    p[:, 3] = 0                                                         # an empty slice between two noisy ones
    out = _check(L, tmp_path, p, [0], [40_000], [16_000], [NAME], 1)
    assert out[0][0] == NAME + b"\t16000\t56000\t0.37\n"
    ix = tabix.read_index(out[0][1])
    assert ix["bins"][0].keys() == {585} and len(ix["linear"][0]) == 4 and len(set(ix["linear"][0].tolist())) == 1
    assert out[2][0] == b"" and tabix.read_index(out[2][1])["names"] == []
    assert len(out[1][0]) > BLOCK and len(out[3][0]) > BLOCK


def test_lines_that_meet_at_and_straddle_window_edges(L, tmp_path):
    from deepgrp_amd import tabix
    n = 140_000
    p = np.zeros((n, C5), np.float32)
    for edge in (16_384, 131_072):
        p[edge - 300:edge, 1], p[edge:edge + 200, 1] = 0.3, 0.4         # two lines that meet exactly at the edge
        p[edge - 50:edge + 70, 2] = 0.5                                 # one that straddles it
    p[:, 3] = noisy(n, 33, 5)
    p[:, 4] = noisy(n, 34, 9)
    out = _check(L, tmp_path, p, [0], [n], [0], [b"chr7"], 1)
    assert [l[2:] for l in parse(out[0][0])] == [(16_084, 16_384), (16_384, 16_584), (130_772, 131_072), (131_072, 131_272)]
    assert tabix.read_index(out[0][1])["bins"][0].keys() == {4681, 4682, 4681 + 7, 4681 + 8}
    assert tabix.read_index(out[1][1])["bins"][0].keys() == {585, 73}


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
        k += 0 if r % 5 in (1, 2) else 1                                # three records in a row share a name
        names.append(b"contig_%d" % k)
        if r != 204:                                                    # record 204 has no line in any class
            probs[row0[r]:row0[r] + n[r]] = _noisy_probs(int(n[r]), 100 + r, 3 + r % 5)
    assert names[150] == names[151] != names[149] and names[204] not in (names[203], names[205])
    return probs, row0, n, spos, names


def test_a_batch_of_300_records(L, tmp_path):
    from deepgrp_amd import tabix
    probs, row0, n, spos, names = _batch()
    one = _check(L, tmp_path / "one", probs, row0, n, spos, names, 1)
    two = _check(L, tmp_path / "two", probs, row0, n, spos, names, 1, splits=[151])     # a name goes on in the next write
    for (text, pl), (text2, pl2) in zip(one, two):
        ix = tabix.read_index(pl)
        assert text == text2 and ix["names"] == tabix.read_index(pl2)["names"]
        assert ix["names"] == list(dict.fromkeys(nm for _l, nm, _s, _e in parse(text)))                 # the names that have a line here
        assert names[204] not in ix["names"] and names[150] in ix["names"] and 150 < len(ix["names"]) < len(set(names))


def test_a_record_that_ends_exactly_at_the_limit_and_one_beyond(L, tmp_path):
    from deepgrp_amd import tabix
    from deepgrp_amd.pipeline import stream_ptr
    top, n = 1 << 29, 20_000
    p = _noisy_probs(n + 1, 7)
    p[:, 4] = 0.99                                                      # one line up to the limit
    out = _check(L, tmp_path, p[:n], [0], [n], [top - n], [b"chrT"], 1)
    ix = tabix.read_index(out[0][1])
    assert max(ix["bins"][0]) == 37_448 and len(ix["linear"][0]) == 32_768
    assert tabix.read_index(out[3][1])["bins"][0].keys() == {585 + 4095}
    assert parse(out[3][0]) == [(b"chrT\t%d\t%d\t0.99" % (top - n, top), b"chrT", top - n, top)]
    # one base longer: refused before any launch, nothing touched
    d_probs = torch.from_numpy(p).cuda()
    nn, sp, noff, blob, cl = _tables([n + 1], [top - n], [b"chrT"], CLASSES)
    r0, off = np.zeros(1, np.int64), np.full(5, -1, np.int64)
    buf = torch.full((1 << 16,), GUARD, dtype=torch.int64, device=d_probs.device)
    assert L.dgrp_track_index_workspace_bytes(1, nn.ctypes.data, sp.ctypes.data, 1, 4, 4) == 0
    rc = L.dgrp_track_index_batch(d_probs.data_ptr(), C5, 1, r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data,
                                  cl.ctypes.data, 4, DIGITS, 1, buf.data_ptr(), 16, off.ctypes.data, buf.data_ptr(), 1 << 16, buf.data_ptr(),
                                  1 << 19, stream_ptr())
    msg = L.dgrp_last_error().decode()
    assert rc == -1 and "record 0 ends at 536870913" in msg and "2^29" in msg, msg
    assert off.tolist() == [0] * 5 and (buf.cpu().numpy() == GUARD).all()


def test_pipeline_method_and_the_refusal_in_python(L):
    from deepgrp_amd import tabix
    from deepgrp_amd.pipeline import ContigPipeline
    p = _noisy_probs(5000, 9)
    d_probs = torch.from_numpy(p).cuda()
    pipe = ContigPipeline.__new__(ContigPipeline)                       # the method needs no model
    got = pipe.track_index_batch_device(d_probs, [0, 2048], [2000, 2500], [10, 30_000], [b"a", "b"], CLASSES, DIGITS, 1)
    want = _index(L, d_probs, [0, 2048], [2000, 2500], [10, 30_000], [b"a", b"b"], CLASSES, 1)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all()
    with pytest.raises(tabix.IndexRefused, match="record 1 ends at"):
        pipe.track_index_batch_device(d_probs, [0, 2048], [2000, 2500], [10, (1 << 29) - 2499], [b"a", b"b"], CLASSES, DIGITS, 1)
