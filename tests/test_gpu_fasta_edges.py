"""The FASTA ingest kernels on the corpus of fasta_edge_cases.py: dgrp_fasta_encode, dgrp_fasta_encode_batch and dgrp_fasta_chunks
against `reference` and the numpy chunk table, with what the kernels look at on the edges the kernels have -- the tile whose last
bytes look ahead into the next one, the lane / wave / workgroup / tile steps of the N stripping, the 1 MiB switch of the batch entry
between its two kernel chains, the 64 MiB sweep of the chunk finder's capped grid.  Every buffer the library writes sits between
sentinels, the workspace is exactly as long as the library asks for and comes in with each of stream_harness.FILLS, the bytes behind
a body are the ones an over-read would trip on, and the input is unchanged afterwards."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_edge_cases as fc                          # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import FILLS                       # noqa: E402

GUARD = 512
SENT = 0xA5                                            # in d_idx and its guards: no class index
WGUARD = 0x5C                                          # the workspace's guards: none of FILLS
PER_CALL = 40


@pytest.fixture(scope="module")
def gpu():
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import require_gpu
    return lib(), require_gpu()


def _sp():
    from deepgrp_amd.pipeline import stream_ptr
    return stream_ptr()


def _guarded(nbytes, dev, guard=SENT, fill=None):
    buf = torch.full((nbytes + 2 * GUARD,), guard, dtype=torch.uint8, device=dev)
    if fill is not None:
        buf[GUARD:GUARD + nbytes] = fill
    return buf, buf.data_ptr() + GUARD


def _intact(buf, nbytes, guard=SENT):
    return bool((buf[:GUARD] == guard).all()) and bool((buf[GUARD + nbytes:] == guard).all())


_REF = {}


def ref_of(body: bytes):
    """`reference` of a body, computed once per process."""
    if body not in _REF:
        _REF[body] = fc.reference(body)
    return _REF[body]


def encode_one(gpu, body: bytes, shift: int = 0, fill: int = FILLS[0]):
    """dgrp_fasta_encode on `body` at d_raw + shift -> (the four info values, the capacity of d_idx as it is afterwards).  A line
    feed stands behind the body: a look-ahead that leaves it sees a blank line, or completes a CRLF."""
    L, dev = gpu
    n = len(body)
    host = np.full(shift + n + fc.VEC, 10, np.uint8)
    host[:shift] = 10
    host[shift:shift + n] = np.frombuffer(body, np.uint8)
    d_raw = torch.from_numpy(host.copy()).to(dev)
    idx, p_idx = _guarded(n, dev)
    wb = int(L.dgrp_fasta_workspace_bytes(n))
    assert wb > 0 and wb % 256 == 0
    work, p_work = _guarded(wb, dev, WGUARD, fill)
    info = (C.c_int64 * 4)(-9, -9, -9, -9)
    rc = L.dgrp_fasta_encode(d_raw.data_ptr() + shift, n, p_idx, info, p_work, wb, _sp())
    assert rc == 0, L.dgrp_last_error()
    assert _intact(work, wb, WGUARD) and _intact(idx, n)
    assert np.array_equal(d_raw.cpu().numpy(), host)
    return list(info), idx[GUARD:GUARD + n].cpu().numpy()


def hold_one(body: bytes, info, got, what):
    plain, total, startpos, kept, idx = ref_of(body)
    assert info[0] == plain, what
    if plain:
        assert info[1:] == [total, startpos, kept], what
        np.testing.assert_array_equal(got[:total], idx, str(what))
        assert (got[total:] == SENT).all(), what


_SINGLE = {}


def single_info(gpu, body: bytes):
    """The four values dgrp_fasta_encode gives for the body (one call per body and process)."""
    if body not in _SINGLE:
        _SINGLE[body] = encode_one(gpu, body)[0]
    return _SINGLE[body]


def encode_batch(gpu, text: bytes, off, ln, fill: int = FILLS[0]):
    """One dgrp_fasta_encode_batch over the records (off, ln) of `text` -> (info [nrec, 4], d_idx [len(text)] as it is afterwards)."""
    L, dev = gpu
    host = np.frombuffer(text, np.uint8)
    d_raw = torch.from_numpy(host.copy()).to(dev)
    idx, p_idx = _guarded(len(text), dev)
    wb = int(L.dgrp_fasta_batch_workspace_bytes(len(off), int(ln.sum())))
    assert wb > 0 and wb % 256 == 0
    work, p_work = _guarded(wb, dev, WGUARD, fill)
    infos = np.full((len(off), 4), -9, np.int64)
    off, ln = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(ln, np.int64)
    off0, ln0 = off.copy(), ln.copy()
    rc = L.dgrp_fasta_encode_batch(d_raw.data_ptr(), len(off), off.ctypes.data, ln.ctypes.data, p_idx, infos.ctypes.data, p_work, wb, _sp())
    assert rc == 0, L.dgrp_last_error()
    assert _intact(work, wb, WGUARD) and _intact(idx, len(text))
    assert np.array_equal(d_raw.cpu().numpy(), host) and np.array_equal(off, off0) and np.array_equal(ln, ln0)
    return infos, idx[GUARD:GUARD + len(text)].cpu().numpy()


def hold_batch(bodies, off, infos, got, what):
    """Every record's info and indices against `reference`; every byte of d_idx outside [off, off + total) of a plain record and
    outside [off, off + len) of any other (whose indices nobody reads) still the sentinel."""
    want = np.full(got.size, SENT, np.uint8)
    stated = np.ones(got.size, bool)
    for r, body in enumerate(bodies):
        plain, total, startpos, kept, idx = ref_of(body)
        o = int(off[r])
        assert infos[r, 0] == plain, (what, r)
        if plain:
            assert infos[r, 1:].tolist() == [total, startpos, kept], (what, r)
            want[o:o + total] = idx
        else:
            stated[o:o + len(body)] = False
    bad = np.flatnonzero((got != want) & stated)
    assert bad.size == 0, (what, "first wrong byte of d_idx", int(bad[0]), int(np.searchsorted(off, bad[0], "right")) - 1)


def batch_of(cases):
    """The bodies as records of one buffer: header bytes of changing length between them (odd and even offsets), a line feed right
    behind every body (what an over-read trips on)."""
    text, off = bytearray(b">first\n"), []
    for k, c in enumerate(cases):
        off.append(len(text))
        text += c.body + b"\n>h" + b"x" * (k % 5) + b"\n"
    return bytes(text), np.array(off, np.int64), np.array([len(c.body) for c in cases], np.int64)


def both_entries(gpu, cases, what):
    """The cases through dgrp_fasta_encode one by one and as records of dgrp_fasta_encode_batch calls of PER_CALL records."""
    for k, c in enumerate(cases):
        info, got = encode_one(gpu, c.body, fill=FILLS[k % 3])
        assert info[0] == c.plain, c.name
        hold_one(c.body, info, got, c.name)
        _SINGLE.setdefault(c.body, info)
    for g in range(0, len(cases), PER_CALL):
        part = cases[g:g + PER_CALL]
        text, off, ln = batch_of(part)
        infos, got = encode_batch(gpu, text, off, ln, fill=FILLS[(g // PER_CALL) % 3])
        hold_batch([c.body for c in part], off, infos, got, what)
        for r, c in enumerate(part):
            assert infos[r].tolist() == single_info(gpu, c.body), c.name


# ---------------------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("name", list(fc.FEATURES))
def test_single_entry_on_a_feature_at_every_split_of_both_tile_edges(gpu, name):
    cases = fc.edge_bodies(name)
    for k, c in enumerate(cases):
        info, got = encode_one(gpu, c.body, fill=FILLS[k % 3])
        assert info[0] == fc.FEATURES[name][1], c.name
        hold_one(c.body, info, got, c.name)
        _SINGLE.setdefault(c.body, info)
    for c in cases:
        if c.at + len(fc.FEATURES[name][0]) == fc.TILE + 1 or (len(fc.FEATURES[name][0]) == 1 and c.at == fc.TILE - 1):
            info, got = encode_one(gpu, c.body, shift=1)                     # the feature's last byte the first of tile 1; d_raw odd
            hold_one(c.body, info, got, (c.name, "shift 1"))
            assert info == single_info(gpu, c.body)
            break
    else:
        raise AssertionError("no case for the shifted call")


MATRIX = [c for name in fc.FEATURES for c in fc.edge_bodies(name)]


@pytest.mark.parametrize("g", range(0, len(MATRIX), PER_CALL))
def test_batch_entry_small_path_on_the_same_bodies(gpu, g):
    part = MATRIX[g:g + PER_CALL]
    text, off, ln = batch_of(part)
    assert {int(o) % 2 for o in off} == {0, 1}
    infos, got = encode_batch(gpu, text, off, ln, fill=FILLS[(g // PER_CALL) % 3])
    hold_batch([c.body for c in part], off, infos, got, g)
    for r, c in enumerate(part):
        assert infos[r, 0] == c.plain, c.name
        assert infos[r].tolist() == single_info(gpu, c.body), c.name        # all four, plain or not


def test_ends_of_the_body_and_lengths_about_the_tile(gpu):
    both_entries(gpu, fc.end_bodies(), "ends")


def test_n_stripping_over_lanes_waves_and_tiles(gpu):
    cases = fc.n_bodies()
    both_entries(gpu, cases, "n")
    for c in cases:
        if "_none" in c.name or c.name in ("n_single_N", "n_single_n"):
            total = ref_of(c.body)[1]
            assert single_info(gpu, c.body) == [1, total, total, -total], c.name


def test_an_empty_body_touches_nothing(gpu):
    info, got = encode_one(gpu, b"")
    assert info == [1, 0, 0, 0] and got.size == 0


# ---------------------------------------------------------------------------------------------------------------- path switch
@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
def test_mixed_batch_across_the_small_bytes_switch(gpu, fill):
    b = fc.mixed_batch()
    infos, got = encode_batch(gpu, b.text, b.off, b.len, fill=fill)
    assert infos[:, 0].tolist() == b.plain and infos[7, 0] == 0              # the space in the last tile of a large record
    hold_batch(b.bodies, b.off, infos, got, "mixed")
    for r in (0, 6, 10):
        assert b.len[r] == 0 and infos[r].tolist() == [1, 0, 0, 0]
    # the same bytes through fasta_record_kernel (SMALL - 1, SMALL) and through count / scan / scatter (SMALL + 1)
    total = int(infos[2, 1])
    assert total == ref_of(b.bodies[2])[1] and infos[3, 1] == total + 1 and infos[4, 1] == total + 2
    o2, o3, o4 = (int(b.off[r]) for r in (2, 3, 4))
    assert np.array_equal(got[o2:o2 + total], got[o3:o3 + total]) and np.array_equal(got[o2:o2 + total], got[o4:o4 + total])
    st = int(infos[2, 2])
    assert st >= 5 and infos[3, 2] == st == infos[4, 2] and infos[3, 3] == infos[4, 3] == total + 1 - st    # "NNnNn" ... "A" | "AN"


def test_an_all_empty_batch_writes_nothing(gpu):
    e = fc.empty_batch()
    infos, got = encode_batch(gpu, e.text, e.off, e.len)
    assert infos.tolist() == [[1, 0, 0, 0]] * 3 and (got == SENT).all()


# ---------------------------------------------------------------------------------------------------------------- chunk seam
def _chunks(gpu, d_raw, nbytes, cap, fill):
    L, dev = gpu
    st, lf, n = np.full(cap, -7, np.int64), np.full(cap, -7, np.int64), C.c_int64(-1)
    wb = int(L.dgrp_fasta_chunks_workspace_bytes(cap))
    work, p_work = _guarded(wb, dev, WGUARD, fill)
    rc = L.dgrp_fasta_chunks(d_raw.data_ptr(), nbytes, cap, st.ctypes.data, lf.ctypes.data, C.byref(n), p_work, wb, _sp())
    assert rc == 0, L.dgrp_last_error()
    assert _intact(work, wb, WGUARD)
    return n.value, st, lf


@pytest.mark.parametrize("shift", fc.SEAM_SHIFTS)
def test_chunk_starts_at_the_seam_of_the_grid_stride_sweeps(gpu, shift):
    dev = gpu[1]
    d = fc.seam_text(shift)
    starts, first_lf = fc.seam_answer(d)
    d_raw = torch.from_numpy(d).to(dev)
    assert d_raw.data_ptr() % fc.VEC == 0
    fill = FILLS[fc.SEAM_SHIFTS.index(shift)]
    n, st, lf = _chunks(gpu, d_raw, d.size, starts.size, fill)
    assert n == starts.size
    assert st.tolist() == starts.tolist() and lf.tolist() == first_lf.tolist()
    n2, st2, lf2 = _chunks(gpu, d_raw, d.size, starts.size - 1, fill)      # one too few: the count, and nothing else
    assert n2 == starts.size and (st2 == -7).all() and (lf2 == -7).all()
    assert bool((d_raw.cpu() == torch.from_numpy(d)).all())


# ---------------------------------------------------------------------------------------------------------------- the package
_FILE = {}


def _package_file(orc, tmp_path_factory):
    """mixed_batch's text with an odd record and a header-only record behind it, and what the reference's loop yields from it."""
    if not _FILE:
        b = fc.mixed_batch()
        path = tmp_path_factory.mktemp("fasta_edges") / "mixed.fa"
        path.write_bytes(b.text + b">odd\nAC GT\n>onlyheader\n")
        with open(path, "r") as fh:
            loop = orc.read_multi_fasta(fh)
        want = []
        for h, s in loop:
            st, n = orc.strip_n(s.encode())
            want.append((h, st, n, orc.encode_idx(s.encode()[st:st + max(n, 0)])))
        _FILE.update(path=str(path), want=want, ndev=sum(b.plain) + 1)
    return _FILE


@pytest.mark.parametrize("group_records", (4096, 3))
def test_through_read_multi_fasta_device(gpu, orc, tmp_path_factory, group_records):
    from deepgrp_amd.fasta import DeviceRecord, read_multi_fasta_device
    f = _package_file(orc, tmp_path_factory)
    got, ndev = [], 0
    for h, rec in read_multi_fasta_device(f["path"], group_records=group_records):
        if isinstance(rec, DeviceRecord):
            ndev += 1
            got.append((h, rec.startpos, rec.length, rec.d_idx.cpu().numpy()))
        else:
            st, n = orc.strip_n(rec.encode())
            got.append((h, st, n, orc.encode_idx(rec.encode()[st:st + max(n, 0)])))
    assert [g[0] for g in got] == [w[0] for w in f["want"]] and len(got) == 13
    for (h, st, n, idx), (_wh, wst, wn, widx) in zip(got, f["want"]):
        assert (st, n) == (wst, wn), h
        np.testing.assert_array_equal(idx, widx, h)
    assert ndev == f["ndev"] == 11                                            # every plain body with a header; the spoiled and the odd one not
