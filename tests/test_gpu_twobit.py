"""The 2bit kernels and the 2bit ingest on the device, against the corpus's own statement of the format (tests/twobit_corpus.py):
dgrp_twobit_encode_batch gives the class indices and writes nothing else, dgrp_twobit_text_batch gives the text of the file byte for
byte, dgrp_fasta_encode_batch on that text agrees with the 2bit path, and read_multi_fasta_device yields for x.2bit what it yields for
the text of x.2bit.  Every comparison is exact."""
import numpy as np
import pytest

import twobit_corpus as tc

pytestmark = pytest.mark.gpu

GUARD = 0xEE
FILES = {"sizes": tc.sizes_file, "blocks": tc.blocks_file, "odd": tc.odd_file, "batch": lambda: tc.batch_file(3000)}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """{name: (records, parsed file, file bytes on the device)} -- parsed and uploaded once, never written."""
    import torch

    from deepgrp_amd import twobit
    d = tmp_path_factory.mktemp("twobit")
    out = {}
    for name, make in FILES.items():
        recs = make()
        for order in ("<", ">") if name in ("sizes", "blocks") else ("<",):
            path = d / f"{name}{'_be' if order == '>' else ''}.2bit"
            path.write_bytes(tc.write(recs, order))
            tb = twobit.open_twobit(path)
            out[path.stem] = (recs, tb, torch.from_numpy(np.fromfile(path, np.uint8)).cuda())
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if len(a) else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _encode(tb, d_file, out_off, d_idx):
    import torch

    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    d_iv = _dev(tb.n_iv)
    wb = int(L.dgrp_twobit_workspace_bytes(tb.nrec))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    check(L.dgrp_twobit_encode_batch(d_file.data_ptr(), tb.size, tb.nrec, tb.packed_off.ctypes.data, tb.dna_size.ctypes.data, _ptr(d_iv),
                                     tb.n_off.ctypes.data, len(tb.n_iv), out_off.ctypes.data, d_idx.data_ptr(), int(d_idx.numel()),
                                     work.data_ptr(), wb, stream_ptr()), "dgrp_twobit_encode_batch")
    return d_iv, work                                                  # alive until the caller has synchronised


def _text(tb, d_file, text_off, d_text):
    import torch

    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    d_n, d_m = _dev(tb.n_iv), _dev(tb.m_iv)
    wb = int(L.dgrp_twobit_workspace_bytes(tb.nrec))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    check(L.dgrp_twobit_text_batch(d_file.data_ptr(), tb.size, tb.nrec, tb.name_off.ctypes.data, tb.name_len.ctypes.data,
                                   tb.packed_off.ctypes.data, tb.dna_size.ctypes.data, _ptr(d_n), tb.n_off.ctypes.data, len(tb.n_iv),
                                   _ptr(d_m), tb.m_off.ctypes.data, len(tb.m_iv), text_off.ctypes.data, d_text.data_ptr(),
                                   int(d_text.numel()), work.data_ptr(), wb, stream_ptr()), "dgrp_twobit_text_batch")
    return d_n, d_m, work


def _aligned_phase(packed_addr: int) -> int:
    """Where in a 16-byte word of the index buffer a record has to start for the kernel's 4-byte packed loads to be aligned, found by
    trying: the second word of a record that starts `o` bytes into its first word begins with base 16 - o, which has to be the first
    base of a packed byte whose address is a multiple of 4."""
    ok = [o for o in range(16) if (16 - o) % 4 == 0 and (packed_addr + (16 - o) // 4) % 4 == 0]
    assert len(ok) == 1, (packed_addr, ok)
    return ok[0]


def _layouts(tb, d_file):
    """Index offsets per record (the buffer itself is 16-byte aligned): placed so that packed loads and index stores are both
    aligned, as the ingest places them, and with gaps of 0..19 bytes (every alignment of the output against the packed bytes)."""
    dna = tb.dna_size
    phase = np.array([_aligned_phase(d_file.data_ptr() + int(p)) for p in tb.packed_off], np.int64)
    slot = (dna + 31) & ~np.int64(15)
    yield "placed", np.ascontiguousarray(np.cumsum(slot) - slot + phase, np.int64), int(slot.sum()) + 32
    gaps = np.random.default_rng(tc.SEED + 9).integers(0, 20, tb.nrec)
    off = np.cumsum(dna + gaps) - dna
    yield "gaps", np.ascontiguousarray(off, np.int64), int(off[-1] + dna[-1]) + 11


@pytest.mark.parametrize("which", ["sizes", "sizes_be", "blocks", "blocks_be", "odd", "batch"])
def test_encode_gives_the_indices_and_writes_nothing_else(corpus, which):
    import torch
    recs, tb, d_file = corpus[which]
    for tag, out_off, cap in _layouts(tb, d_file):
        d_idx = torch.full((cap,), GUARD, dtype=torch.uint8, device="cuda")
        assert d_idx.data_ptr() % 16 == 0
        want = np.full(cap, GUARD, np.uint8)
        for r, rec in enumerate(recs):
            want[out_off[r]:out_off[r] + len(rec.codes)] = tc.indices(rec)
        keep = _encode(tb, d_file, out_off, d_idx)
        got = d_idx.cpu().numpy()
        del keep
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (which, tag, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("which", ["sizes", "sizes_be", "blocks", "odd", "batch"])
def test_text_is_the_text_of_the_file(corpus, which):
    import torch
    recs, tb, d_file = corpus[which]
    want = np.frombuffer(tc.text(recs), np.uint8)
    assert tb.text_size == want.size
    for shift in (0, 5):                                               # records in a row, the first at an aligned or an odd address
        d_text = torch.full((want.size + shift + 9,), GUARD, dtype=torch.uint8, device="cuda")
        keep = _text(tb, d_file, np.ascontiguousarray(tb.text_off[:-1] + shift), d_text)
        got = d_text.cpu().numpy()
        del keep
        assert (got[:shift] == GUARD).all() and (got[shift + want.size:] == GUARD).all(), (which, shift)
        bad = np.flatnonzero(got[shift:shift + want.size] != want)
        assert bad.size == 0, (which, shift, bad[:8].tolist(), bytes(got[shift:][bad[:8]]), bytes(want[bad[:8]]))


@pytest.mark.parametrize("which", ["sizes", "blocks", "odd", "batch"])
def test_the_fasta_encoder_on_the_text_agrees_with_the_2bit_path(corpus, which):
    """dgrp_fasta_encode_batch on the bodies of the device-built text: plain, and the indices, startpos and kept length of the 2bit
    path (the encode kernel and the parser's N intervals)."""
    import torch

    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    recs, tb, d_file = corpus[which]
    d_text = torch.empty(tb.text_size, dtype=torch.uint8, device="cuda")
    keep = _text(tb, d_file, np.ascontiguousarray(tb.text_off[:-1]), d_text)
    body = np.ascontiguousarray(tb.text_off[:-1] + 2 + tb.name_len)
    blen = np.ascontiguousarray(tb.text_off[1:] - body)
    d_fa = torch.full((tb.text_size,), GUARD, dtype=torch.uint8, device="cuda")
    info = np.zeros((tb.nrec, 4), np.int64)
    wb = int(L.dgrp_fasta_batch_workspace_bytes(tb.nrec, int(blen.sum())))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    check(L.dgrp_fasta_encode_batch(d_text.data_ptr(), tb.nrec, body.ctypes.data, blen.ctypes.data, d_fa.data_ptr(), info.ctypes.data,
                                    work.data_ptr(), wb, stream_ptr()), "dgrp_fasta_encode_batch")
    del keep
    assert (info[:, 0] == 1).all()
    assert np.array_equal(info[:, 1], tb.dna_size)
    assert np.array_equal(info[:, 2], tb.startpos) and np.array_equal(info[:, 3], tb.kept)
    _tag, out_off, cap = next(_layouts(tb, d_file))
    d_idx = torch.empty(cap, dtype=torch.uint8, device="cuda")
    keep = _encode(tb, d_file, out_off, d_idx)
    fa, tw = d_fa.cpu().numpy(), d_idx.cpu().numpy()
    del keep
    for r in range(tb.nrec):
        n = int(tb.dna_size[r])
        assert np.array_equal(fa[body[r]:body[r] + n], tw[out_off[r]:out_off[r] + n]), recs[r].name


def test_both_entries_on_a_side_stream_and_without_records(corpus):
    import torch

    from deepgrp_amd._lib import lib
    L = lib()
    recs, tb, d_file = corpus["blocks"]
    _tag, out_off, cap = next(_layouts(tb, d_file))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_idx = torch.full((cap,), GUARD, dtype=torch.uint8, device="cuda")
        d_text = torch.full((tb.text_size,), GUARD, dtype=torch.uint8, device="cuda")
        keep = _encode(tb, d_file, out_off, d_idx), _text(tb, d_file, np.ascontiguousarray(tb.text_off[:-1]), d_text)
        # nrec == 0: nothing to do, no pointer needed
        assert L.dgrp_twobit_encode_batch(None, 0, 0, None, None, None, None, 0, None, None, 0, None, 0, side.cuda_stream) == 0
        assert L.dgrp_twobit_text_batch(None, 0, 0, None, None, None, None, None, None, 0, None, None, 0, None, None, 0, None, 0,
                                        side.cuda_stream) == 0
        side.synchronize()
        idx, text = d_idx.cpu().numpy(), d_text.cpu().numpy()
    del keep
    assert bytes(text) == tc.text(recs)
    for r, rec in enumerate(recs):
        assert np.array_equal(idx[out_off[r]:out_off[r] + len(rec.codes)], tc.indices(rec)), rec.name
    assert (idx[:out_off[0]] == GUARD).all() and (idx[out_off[-1] + len(recs[-1].codes):] == GUARD).all()


def _same(a, b):
    """The yields of two ingests: same names in the same order, same kind of record, same startpos, length and indices."""
    from deepgrp_amd.fasta import DeviceRecord
    assert [h for h, _r in a] == [h for h, _r in b]
    for (h, x), (_h, y) in zip(a, b):
        assert type(x) is type(y), h
        if isinstance(x, DeviceRecord):
            assert (x.startpos, x.length) == (y.startpos, y.length), h
            assert np.array_equal(x.d_idx.cpu().numpy(), y.d_idx.cpu().numpy()), h
        else:
            assert x == y, h


@pytest.mark.parametrize("which", ["sizes", "blocks", "odd"])
@pytest.mark.parametrize("order", ["<", ">"])
def test_ingest_of_a_2bit_file_is_the_ingest_of_its_text(tmp_path, which, order):
    from deepgrp_amd.fasta import DeviceRecord, read_multi_fasta_device
    from deepgrp_amd.pipeline import record_indices
    recs = FILES[which]()
    (tmp_path / "x.2bit").write_bytes(tc.write(recs, order))
    (tmp_path / "x.fa").write_bytes(tc.text(recs))
    got, want = list(read_multi_fasta_device(tmp_path / "x.2bit")), list(read_multi_fasta_device(tmp_path / "x.fa"))
    _same(got, want)
    named = [r for r in recs if (b">" + r.name).strip()[1:]]
    assert [h for h, _r in got] == [(b">" + r.name).decode().strip()[1:] for r in named]     # a record without a name is dropped
    assert all(isinstance(r, DeviceRecord) for _h, r in got)
    for (h, rec), r in zip(got, named):
        idx = tc.indices(r)
        st, kept = tc.strip_n(idx)
        assert (rec.startpos, rec.length) == (st, kept), h
        if kept < 0:
            with pytest.raises(ValueError):                            # a record of N only: the reference's ValueError, from both
                record_indices(rec)
            with pytest.raises(ValueError):
                record_indices(dict(want)[h])
        else:
            assert np.array_equal(rec.d_idx.cpu().numpy(), idx[st:st + kept]), h
    # small groups: the same records whatever the grouping
    _same(list(read_multi_fasta_device(tmp_path / "x.2bit", group_bytes=100, group_records=3)), want)


def test_ingest_of_names_that_are_not_ascii(tmp_path, monkeypatch):
    """A name that is not ASCII takes the reference loop in the FASTA ingest; the 2bit ingest hands the device-built text to that
    same ingest, so both yield the same.  The reference loop reads text in the locale's encoding: UTF-8 here, whatever the locale."""
    import io

    from deepgrp_amd import fasta
    monkeypatch.setattr(fasta, "_text_lines", lambda raw: io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", newline=None))
    rng = np.random.default_rng(tc.SEED + 4)
    recs = [tc._rec(rng, b"plain", 70, [(0, 3)], [(10, 9)]), tc._rec(rng, "créole".encode("utf-8"), 130, [(100, 30)], [(0, 60)]),
            tc._rec(rng, b"", 20), tc._rec(rng, b"tail", 51)]
    (tmp_path / "x.2bit").write_bytes(tc.write(recs))
    (tmp_path / "x.fa").write_bytes(tc.text(recs))
    want = list(fasta.read_multi_fasta_device(tmp_path / "x.fa"))
    got = list(fasta.read_multi_fasta_device(tmp_path / "x.2bit"))
    _same(got, want)
    assert [h for h, _r in got] == ["plain", "créole", "tail"]


def test_the_ingest_places_every_record_on_the_aligned_path(corpus):
    """DeviceTwoBit.encode chooses the index offsets at which the kernel's packed loads are aligned, for packed bytes at every
    address mod 4 (names of 0..17 bytes), and its indices are the corpus's."""
    from deepgrp_amd import fasta, twobit
    recs, tb, _d_file = corpus["sizes"]
    dtb = twobit.DeviceTwoBit(tb, _d_file.device, fasta._upload_file)
    d_idx, out_off = dtb.encode(0, tb.nrec)
    got = d_idx.cpu().numpy()
    seen = set()
    for r, rec in enumerate(recs):
        addr = dtb.d_file.data_ptr() + int(tb.packed_off[r])
        assert (d_idx.data_ptr() + int(out_off[r])) % 16 == _aligned_phase(addr), rec.name
        assert np.array_equal(got[out_off[r]:out_off[r] + len(rec.codes)], tc.indices(rec)), rec.name
        seen.add(addr % 4)
    assert seen == {0, 1, 2, 3}
