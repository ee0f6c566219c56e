"""dgrp_twobit_pack_batch on the device against tests/mask_twobit_cases.py, an independent statement of the 2bit record: the blobs
byte for byte inside a buffer pre-filled with a guard byte (nothing else is written), the counts and the blob offsets exactly --
and the loop closed through the reader that already exists: the written file, parsed by open_twobit and turned into text by
dgrp_twobit_text_batch, is the normalised masked text."""
import numpy as np
import pytest

import mask_twobit_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 0xA5
CASES = mc.body_cases()


@pytest.fixture(scope="module")
def want():
    """{label: (expected blob, expected counts)} -- stated once, never written."""
    return {label: (mc.blob(mc.sequence(body)), mc.counts(mc.sequence(body))) for label, body in CASES}


def _pack(bodies, aligned, out_off=0, cap=None, room=None, more_work=0):
    """One call over `bodies` placed in one buffer -> (return code, output buffer as numpy, counts, blob offsets)."""
    import torch

    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    buf, off, ln = mc.place(bodies, aligned)
    d_raw = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    assert d_raw.data_ptr() % 16 == 0
    cap = out_off + room + 48 if cap is None else cap
    d_out = torch.full((cap,), GUARD, dtype=torch.uint8, device="cuda")
    counts, blob_off = np.full((len(bodies), 3), -1, np.int64), np.full(len(bodies) + 1, -1, np.int64)
    wb = int(L.dgrp_twobit_pack_workspace_bytes(len(bodies), int(ln.sum()))) + more_work
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    rc = L.dgrp_twobit_pack_batch(d_raw.data_ptr(), len(bodies), off.ctypes.data, ln.ctypes.data, d_out.data_ptr(), out_off, cap,
                                  counts.ctypes.data, blob_off.ctypes.data, work.data_ptr(), wb, stream_ptr())
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), counts, blob_off


def _compare(labels, blobs, cnts, rc, out, counts, blob_off, out_off):
    from deepgrp_amd._lib import lib
    assert rc == 0, lib().dgrp_last_error().decode()
    assert counts.tolist() == cnts
    ends = out_off + np.cumsum([len(b) for b in blobs])
    assert blob_off.tolist() == [out_off] + ends.tolist()
    for label, b, lo, hi in zip(labels, blobs, blob_off[:-1], blob_off[1:]):
        assert out[lo:hi].tobytes() == b, label
    assert (out[:out_off] == GUARD).all() and (out[blob_off[-1]:] == GUARD).all()
    return blob_off[:-1] + [16 + 8 * (c[1] + c[2]) for c in cnts]      # where every packedDna starts


@pytest.mark.parametrize("out_off", [0, 5])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "drifting"])
def test_every_case_byte_for_byte(want, aligned, out_off):
    """All cases in one call: bodies at multiples of 16 (the tile edge where the case puts it) or at every address mod 16."""
    labels = [label for label, _b in CASES]
    blobs, cnts = [want[k][0] for k in labels], [want[k][1] for k in labels]
    rc, out, counts, blob_off = _pack([b for _l, b in CASES], aligned, out_off, room=sum(map(len, blobs)))
    packed_at = _compare(labels, blobs, cnts, rc, out, counts, blob_off, out_off)
    # the cases mean what their names say: the maximum of mask blocks, both table kinds on tile-crossing records, every placement
    n = dict(zip(labels, cnts))
    assert n["case_alternates"] == [200, 0, 100] and n["n_alternates"] == [200, 100, 0] and n["lineends_only"] == [0, 0, 0]
    assert n["case_alternates_tiles"][2] == (n["case_alternates_tiles"][0] + 1) // 2 > mc.TILE
    assert n["crlf_straddles_the_tile_run"][2] == 1 and n["crlf_straddles_the_tile_open_run"][1:] == [1, 1]
    assert set((packed_at % 16).tolist()) == set(range(16))


@pytest.mark.parametrize("label", ["oneline8229", "case_alternates_tiles", "crlf_straddles_the_tile_run"])
def test_one_record_placed_at_every_address(want, label):
    """packedDna of a record of more than one tile at every address mod 16 (out_off moves the blob byte by byte)."""
    body = dict(CASES)[label]
    blob, cnt = want[label]
    seen = set()
    for out_off in range(16):
        rc, out, counts, blob_off = _pack([body], True, out_off, room=len(blob))
        seen |= set((_compare([label], [blob], [cnt], rc, out, counts, blob_off, out_off) % 16).tolist())
    assert seen == set(range(16))


def test_a_batch_of_3000_records_and_a_larger_workspace():
    """3 000 records of 20..400 characters in one call, records without a tile between records with tiles, the workspace larger
    than asked for."""
    bodies = mc.batch_bodies(3000)
    seqs = [mc.sequence(b) for b in bodies]
    blobs, cnts = [mc.blob(s) for s in seqs], [mc.counts(s) for s in seqs]
    assert sum(1 for b in bodies if not b) > 300 and sum(1 for b in bodies if b == b"\n") > 200
    rc, out, counts, blob_off = _pack(bodies, False, 3, room=sum(map(len, blobs)), more_work=4096 + 24)
    _compare([str(i) for i in range(len(bodies))], blobs, cnts, rc, out, counts, blob_off, 3)


def test_blobs_that_do_not_fit_are_refused_with_their_sizes(want):
    """An output one byte short of the blobs (but with room for their fixed words): DGRP_ENOMEM once the counts are known, the
    counts and offsets filled, nothing written."""
    from deepgrp_amd._lib import lib
    labels = [label for label, _b in CASES]
    need = sum(len(want[k][0]) for k in labels)
    rc, out, counts, blob_off = _pack([b for _l, b in CASES], False, 2, cap=2 + need - 1)
    assert rc == -3 and "output buffer" in lib().dgrp_last_error().decode()
    assert counts.tolist() == [want[k][1] for k in labels] and blob_off[-1] == 2 + need
    assert (out == GUARD).all()


def test_the_written_file_reads_back_as_the_normalised_masked_text(want, tmp_path):
    """Device blobs -> twobit.write_file -> open_twobit -> DeviceTwoBit.text(): the masked text with names cut to their first
    word, sequences re-wrapped at 50 bases and non-ACGT letters as N or n."""
    from deepgrp_amd import twobit
    from deepgrp_amd.fasta import _upload_file
    from deepgrp_amd.pipeline import require_gpu
    labels = [label for label, _b in CASES]
    bodies = [b for _l, b in CASES]
    rc, out, _counts, blob_off = _pack(bodies, False, 0, room=sum(len(want[k][0]) for k in labels))
    assert rc == 0
    headers = [b"rec%d %s" % (i, label.encode()) for i, label in enumerate(labels)]
    text = b"".join(b">" + h + b"\n" + body + (b"" if not body or body.endswith(b"\n") else b"\n") for h, body in zip(headers, bodies))
    path = tmp_path / "masked.2bit"
    twobit.write_file([twobit.record_name(h.decode()) for h in headers], [out[lo:hi] for lo, hi in zip(blob_off[:-1], blob_off[1:])], path)
    assert path.read_bytes() == mc.file_of(text)
    tb = twobit.open_twobit(path)
    got = twobit.DeviceTwoBit(tb, require_gpu(), _upload_file).text().cpu().numpy().tobytes()
    assert got == mc.normalised(text)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_records_of_the_host_path_are_packed_from_the_host_masked_bytes(tmp_path, mode):
    """masking.mask_fasta(twobit=True) on a file whose records take both paths -- plain ones, a chunk of two records with lone-CR
    line ends, text before the first header, an empty header: the file of the plain masked copy, byte for byte; sequence lines
    that are not ASCII are refused."""
    from deepgrp_amd import masking, twobit
    from deepgrp_amd.pipeline import SEGMENT_DTYPE
    text = (b"ACGT\n>a first\nACGTacgtNNACGTACGTAC\nGTnnACGT\n>b lone\rACGTNNacgtAC\rACGRYacg\r>c in the same chunk\rNNNNACGTAC\n"
            b">\nGGGG\n>d crlf\r\nACGTACGTAC\r\nnnACGTAC\r\n>e\nAC")
    src = tmp_path / "mixed.fa"
    src.write_bytes(text)
    assert [n for n, _s in mc.records(text)] == [b"a", b"b", b"c", b"d", b"e"]
    rows = np.array([(2, 9, 1, 0), (12, 20, 2, 0), (3, 15, 1, 1), (0, 6, 3, 2), (5, 12, 1, 3), (1, 2, 1, 4)], SEGMENT_DTYPE)
    plain, packed = tmp_path / "plain.fa", tmp_path / "packed.2bit"
    assert masking.mask_fasta(src, plain, rows, mode=mode) == 5
    assert masking.mask_fasta(src, packed, rows, mode=mode, twobit=True) == 5
    masked = plain.read_bytes()
    assert masked != text and len(masked) == len(text)
    assert packed.read_bytes() == mc.file_of(masked)
    assert [f for f in sorted(p.name for p in tmp_path.iterdir())] == ["mixed.fa", "packed.2bit", "plain.fa"]      # no spool left
    bad = tmp_path / "latin1.fa"
    bad.write_bytes(b">ok\nACGT\n>caf\xe9\rAC\xe9GT\rAC\n")
    with pytest.raises(twobit.Refused, match="latin1.fa: record .* not ASCII"):
        masking.mask_fasta(bad, tmp_path / "bad.2bit", np.zeros(0, SEGMENT_DTYPE), twobit=True)
