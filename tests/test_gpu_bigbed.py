"""The two device entries of --bed_bigbed, byte for byte: dgrp_bed_blocks_batch against bigbed.reference_blocks, dgrp_bed_zoom_batch
against bigbed.reference_zoom and reference_totals, on synthetic rows and scores at the smallest shapes where they can go wrong;
the device refusals and the capacity protocol with guards behind the buffers; the stream contract (stream_harness.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bigbed_cases import HIGH, ladder, rows_scores      # noqa: E402
from stream_harness import FILLS, Harness, i64ptr       # noqa: E402

TOP = (1 << 32) - 1
LEVELS = 10
GUARD = 4096
ROW = {"blocks": 32, "zoom": 40}                        # bytes of a table row: dgrp_bed_block, dgrp_track_zoom_block


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def pipe_dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _batch(counts):
    spans, contigs = [], []
    for r, n in enumerate(counts):
        spans += ladder(n)
        contigs += [r] * n
    return spans, contigs


def _cases():
    """name -> (by_contig, rows, scores, min_score, rec_end, chrom0)"""
    out = {}
    for n in (1, 511, 512, 513, 1025):                                  # one record around the block size; every label and score form
        out[f"one{n}"] = (False,) + rows_scores(ladder(n)) + (0, [50_000], 0)
    out["all_filtered"] = (False,) + rows_scores(ladder(3), low=(0, 1, 2)) + (300, [50_000], 3)
    out["drop_0_511_512_last"] = (False,) + rows_scores(ladder(1025), low=(0, 511, 512, 1024), means=HIGH) + (300, [50_000], 0)
    spans, contigs = _batch([0, 3, 512, 0, 700])
    out["batch"] = (True,) + rows_scores(spans, contigs) + (0, [77, 50_000, 50_000, 1, 50_000], 7)
    # a row [0, 1), rows that touch, a row exactly on a window, a row that ends at 2^32 - 1
    spans = [(0, 1), (1, 2), (2, 1024), (1024, 2048), (5 * 1024, 6 * 1024), (0, 1), (TOP - 5, TOP)]
    out["edges"] = (True,) + rows_scores(spans, [0, 0, 0, 0, 0, 1, 1], means=HIGH) + (0, [6 * 1024, TOP], 0)
    # zoom: a record shorter than 1024, rows inside one window, a row on a window, a row over 2930 level-0 windows, a record
    # without a row and one whose rows are all filtered
    spans = [(10, 20), (30, 40), (1024, 2048), (3000, 3010), (3010, 3050), (7, 19), (1024, 1024 + 3_000_000), (3_100_000, 3_100_001),
             (100, 200), (300, 5000)]
    contigs = [0, 0, 1, 1, 1, 2, 2, 2, 4, 4]
    out["zoom"] = (True,) + rows_scores(spans, contigs, low=(8, 9), means=HIGH) + (300, [900, 5000, 3_200_000, 2000, 6000], 2)
    return out


CASES = _cases()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


@pytest.fixture(scope="module")
def reference():
    """Computed once per case, shared and left unchanged: (blocks, block table, zoom records, record offsets, zoom table, block
    offsets, totals)."""
    from deepgrp_amd import bigbed as bb
    out = {}
    for name, (by_contig, rows, scores, low, _ends, chrom0) in CASES.items():
        out[name] = (bb.reference_blocks(by_contig, rows, scores, low, chrom0) + bb.reference_zoom(by_contig, rows, scores, low, chrom0)
                     + (bb.reference_totals(by_contig, rows, scores, low),))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_blocks_are_the_reference_bytes(pipe_dev, reference, name):
    from deepgrp_amd import bigbed as bb
    from deepgrp_amd.pipeline import ContigPipeline
    by_contig, rows, scores, low, ends, chrom0 = CASES[name]
    data, table = reference[name][:2]
    d_out, d_tab, items = ContigPipeline.bed_blocks_batch(by_contig, _dev(rows, pipe_dev), _dev(scores, pipe_dev), low, ends, chrom0)
    got_tab = d_tab.cpu().numpy().view(bb.BLOCK_DTYPE)
    assert items == int(table["items"].sum()) and got_tab.tolist() == table.tolist()
    assert d_out.cpu().numpy().tobytes() == data
    if name == "batch":
        assert table["rec"].tolist() == [1, 2, 4, 4] and table["items"].tolist() == [3, 512, 512, 188]      # blocks never span records
    if name == "all_filtered":
        assert items == 0 and len(table) == 0 and data == b""
    if name == "edges":
        assert data.endswith(b"\0") and TOP.to_bytes(4, "little") in data[-60:]


@pytest.mark.parametrize("name", list(CASES))
def test_zoom_records_are_the_reference_bytes(pipe_dev, reference, name):
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd.pipeline import ContigPipeline
    by_contig, rows, scores, low, ends, chrom0 = CASES[name]
    zdata, roff, ztable, boff, totals = reference[name][2:]
    d_out, got_roff, d_tab, got_boff, got_tot = ContigPipeline.bed_zoom_batch(by_contig, _dev(rows, pipe_dev), _dev(scores, pipe_dev), low, ends, chrom0)
    assert got_roff.tolist() == roff.tolist() and got_boff.tolist() == boff.tolist()
    assert tuple(int(x) for x in got_tot[0]) == totals
    assert d_tab.cpu().numpy().view(bw.ZOOM_BLOCK_DTYPE).tolist() == ztable.tolist()
    assert d_out.cpu().numpy().tobytes() == zdata
    if name == "zoom":
        assert roff[1] > 2930 and boff[1] == 3 and roff[6] - roff[5] == 5 and totals[0] == 3_001_107
    if name == "all_filtered":
        assert totals == (0, 0, 0, 0, 0) and zdata == b""


def test_bigbed_and_bigwig_zoom_are_one_ladder(pipe_dev):
    """csrc/bbi_zoom.h is instantiated for both formats.  Coverage rows on 64-base boundaries and the one-class indicator track of
    the same rows (probability 1.0 on the rows' bases, bins of 64, so windows of 1024 bases in both) give the same records, offsets
    and block tables; only the totals are in other units (q = 100 a base against 1)."""
    from deepgrp_amd.pipeline import ContigPipeline
    ends = np.array([900, 70_016, 5_000, 64], np.int64)
    spans = [(0, 64), (128, 896), (0, 1024), (1024, 1088), (4096, 66_560), (69_952, 70_016), (0, 64)]
    contigs = [0, 0, 1, 1, 1, 1, 3]                                        # (record 2 has no row)
    rows, scores = rows_scores(spans, contigs, means=HIGH)
    bed = ContigPipeline.bed_zoom_batch(True, _dev(rows, pipe_dev), _dev(scores, pipe_dev), 0, ends, 7)
    row0 = np.r_[0, np.cumsum((ends[:-1] + 63) // 64 * 64)].astype(np.int64)
    p = np.zeros((int(row0[-1] + ends[-1]), 1), np.float32)
    for (a, b), r in zip(spans, contigs):
        p[row0[r] + a:row0[r] + b, 0] = 1.0
    track = ContigPipeline.track_zoom_batch_device(None, torch.from_numpy(p).to(pipe_dev), row0, ends, np.zeros(4, np.int64), (0,), 2, 64, 7)
    raw = lambda t: t.cpu().numpy().tobytes()
    assert bed[1].tolist() == track[1].tolist() == [0, 66, 86, 93, 97, 100, 103, 106, 109, 112, 115]
    assert raw(bed[0]) == raw(track[0]) and len(raw(bed[0])) == 3680
    assert bed[3].tolist() == track[3].tolist() and raw(bed[2]) == raw(track[2]) and len(raw(bed[2])) == 40 * int(bed[3][-1]) > 0
    c = sum(b - a for a, b in spans)
    assert tuple(int(x) for x in bed[4][0]) == (c, 1, 1, c, c)
    assert tuple(int(x) for x in track[4][0]) == (c, 100, 100, 100 * c, 10_000 * c)


# ---------------------------------------------------------------------------------------------------- refusals and capacities
def _raw(L, entry, by_contig, d_rows, d_scores, nrows, low, ends, chrom0, out, cap, table, tcap, work, wb, stream=None):
    """-> (rc, the host counts: blocks (bytes, blocks, items); zoom (record offsets, block offsets, totals))"""
    ends = np.ascontiguousarray(ends, np.int64)
    if entry == "blocks":
        a, b, c = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
        rc = L.dgrp_bed_blocks_batch(int(by_contig), d_rows.data_ptr(), d_scores.data_ptr(), nrows, low, len(ends), i64ptr(ends), chrom0,
                                     out.data_ptr(), cap, C.byref(a), table.data_ptr(), tcap, C.byref(b), C.byref(c), work.data_ptr(), wb, stream)
        return rc, (a.value, b.value, c.value)
    roff, boff, tot = np.full(LEVELS + 1, -7, np.int64), np.full(LEVELS + 1, -7, np.int64), np.full(5, 99, np.uint64)
    rc = L.dgrp_bed_zoom_batch(int(by_contig), d_rows.data_ptr(), d_scores.data_ptr(), nrows, low, len(ends), i64ptr(ends), chrom0, out.data_ptr(),
                               cap, roff.ctypes.data, table.data_ptr(), tcap, boff.ctypes.data, tot.ctypes.data, work.data_ptr(), wb, stream)
    return rc, (roff.tolist(), boff.tolist(), tot.tolist())


def _query(L, entry, nrows, ends):
    ends = np.ascontiguousarray(ends, np.int64)
    q = L.dgrp_bed_blocks_workspace_bytes if entry == "blocks" else L.dgrp_bed_zoom_workspace_bytes
    return q(nrows, len(ends), i64ptr(ends))


def _change(rows, scores, what):
    rows, scores = rows.copy(), scores.copy()
    if what == "overlap":
        rows["start"][700] = rows["end"][699] - 1
    elif what == "descending":
        rows["start"][700], rows["end"][700] = rows["start"][698], rows["start"][698] + 3
    elif what == "overlap_of_a_filtered_row":
        rows["end"][0] = rows["start"][1] + 1                           # (row 0 is filtered: it counts all the same)
    elif what == "end_above_the_record":
        rows["end"][-1] = 50_001
    elif what == "records_descend":
        rows["contig"][5] = -1
    elif what == "no_base":
        scores["bases"][3] = 0
    elif what == "sum_too_large":
        scores["sum"][3] = (int(scores["bases"][3]) << 24) + 1
    return rows, scores


@pytest.mark.parametrize("entry", ["blocks", "zoom"])
@pytest.mark.parametrize("what,word", [("overlap", "starts below the end of a row in front of it"), ("descending", "starts below the end of a row in front"),
                                       ("overlap_of_a_filtered_row", "starts below the end"), ("end_above_the_record", "ends behind its record's end"),
                                       ("records_descend", "outside the records"), ("no_base", "no scored base"),
                                       ("sum_too_large", "outside the envelope"), ("rec_end_above", "4294967296")])
def test_refusals_leave_guarded_buffers_untouched(L, pipe_dev, entry, what, word):
    rows, scores = rows_scores(ladder(1025), [0] * 1025, low=(0,), means=HIGH)
    rows, scores = _change(rows, scores, what)
    ends = [TOP + 1] if what == "rec_end_above" else [50_000]
    wb = _query(L, entry, len(rows), [50_000])
    assert wb > 0 and (_query(L, entry, len(rows), ends) == 0) == (what == "rec_end_above")
    work = torch.empty(wb, dtype=torch.uint8, device=pipe_dev)
    out = torch.full((1 << 17,), 0x5A, dtype=torch.uint8, device=pipe_dev)
    table = torch.full((64 * ROW[entry],), 0x5A, dtype=torch.uint8, device=pipe_dev)
    rc, host = _raw(L, entry, True, _dev(rows, pipe_dev), _dev(scores, pipe_dev), len(rows), 300, ends, 0, out, 1 << 17, table, 64, work, wb)
    msg = L.dgrp_last_error().decode()
    assert rc == -1 and msg.startswith(f"dgrp_bed_{entry}_batch: ") and word in msg, msg
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all() and (table.cpu().numpy() == 0x5A).all()
    assert host == ((0, 0, 0) if entry == "blocks" else ([0] * 11, [0] * 11, [0] * 5))


@pytest.mark.parametrize("entry", ["blocks", "zoom"])
def test_capacity_protocol_with_guards(L, pipe_dev, reference, entry):
    """Too little room for the bytes, or for the table: the counts are filled in full and nothing is written; exactly enough: the
    bytes behind both buffers stay as they were."""
    by_contig, rows, scores, low, ends, chrom0 = CASES["batch"]
    data, table = reference["batch"][:2] if entry == "blocks" else (reference["batch"][2], reference["batch"][4])
    need, nrows, row = len(data), len(table), ROW[entry]
    counts = (need, nrows, 1215) if entry == "blocks" else (reference["batch"][3].tolist(), reference["batch"][5].tolist(), list(reference["batch"][6]))
    wb = _query(L, entry, len(rows), ends)
    work = torch.empty(wb, dtype=torch.uint8, device=pipe_dev)
    d_rows, d_scores = _dev(rows, pipe_dev), _dev(scores, pipe_dev)
    for cap, tcap, written in ((need - 1, nrows, False), (need, nrows - 1, False), (0, 0, False), (need, nrows, True)):
        out = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=pipe_dev)
        tab = torch.full((nrows * row + GUARD,), 0x5A, dtype=torch.uint8, device=pipe_dev)
        rc, host = _raw(L, entry, by_contig, d_rows, d_scores, len(rows), low, ends, chrom0, out, cap, tab, tcap, work, wb)
        torch.cuda.synchronize()
        assert rc == 0 and host == counts, L.dgrp_last_error()
        got, gtab = out.cpu().numpy(), tab.cpu().numpy()
        if written:
            assert got[:need].tobytes() == data and gtab[:nrows * row].tobytes() == table.tobytes()
            assert (got[need:] == 0x5A).all() and (gtab[nrows * row:] == 0x5A).all()
        else:
            assert (got == 0x5A).all() and (gtab == 0x5A).all()
    small = torch.empty(wb - 1, dtype=torch.uint8, device=pipe_dev)
    rc, _host = _raw(L, entry, by_contig, d_rows, d_scores, len(rows), low, ends, chrom0, out, need, tab, nrows, small, wb - 1)
    assert rc == -3


@pytest.mark.parametrize("entry", ["blocks", "zoom"])
def test_two_calls_give_the_same_bytes_whatever_the_workspace_held(L, pipe_dev, reference, entry):
    by_contig, rows, scores, low, ends, chrom0 = CASES["zoom"]
    data = reference["zoom"][0] if entry == "blocks" else reference["zoom"][2]
    wb = _query(L, entry, len(rows), ends)
    d_rows, d_scores = _dev(rows, pipe_dev), _dev(scores, pipe_dev)
    seen = []
    for fill in FILLS:
        work = torch.full((wb,), fill, dtype=torch.uint8, device=pipe_dev)
        out = torch.full((len(data) + GUARD,), 0x5A, dtype=torch.uint8, device=pipe_dev)
        tab = torch.full((64 * ROW[entry],), 0x5A, dtype=torch.uint8, device=pipe_dev)
        rc, host = _raw(L, entry, by_contig, d_rows, d_scores, len(rows), low, ends, chrom0, out, len(data) + GUARD, tab, 64, work, wb)
        torch.cuda.synchronize()
        assert rc == 0
        seen.append((host, out.cpu().numpy().tobytes(), tab.cpu().numpy().tobytes()))
    assert seen[0] == seen[1] == seen[2] and seen[0][1][:len(data)] == data


# ---------------------------------------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def H(L, pipe_dev):
    h = Harness(pipe_dev)
    h.choose_side(L)
    return h


@pytest.mark.parametrize("entry", ["blocks", "zoom"])
def test_sync_bigbed_entries_honour_the_stream(H, L, reference, entry):
    """One synchronisation (the read-back of counts and flags), the write kernel behind it: the stream is not drained on return,
    the inputs are read behind the stream's earlier work, and the host table may be dropped on return."""
    by_contig, rows, scores, low, ends, chrom0 = CASES["batch"]
    poison_rows, poison_scores = rows.copy(), scores.copy()
    poison_rows["start"] += 3
    poison_rows["end"] += 3
    poison_scores["sum"] //= 2
    poison_scores["qmin"] //= 2
    data = reference["batch"][0] if entry == "blocks" else reference["batch"][2]
    cap, tcap = len(data) + GUARD, 64
    wb = _query(L, entry, len(rows), ends)

    def call(b, wk, st, t):
        return _raw(L, entry, by_contig, b["rows"], b["scores"], len(rows), low, t["ends"], chrom0, b["out"], cap, b["table"], tcap, wk, wb, st)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    late, host, _idle, host_idle = H.run(call, {"rows": (raw(rows), raw(poison_rows)), "scores": (raw(scores), raw(poison_scores))},
                                         {"out": np.full(cap, 0x5A, np.uint8), "table": np.full(tcap * ROW[entry], 0x5A, np.uint8)},
                                         work_bytes=wb, fill=FILLS[0], sync=True, tables={"ends": np.array(ends, np.int64)}, drained=False)
    assert host == host_idle
    assert late["out"][:len(data)].tobytes() == data and (late["out"][len(data):] == 0x5A).all()
