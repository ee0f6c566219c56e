"""dgrp_repeat_summary_batch (predict --summary_dir) on the GPU against summary.count_host / summary.bins_host over the corpus of
tests/summary_cases.py: every count is an integer, so every comparison is exact."""
import functools

import numpy as np
import pytest

import summary_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import Harness, last_error      # noqa: E402

CLASSES = (2, 5, 16)
LONGER = 1 << 20                                     # a bin longer than every record
BINS = (0, 1, 7, 4096, LONGER)
ENOMEM = -3


@functools.lru_cache(maxsize=None)
def _case(C, build="corpus"):
    """The corpus (or sc.many_tiles) for C classes with the reference counts of every record (made once, never changed)."""
    from deepgrp_amd import summary
    buf, offs, lens, rowsets = getattr(sc, build)(C)
    assert len(buf) < 400_000
    rows, row_off = sc.seg_array(rowsets)
    pos = [sc.positions(buf, int(o), int(n)) for o, n in zip(offs, lens)]
    counts = np.stack([summary.count_host(buf, p, rows[row_off[k]:row_off[k + 1]], C) for k, p in enumerate(pos)])
    assert counts.sum() == sum(p.size for p in pos) and (counts[:, 1:].sum(axis=(1, 2, 3)) > 0).sum() > 20
    return dict(C=C, buf=buf, h_off=offs, h_len=lens, rows=rows, row_off=row_off, pos=pos, counts=counts)


@functools.lru_cache(maxsize=None)
def _want_bins(C, bin, build="corpus"):
    """The density table as the entry lays it out: ceil(body bytes / bin) bins per record, those behind the sequence zero."""
    from deepgrp_amd import summary
    c = _case(C, build)
    off = sc.reserved_bins(c["h_len"], bin)
    out = np.zeros((int(off[-1]), C), np.int64)
    for k, p in enumerate(c["pos"]):
        got = summary.bins_host(c["buf"], p, c["rows"][c["row_off"][k]:c["row_off"][k + 1]], C, bin)
        assert len(got) <= off[k + 1] - off[k]
        out[off[k]:off[k] + len(got)] = got
    return out


def _counts_for(c, rows, row_off):
    from deepgrp_amd import summary
    return np.stack([summary.count_host(c["buf"], p, rows[row_off[k]:row_off[k + 1]], c["C"]) for k, p in enumerate(c["pos"])])


def _run(c, bin, rows=None, row_off=None, short=0, nrec=None, stream=None):
    """One call of the entry; the three outputs hold 0xFF bytes on entry.  -> (rc, counts, bins, bad)"""
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    C = c["C"]
    rows = c["rows"] if rows is None else rows
    row_off = c["row_off"] if row_off is None else row_off
    n = len(c["h_off"]) if nrec is None else nrec
    bin_off = sc.reserved_bins(c["h_len"], bin)
    d_raw = torch.from_numpy(np.frombuffer(c["buf"], np.uint8).copy()).to(dev)
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    d_counts = torch.full((len(c["h_off"]) * C * 10 * 8,), 0xFF, dtype=torch.uint8, device=dev)
    d_bins = torch.full((max(int(bin_off[-1]), 1) * C * 8,), 0xFF, dtype=torch.uint8, device=dev)
    d_bad = torch.full((8,), 0xFF, dtype=torch.uint8, device=dev)
    wb = int(L.dgrp_repeat_summary_workspace_bytes(len(c["h_off"]), int(c["h_len"].sum()), len(rows)))
    work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream() if stream is None else stream
    rc = L.dgrp_repeat_summary_batch(d_raw.data_ptr(), n, c["h_off"].ctypes.data, c["h_len"].ctypes.data, d_rows.data_ptr(),
                                     row_off.ctypes.data, C, bin, bin_off.ctypes.data if bin else None, d_counts.data_ptr(),
                                     d_bins.data_ptr(), d_bad.data_ptr(), work.data_ptr(), wb - short, st.cuda_stream)
    st.synchronize()
    counts = d_counts.cpu().numpy().view(np.int64).reshape(-1, C, 5, 2)
    bins = d_bins.cpu().numpy().view(np.int64).reshape(-1, C)
    return rc, counts, bins, int(d_bad.cpu().numpy().view(np.int64)[0])


@pytest.mark.parametrize("bin", BINS)
@pytest.mark.parametrize("C", CLASSES)
def test_counts_and_bins_equal_the_numpy_statement(C, bin):
    c = _case(C)
    assert bin < LONGER or all(p.size < LONGER for p in c["pos"])
    rc, counts, bins, bad = _run(c, bin)
    assert rc == 0, last_error()
    assert bad == -1
    np.testing.assert_array_equal(counts, c["counts"])
    if bin:
        np.testing.assert_array_equal(bins, _want_bins(C, bin))
    else:
        assert (bins == -1).all()                                          # without a bin the table is not touched


@pytest.mark.parametrize("bin", (0, 7, 4096))
@pytest.mark.parametrize("C", (5, 16))
def test_a_workgroup_that_walks_several_tiles(C, bin):
    """More than 2 * 2048 tiles: every workgroup walks several consecutive tiles, as on a chromosome.  It changes record inside its
    range (the flush in the middle of the loop, the counters zeroed and used again), two records run from one workgroup's range
    into the next one's, the last workgroup's range is short.  Bins of 7 cut every tile into several bins; with bins of 4096 the
    short records' tiles lie in one bin each (the LDS bin columns, reused from tile to tile) and the long records have tiles of
    both forms.  C = 16 has 16 copies of every counter, C = 5 has 64."""
    c = _case(C, "many_tiles")
    rc, counts, bins, bad = _run(c, bin)
    assert rc == 0, last_error()
    assert bad == -1
    np.testing.assert_array_equal(counts, c["counts"])
    if bin:
        want = _want_bins(C, bin, "many_tiles")
        np.testing.assert_array_equal(bins, want)
        if bin == 4096:
            assert (want[:, 1:].sum(axis=1) > 0).sum() > 1000            # the one-bin form carried counts
    # a bad row in the second long record: left out there and nowhere else
    if bin == 7:
        rows = c["rows"].copy()
        k = 3001
        bad_at = int(c["row_off"][k]) + 2
        rows[bad_at]["label"] = C
        absent, row_off = np.delete(rows, bad_at), c["row_off"].copy()
        row_off[k + 1:] -= 1
        rc, counts, _bins, got = _run(c, bin, rows=rows)
        assert rc == 0 and got == bad_at
        np.testing.assert_array_equal(counts, _counts_for(c, absent, row_off))


def test_called_twice_on_one_stream_the_entry_gives_the_same_bytes():
    """The outputs hold 0xFF on entry: the entry zeroes them itself, and integer atomics give the same bytes in any order."""
    c = _case(5)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a = _run(c, 7, stream=stream)
        b = _run(c, 7, stream=stream)
    assert a[0] == 0 and b[0] == 0
    assert a[1].tobytes() == b[1].tobytes() == c["counts"].tobytes()
    assert a[2].tobytes() == b[2].tobytes() == _want_bins(5, 7).tobytes()
    assert a[3] == b[3] == -1


def test_a_workspace_one_byte_short_is_enomem():
    c = _case(5)
    rc, counts, bins, bad = _run(c, 7, short=1)
    assert rc == ENOMEM and "workspace too small" in last_error()
    assert (counts == -1).all() and (bins == -1).all() and bad == -1      # nothing was queued: the 0xFF bytes stand


def test_no_record_is_ok_and_touches_nothing():
    c = _case(5)
    rc, counts, bins, bad = _run(c, 7, nrec=0)
    assert rc == 0
    assert counts.tobytes() == b"\xff" * counts.nbytes and bins.tobytes() == b"\xff" * bins.nbytes and bad == -1


@pytest.mark.parametrize("what", ["label_high", "label_negative", "empty", "order", "beyond"])
def test_a_bad_row_is_named_and_left_out(what):
    """Each kind of bad row: its index in d_bad, and every count as if the row were absent."""
    c = _case(5)
    rows = c["rows"].copy()
    k = next(k for k in range(len(c["h_off"])) if c["row_off"][k + 1] - c["row_off"][k] >= 6 and c["pos"][k].size > 3000)
    lo, hi = int(c["row_off"][k]), int(c["row_off"][k + 1])
    n = c["pos"][k].size
    if what == "label_high":
        bad = lo + 2
        rows[bad]["label"] = 5
    elif what == "label_negative":
        bad = lo + 3
        rows[bad]["label"] = -1
    elif what == "empty":
        bad = lo + 1
        rows[bad]["end"] = rows[bad]["start"]
    elif what == "order":
        bad = next(i for i in range(lo, hi - 1) if rows[i + 1]["end"] - rows[i + 1]["start"] >= 2)
        rows[bad]["end"] = rows[bad + 1]["start"] + 1
    else:
        bad = hi - 1
        rows[bad]["end"] = n + 1
    absent = np.delete(rows, bad)
    row_off = c["row_off"].copy()
    row_off[k + 1:] -= 1
    want = _counts_for(c, absent, row_off)
    rc, counts, bins, got = _run(c, 7, rows=rows)
    assert rc == 0, last_error()
    assert got == bad
    np.testing.assert_array_equal(counts, want)
    rc, counts2, bins2, got2 = _run(c, 7, rows=absent, row_off=row_off)
    assert rc == 0 and got2 == -1
    np.testing.assert_array_equal(counts2, want)
    np.testing.assert_array_equal(bins, bins2)


def test_two_bad_rows_name_the_first():
    c = _case(5)
    rows = c["rows"].copy()
    rows[40]["label"] = 9
    rows[17]["label"] = -2
    rc, _counts, _bins, bad = _run(c, 0, rows=rows)
    assert rc == 0 and bad == 17


def test_the_host_tables_are_checked_first():
    from deepgrp_amd._lib import lib
    L = lib()
    c = _case(5)
    for C in (1, 65):
        rc = L.dgrp_repeat_summary_batch(None, 1, c["h_off"].ctypes.data, c["h_len"].ctypes.data, None, c["row_off"].ctypes.data, C, 0,
                                         None, None, None, None, None, 0, None)
        assert rc == -1 and "classes" in last_error()
    short = sc.reserved_bins(c["h_len"], 7)
    short[-1] -= 1
    rc = L.dgrp_repeat_summary_batch(None, len(c["h_off"]), c["h_off"].ctypes.data, c["h_len"].ctypes.data, None, c["row_off"].ctypes.data,
                                     5, 7, short.ctypes.data, None, None, None, None, 1 << 40, None)
    assert rc == -1 and "bins" in last_error()
    assert L.dgrp_repeat_summary_workspace_bytes(-1, 0, 0) == 0 and L.dgrp_repeat_summary_workspace_bytes(1, 4096, 0) > 0


def test_stream_contract_behind_a_delayed_producer():
    """Issued on a non-default stream whose producer still sits behind a delay, the entry returns at once and the result is that
    of the idle default stream: the reference counts.  The host tables are scribbled as soon as the call has returned."""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import require_gpu
    L = lib()
    H = Harness(require_gpu())
    assert H.choose_side(L) is not None, H.control
    c = _case(5)
    C, bin = 5, 7
    nrec = len(c["h_off"])
    real = np.frombuffer(c["buf"], np.uint8).copy()
    poison = np.where((real == 10) | (real == 13), real, np.uint8(ord("n")))          # the same positions, other bytes
    rows_poison = c["rows"].copy()
    rows_poison["label"] = 0
    bin_off = sc.reserved_bins(c["h_len"], bin)
    wb = int(L.dgrp_repeat_summary_workspace_bytes(nrec, int(c["h_len"].sum()), len(c["rows"])))

    def call(b, wk, stream, t):
        return L.dgrp_repeat_summary_batch(b["raw"].data_ptr(), nrec, t["off"].ctypes.data, t["len"].ctypes.data, b["rows"].data_ptr(),
                                           t["row_off"].ctypes.data, C, bin, t["bin_off"].ctypes.data, b["counts"].data_ptr(),
                                           b["bins"].data_ptr(), b["bad"].data_ptr(), wk.data_ptr(), wb, stream), None

    late, *_ = H.run(call, {"raw": (real, poison), "rows": (c["rows"].view(np.uint8), rows_poison.view(np.uint8))},
                     {"counts": np.full(nrec * C * 10, -7, np.int64), "bins": np.full(int(bin_off[-1]) * C, -7, np.int64),
                      "bad": np.full(1, -7, np.int64)}, work_bytes=wb,
                     tables={"off": c["h_off"], "len": c["h_len"], "row_off": c["row_off"], "bin_off": bin_off})
    np.testing.assert_array_equal(late["counts"].reshape(nrec, C, 5, 2), c["counts"])
    np.testing.assert_array_equal(late["bins"].reshape(-1, C), _want_bins(C, bin))
    assert late["bad"].tolist() == [-1]
