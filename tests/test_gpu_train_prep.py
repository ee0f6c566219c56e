"""`train` from a sequence file on the GPU: dgrp_truth_multihot_batch, dgrp_class_window_starts and dgrp_train_resolve_starts against
the numpy statement (tests/train_prep_oracle.py), byte for byte, every output between guard bytes that must survive; then
training() on a DeviceData against training() on the host Data of the same record."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import train_prep_oracle as tpo

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -3
GUARD, FILL = 64, 0x5A
SET_BLOCK = 8192                                  # window starts per workgroup of the class-set kernels as built
SEGMENT = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


def _lib():
    from deepgrp_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(nbytes):
    """A device buffer of FILL bytes with GUARD bytes either side of the `nbytes` an entry may write (16-byte aligned)."""
    whole = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == FILL).all() and (host[GUARD + nbytes:] == FILL).all())


def _err():
    return _lib()[1].dgrp_last_error().decode()


# ------------------------------------------------------------------------------------------------ truth
LENGTHS = [1, 63, 64, 65, 8191, 8192, 8193, 20000]


def _truth_side(classes):
    """Records back to back with non-zero origins, and their rows in original coordinates."""
    rng = np.random.default_rng(classes)
    ln = np.array(LENGTHS, np.int64)
    off = np.concatenate(([0], np.cumsum(ln)))[:-1].astype(np.int64)
    org = np.array([7, 1000, 3, 50, 123456, 1, 99, 5_000_000_000], np.int64)        # (one beyond 2^32)
    top, two = classes - 1, min(2, classes - 1)
    rows = [[] for _ in ln]
    rows[0] = [(org[0], org[0] + 1, top)]                                # the whole one-base record, the highest label
    rows[1] = []                                                         # no rows: row 0 all ones
    rows[2] = [(org[2] + 60, org[2] + 64 + 10, 1)]                       # ends past the record's last base: clipped, record 3 untouched
    rows[3] = [(org[3] - 5, org[3] + 3, two)]                            # starts before the first base of the next record: clipped
    g = org[4]
    rows[4] = [(g + 100, g + 300, 1), (g + 100, g + 300, top),           # two classes on the same bases
               (g + 200, g + 500, 1),                                    # the same class overlapping itself
               (g - 50, g + 20, two), (g + 8000, g + 9000, top),         # clipped at either end
               (g + 10000, g + 10100, 1), (0, g - 1, 1),                 # wholly outside, after and before
               (g + 40, g + 40, 1)]                                      # empty
    rows[5] = [(org[5], org[5] + 8192, top), (org[5] + 8191, org[5] + 8192, 1)]      # the whole record; its last base
    for r in (6, 7):
        n = int(ln[r])
        starts = rng.integers(-100, n + 100, 60)
        sizes = np.where(rng.random(60) < 0.1, rng.integers(8000, 12000, 60), rng.integers(0, 400, 60))
        rows[r] = [(int(org[r] + max(s, -int(org[r]))), int(org[r] + max(s, -int(org[r])) + z), int(rng.integers(1, classes)))
                   for s, z in zip(starts, sizes)]
    return off, ln, org, [[(int(a), int(b), int(c)) for a, b, c in rr] for rr in rows]


def _call_truth(classes, off, ln, org, rows, view):
    _l, L = _lib()
    n_total = int(ln.sum())
    row_off = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    flat = np.zeros(int(row_off[-1]), SEGMENT)
    k = 0
    for rr in rows:
        for a, b, c in rr:
            flat[k] = (a, b, c, 0)
            k += 1
    d_rows = torch.from_numpy(flat.view(np.uint8)).cuda() if flat.size else None
    wb = L.dgrp_truth_workspace_bytes(len(ln), int(row_off[-1]))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    return L.dgrp_truth_multihot_batch(view.data_ptr(), classes, n_total, len(ln), off.ctypes.data, ln.ctypes.data, org.ctypes.data,
                                       d_rows.data_ptr() if d_rows is not None else None, row_off.ctypes.data, work.data_ptr(), wb,
                                       _stream())


@pytest.mark.parametrize("classes", [2, 5, 16])
def test_truth_equals_the_statement_byte_for_byte(classes):
    off, ln, org, rows = _truth_side(classes)
    n_total = int(ln.sum())
    want = tpo.truth(classes, n_total, off, ln, org, rows)
    assert want[0, off[1]:off[1] + ln[1]].all() and want[classes - 1, off[0]] == 1 and (want.sum(axis=0) >= 1).all()
    assert want[1, off[2] + 63] == 1 and not want[1:, off[3] + 3:off[3] + 65].any()
    if classes > 2:
        assert (want[1:, off[4] + 100:off[4] + 300].sum(axis=0) == 2).all()           # two classes on one base give two ones
    whole, view = _guarded(classes * n_total)
    assert _call_truth(classes, off, ln, org, rows, view) == 0, _err()
    got = view.cpu().numpy().view(np.int8).reshape(classes, n_total)
    assert np.array_equal(got, want)
    assert _guards_intact(whole, classes * n_total)
    again, view2 = _guarded(classes * n_total)
    assert _call_truth(classes, off, ln, org, rows, view2) == 0
    assert torch.equal(view, view2)


def test_truth_without_rows_is_all_background():
    off, ln, org, rows = _truth_side(5)
    n_total = int(ln.sum())
    whole, view = _guarded(5 * n_total)
    assert _call_truth(5, off, ln, org, [[] for _ in rows], view) == 0, _err()
    got = view.cpu().numpy().reshape(5, n_total)
    assert (got[0] == 1).all() and not got[1:].any() and _guards_intact(whole, 5 * n_total)


@pytest.mark.parametrize("bad,word", [((10, 20, 5), "label 5"), ((30, 29, 1), "[30, 29)")], ids=["label-C", "end-below-start"])
def test_a_bad_row_is_named_before_anything_is_written(bad, word):
    off, ln, org, rows = _truth_side(5)
    n_total = int(ln.sum())
    rows[6] = rows[6][:7] + [bad] + rows[6][7:]
    index = sum(len(r) for r in rows[:6]) + 7
    whole, view = _guarded(5 * n_total)
    assert _call_truth(5, off, ln, org, rows, view) == EINVAL
    assert f"row {index} " in _err() and word in _err(), _err()
    assert (whole.cpu().numpy() == FILL).all()


# ------------------------------------------------------------------------------------------------ class sets
def _set_side(T):
    """A class row over many records: (row int8 [n_total], off, len).  Lengths around the first window (T .. T + 3), one start
    either side of the workgroup's SET_BLOCK starts, two workgroups and a bit; single ones at 0, 1, 2, T and n - 1; runs longer than
    T; a run on the last bases of a record in front of a record that starts with zeros, and the other way round."""
    rng = np.random.default_rng(T)
    recs = []

    def add(n, ones=(), runs=(), density=0.0):
        row = (rng.random(n) < density).astype(np.int8)
        for p in ones:
            row[p] = 1
        for a, b in runs:
            row[a:b] = 1
        recs.append(row)

    for n in (T, T + 1, T + 2, T + 3):
        add(n, density=0.5)
        add(n, ones=[n - 1])
        add(n, ones=[0])
    small = 2 * T + 10
    for p in (0, 1, 2, T, small - 1):
        add(small, ones=[p])
    add(3 * T + 20, runs=[(T // 2 + 3, T // 2 + 3 + 2 * T + 1)])                      # a run longer than the window
    add(small, runs=[(small - 3, small)])                                            # record A ends in a run ...
    add(small)                                                                       # ... record B is empty: no start of B is a member
    add(small, runs=[(0, 3)])                                                        # and C starts with one: no start of B reaches it
    for members in (SET_BLOCK - 1, SET_BLOCK, SET_BLOCK + 1, 2 * SET_BLOCK + 77):
        add(members + 1 + T, density=1.0 / (2 * T + 3), ones=[members + T])          # sparse, and a one on the last base
    add(SET_BLOCK + 1 + T, ones=[SET_BLOCK + T])                                     # only the last start of the second workgroup
    add(0)
    add(1, ones=[0])
    ln = np.array([len(r) for r in recs], np.int64)
    off = np.concatenate(([0], np.cumsum(ln)))[:-1].astype(np.int64)
    return np.concatenate(recs), off, ln


def _call_starts(d_row, n_total, off, ln, T, out_view, cap):
    _l, L = _lib()
    wb = L.dgrp_class_starts_workspace_bytes(len(ln), n_total)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    count = C.c_int64(-7)
    rc = L.dgrp_class_window_starts(d_row.data_ptr(), n_total, len(ln), off.ctypes.data, ln.ctypes.data, T,
                                    out_view.data_ptr() if out_view is not None else None, cap, C.byref(count), work.data_ptr(), wb,
                                    _stream())
    return rc, int(count.value)


@pytest.mark.parametrize("T", [1, 2, 7, 64, 200, 4096])
def test_class_sets_equal_the_statement(T):
    row, off, ln = _set_side(T)
    n_total = row.size
    want = tpo.class_starts(row, off, ln, T)
    assert want.size > 4000                                            # several workgroups hold members
    # no member's window leaves its record
    rec = np.searchsorted(off + ln, want, side="right")
    assert ((want >= off[rec] + 1) & (want + T <= off[rec] + ln[rec] - 1)).all()
    # the row sits in the middle of a buffer of ones: a window read outside [0, n_total) would add members
    around = torch.ones(n_total + 2 * 8192, dtype=torch.int8, device="cuda")
    d_row = around[8192:8192 + n_total]
    d_row.copy_(torch.from_numpy(row))
    rc, count = _call_starts(d_row, n_total, off, ln, T, None, 0)                   # count only
    assert rc == 0 and count == want.size, _err()
    whole, view = _guarded(8 * want.size)
    rc, count = _call_starts(d_row, n_total, off, ln, T, view, want.size)
    assert rc == 0 and count == want.size, _err()
    assert np.array_equal(view.cpu().numpy().view(np.int64), want) and _guards_intact(whole, 8 * want.size)
    # too small a capacity: the needed count comes back and nothing is written
    whole, view = _guarded(8 * (want.size - 1))
    rc, count = _call_starts(d_row, n_total, off, ln, T, view, want.size - 1)
    assert rc == ENOMEM and count == want.size and (whole.cpu().numpy() == FILL).all()
    # a row of zeros: count 0, nothing written
    zeros = torch.zeros(n_total, dtype=torch.int8, device="cuda")
    whole, view = _guarded(64)
    rc, count = _call_starts(zeros, n_total, off, ln, T, view, 8)
    assert rc == 0 and count == 0 and (whole.cpu().numpy() == FILL).all()


def test_class_sets_single_ones_by_hand():
    """s = 0 is never a member, s = 1 is one as soon as the window (1, 1 + T] holds a one."""
    T, n = 7, 40
    for p, members in ((0, []), (1, []), (2, [1]), (T, list(range(1, T))), (n - 1, list(range(n - 1 - T, n - 1 - T + 1)))):
        row = np.zeros(n, np.int8)
        row[p] = 1
        want = tpo.class_starts(row, [0], [n], T)
        assert want.tolist() == members, p
        whole, view = _guarded(8 * max(len(members), 1))
        rc, count = _call_starts(torch.from_numpy(row).cuda(), n, np.zeros(1, np.int64), np.array([n], np.int64), T, view, max(len(members), 1))
        assert rc == 0 and count == len(members), _err()
        assert view.cpu().numpy().view(np.int64)[:count].tolist() == members


# ------------------------------------------------------------------------------------------------ resolve
def _resolve(picks, sets, off, ln, T):
    _l, L = _lib()
    dev = "cuda"
    d_sets = [torch.from_numpy(np.ascontiguousarray(s, np.int64)).to(dev) for s in sets]
    table = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)
    d_ptr, d_size = table([t.data_ptr() for t in d_sets] or [0]), table([len(s) for s in sets] or [0])
    d_base, d_prefix = table(off), table(tpo.window_prefix(ln, T))
    d_picks = table(picks)
    B = len(picks)
    whole, view = _guarded(8 * B)
    rc = L.dgrp_train_resolve_starts(d_picks.data_ptr(), B, d_ptr.data_ptr(), d_size.data_ptr(), len(sets), d_base.data_ptr(),
                                     d_prefix.data_ptr(), len(ln), view.data_ptr(), _stream())
    assert rc == 0, _err()
    assert _guards_intact(whole, 8 * B)
    return view.cpu().numpy().view(np.int64)


def test_resolve_maps_every_rank_as_the_statement_says():
    T = 30
    ln = np.array([100, 12, 31], np.int64)                               # the second record is shorter than the window
    off = np.array([0, 100, 112], np.int64)
    W = int(tpo.window_prefix(ln, T)[-1])
    assert W == 70 + 0 + 1
    picks = [(-1, k) for k in range(W)]
    got = _resolve(picks, [], off, ln, T)
    assert got.tolist() == list(range(70)) + [112]
    assert np.array_equal(got, tpo.resolve(picks, [], off, ln, T))
    sets = [np.array([3, 9, 40, 41, 69], np.int64), np.array([112], np.int64), np.zeros(0, np.int64)]
    picks = [(0, 0), (0, 4), (0, 2), (1, 0), (2, 5), (-1, 70), (3, 1), (0, 5), (0, 1 << 40), (1, 7), (-1, W), (-1, 1 << 50), (-1, -1),
             (0, -9), (1 << 40, 3), (-5, 2)]
    want = tpo.resolve(picks, sets, off, ln, T)
    assert want.tolist() == [3, 69, 40, 112, 5, 112, 1, 69, 69, 112, 112, 112, 0, 3, 3, 2]
    assert np.array_equal(_resolve(picks, sets, off, ln, T), want)
    # no window anywhere: the start is 0
    assert _resolve([(-1, 5), (0, 1)], [], np.zeros(1, np.int64), np.array([10], np.int64), T).tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ end to end
def test_training_on_a_sequence_file_is_training_on_its_npz(tmp_path):
    """units 4, vecsize 20, batch 8, attention, dropout 0.25, RMSprop, 2 epochs x 3 batches: the returned tensors and the history of
    training() on DeviceData.from_sequence_file equal those of training() on the host Data of the same record, byte for byte."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import preprocessing, synthetic, training
    n = 3000
    idx, _lab = synthetic.synthetic_truth(n, contig=3, flank=50)
    fasta, bed = tmp_path / "chrA.fa", tmp_path / "rm.bed"
    seq = np.frombuffer(b"ACGTN", np.uint8)[idx].tobytes()
    fasta.write_bytes(b">chrA synthetic\n" + b"\n".join(seq[o:o + 60] for o in range(0, n, 60)) + b"\n")
    bed.write_text("".join(synthetic.synthetic_annotation(n, contig=3, name="chrA", flank=50)))
    opt = dgmodel.Options(units=4, vecsize=20, batch_size=8, attention=True, dropout=0.25, optimizer="RMSprop", n_epochs=2, n_batches=3)
    fwd = np.zeros((5, n), np.int8)
    fwd[idx, np.arange(n)] = 1
    y = preprocessing.preprocess_y(bed, "chrA", n, opt.repeats_to_search)
    host = preprocessing.Data(*preprocessing.drop_start_end_n(fwd, y))
    dev = training.DeviceData.from_sequence_file(fasta, bed, opt.repeats_to_search, vecsize=opt.vecsize)
    assert dev.names == ["chrA"] and dev.n == host.truelbl.shape[1] and dev.startpos.tolist() == [50]
    assert np.array_equal(dev.d_truth.cpu().numpy(), host.truelbl)
    assert np.array_equal(dev.d_idx.cpu().numpy(), training.onehot_to_index(host.fwd))
    out = []
    for name, data in (("host", (host, host)), ("device", (dev, dev))):
        weights = dgmodel.initial_weights(opt, 11)
        logdir = str(tmp_path / name)
        best = training.training(data, opt, weights, logdir, seed=11)
        out.append((best, open(os.path.join(logdir, "history.tsv"), "rb").read(), sorted(os.listdir(logdir))))
    (a, hist_a, files_a), (b, hist_b, files_b) = out
    assert hist_a == hist_b and files_a == files_b and len(hist_a.splitlines()) == 3
    assert a["history"] == b["history"]
    for k in ("kernel", "recurrent_kernel", "bias", "scale", "ff_kernel", "ff_bias"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for f in files_a:
        assert open(os.path.join(str(tmp_path), "host", f), "rb").read() == open(os.path.join(str(tmp_path), "device", f), "rb").read(), f
    # the uploaded form of the host arrays samples on the device as well, to the same bytes
    up = training.DeviceData.from_data(host)
    best = training.training((up, up), opt, dgmodel.initial_weights(opt, 11), str(tmp_path / "uploaded"), seed=11)
    assert all(best[k].tobytes() == a[k].tobytes() for k in ("kernel", "recurrent_kernel", "bias", "scale", "ff_kernel", "ff_bias"))
