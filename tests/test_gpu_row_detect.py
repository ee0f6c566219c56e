"""dgrp_paint_row_keys_batch and dgrp_row_detect_batch on the GPU, against curves.reference_detect (every m tried in numpy) on one
batch of records made once, and -- without that statement -- against the entries `evaluate` already has: the rows with score >= m
painted by dgrp_paint_rows_batch and counted by dgrp_row_hits_batch must find an element exactly when its detection score is >= m.
Every comparison is integer or byte equality.

The batch: record lengths at the lane, wave and slice edges (0, 1, 63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 5) with non-zero
origins and sentinel gaps between the records of the key track; predicted rows from none to runs of one base, labels 1..4 and 63,
scores 0, 1, 499, 500, 1000 and random ones, equal neighbours, rows sticking out at both ends; annotation rows overlapping, nested,
in reverse order, empty, outside, one over more than two slices, 5000 single-base ones behind each other (more rows in a slice than
its LDS counters hold), needs from theta 1e-9, 0.5 and 1.0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import SEG, Harness, i64ptr, last_error      # noqa: E402

EINVAL, ENOMEM = -1, -3
LENGTHS = [0, 1, 63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 5]
SPECIAL = (0, 1, 499, 500, 1000)
KEY_SENTINEL, DET_SENTINEL = 0xBEEF, -77
P0, T0 = 2, 3                                   # rows in front of the first record's rows: never read


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _scores_for(clen, want):
    """ROW_SCORE_DTYPE entries whose BED score is `want` (rows without a base inside their record stay all zero: unscored)."""
    from deepgrp_amd.curves import row_scores_of
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE
    sc = np.zeros(len(clen), ROW_SCORE_DTYPE)
    ok = clen > 0
    sc["bases"][ok] = clen[ok]
    sc["sum"][ok] = [(int(w) * (int(b) << 24) + 999) // 1000 for w, b in zip(want[ok], clen[ok])]
    sc["agree"][ok] = clen[ok] // 2
    sc["qmin"][ok] = 5
    assert (row_scores_of(sc[ok]) == want[ok]).all()
    return sc


def _pred_rows(rng, k, n, o):
    """Ascending rows that do not overlap, as predict writes them: [(start, end, label)], [score]"""
    labs = (1, 2, 3, 4, 63)
    if k == 0:
        return [(o + 3, o + 9, 1)], [0]                                  # the record has no base: the row is unscored and ignored
    if k == 1:
        return [(o - 3, o + 4, 63)], [1000]                              # sticks out at both ends
    if k == 2:
        return [], []
    if k == 3:
        return [(o, o + n, 2)], [500]                                    # the whole record
    if k == 4:
        return [(o + i, o + i + 1, labs[i % 5]) for i in range(n)], [SPECIAL[(i // 2) % 5] for i in range(n)]    # runs of one base
    rows, scores, p = [], [], o - 40                                     # the first row starts in front of the record
    i = 0
    while p < o + n + 30:                                                # the last one ends behind it
        ln = int(rng.integers(1, 400)) if k < 8 else int(rng.integers(1, 3000))
        rows.append((max(p, 0), p + ln, labs[i % 5] if rng.random() < 0.7 else labs[int(rng.integers(0, 5))]))
        scores.append(int(rng.choice(SPECIAL)) if rng.random() < 0.5 else int(rng.integers(0, 1001)))
        if i % 7 == 3:                                                   # an equal neighbour: same label and score, touching
            rows.append((p + ln, p + ln + 17, rows[-1][2]))
            scores.append(scores[-1])
            ln += 17
        if i % 7 == 5:                                                   # same label, another score, touching
            rows.append((p + ln, p + ln + 9, rows[-1][2]))
            scores.append((scores[-1] + 1) % 1001)
            ln += 9
        p += ln + (int(rng.integers(0, 60)) if rng.random() < 0.6 else 0)
        i += 1
    return rows, scores


def _true_rows(rng, k, n, o):
    labs = (1, 2, 3, 4, 63, 5)                                           # 5 is never predicted
    rows = []
    for _ in range(int(rng.integers(8, 40))):                            # overlapping, any class
        s = int(rng.integers(max(o - 60, 0), o + n + 60))
        rows.append((s, s + int(rng.integers(0, min(n, 1500) + 2)), labs[int(rng.integers(0, 6))]))
    if n > 100:                                                          # nested, same class and other classes
        s = o + int(rng.integers(0, n // 2))
        e = s + int(rng.integers(30, n - (s - o) + 1))
        rows += [(s, e, 3), (s + 5, e - 5, 1), (s + 7, e - 9, 3), (s + 8, s + 8 + (e - s) // 3, 2)]
    rows += [(o + n // 2, o + n // 2, 1), (o, o, 2)]                      # zero length
    rows += [(max(o - 30, 0), o + min(n, 7), 4), (o + n - min(n, 9), o + n + 25, 2), (0, o + n + 5000, 63), (0, o + n + 1, 1)]
    rows += [(o + n, o + n + 50, 1), (o + n + 10, o + n + 11, 2), (0, o - 1, 1)]          # outside
    if k == 4:
        rows += [(o + i, o + i + 1, labs[i % 5]) for i in range(30)]      # on the runs of one base: every special score comes out
    if k == 8:
        rows.append((o + 100, o + 100 + 2 * 8192 + 4000, 2))             # more than two slices
    if k == 6:
        rows += [(o + 1000 + i, o + 1001 + i, (1, 2, 3, 4, 63)[i % 5]) for i in range(5000)]      # 5000 in a row on the line
    rows.sort(key=lambda r: -r[0])                                       # reverse order ...
    if k % 2:
        rows = [rows[i] for i in rng.permutation(len(rows))]             # ... or any
    return rows


def _seg(rows):
    a = np.zeros(len(rows), SEG)
    for i, (s, e, lab) in enumerate(rows):
        a[i] = (s, e, lab, 0)
    return a


@pytest.fixture(scope="module")
def batch():
    """The records, their rows, scores and needs, the tables as the entries take them, and the statement -- made once, read only."""
    from deepgrp_amd import curves
    from deepgrp_amd.evaluation import clipped_lengths
    rng = np.random.default_rng(20250)
    nrec = len(LENGTHS)
    org = [int(rng.integers(50, 5000)) for _ in LENGTHS]
    off, p = [], 7
    for n in LENGTHS:
        off.append(p)
        p += n + int(rng.integers(1, 40))                                # elements between the records nobody may write
    size = p + 11
    pred, pscore, true, need = [], [], [], []
    thetas = (1e-9, 0.5, 1.0)
    for k, (n, o) in enumerate(zip(LENGTHS, org)):
        rows, want = _pred_rows(rng, k, n, o)
        pr = _seg(rows)
        pred.append(pr)
        pscore.append(_scores_for(clipped_lengths(pr, o, n), np.array(want, np.int64).reshape(len(rows))))
        tr = _seg(_true_rows(rng, k, n, o))
        clen = clipped_lengths(tr, o, n)
        nd = np.array([curves.need_of(thetas[j % 3], clen[j:j + 1])[0] for j in range(len(tr))], np.int64)
        live = np.flatnonzero(clen > 0)
        if len(live) > 1:
            nd[live[0]] = 0                                              # needs nothing: -1 by definition
            nd[live[1]] = clen[live[1]] + 1                              # needs more than it has
        true.append(tr)
        need.append(nd)
    junk = np.zeros(1, SEG)
    junk[0] = (-5, -9, 99, 0)                                            # a row no check would pass, outside the offsets
    p_flat = np.concatenate([np.repeat(junk, P0)] + pred + [junk])
    s_flat = np.concatenate([np.zeros(P0, pscore[0].dtype)] + pscore + [np.zeros(1, pscore[0].dtype)])
    t_flat = np.concatenate([np.repeat(junk, T0)] + true + [junk])
    n_flat = np.concatenate([np.full(T0, 1 << 40, np.int64)] + need + [np.full(1, 1 << 40, np.int64)])
    p_off = (P0 + np.cumsum([0] + [len(x) for x in pred])).astype(np.int64)
    t_off = (T0 + np.cumsum([0] + [len(x) for x in true])).astype(np.int64)
    ints = [curves.row_scores_of(s[s["bases"] > 0]) for s in pscore]
    full = []
    for s, v in zip(pscore, ints):
        a = np.zeros(len(s), np.int64)
        a[s["bases"] > 0] = v
        full.append(a)
    keys, det = curves.reference_detect(org, LENGTHS, pred, full, true, need)
    want_keys = np.full(size, KEY_SENTINEL, np.uint16)
    for r in range(nrec):
        want_keys[off[r]:off[r] + LENGTHS[r]] = keys[r]
    track0 = np.full(size, KEY_SENTINEL, np.uint16)
    for r in range(nrec):
        track0[off[r]:off[r] + LENGTHS[r]] = 0                           # the caller zeroes the records
    tabs = dict(off=np.array(off, np.int64), len=np.array(LENGTHS, np.int64), org=np.array(org, np.int64), po=p_off, to=t_off)
    for a in (want_keys, track0, det, p_flat, s_flat, t_flat, n_flat, *tabs.values()):
        a.setflags(write=False)
    return dict(nrec=nrec, size=size, tabs=tabs, p_flat=p_flat, s_flat=s_flat, t_flat=t_flat, n_flat=n_flat, want_keys=want_keys,
                track0=track0, det=det, pred_int=np.concatenate(full), nrows=max(len(p_flat), len(t_flat)))


def _d(a, dev):
    return torch.from_numpy(np.array(a, order="C", copy=True).view(np.uint8).reshape(-1)).to(dev)


def _paint(L, dev, b, fill=0xA5, stream=None):
    """-> (rc, key track as numpy)"""
    t = b["tabs"]
    wb = L.dgrp_row_detect_workspace_bytes(b["nrec"], b["nrows"])
    work = torch.full((wb,), fill, dtype=torch.uint8, device=dev)
    d_keys, d_rows, d_sc = _d(b["track0"], dev), _d(b["p_flat"], dev), _d(b["s_flat"], dev)
    rc = L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), b["nrec"], i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), d_rows.data_ptr(),
                                     i64ptr(t["po"]), d_sc.data_ptr(), work.data_ptr(), wb, stream)
    torch.cuda.synchronize()
    return rc, d_keys.cpu().numpy().view(np.uint16)


def _detect(L, dev, b, keys, fill=0xA5, stream=None):
    """-> (rc, d_detect as numpy, whole array)"""
    t = b["tabs"]
    wb = L.dgrp_row_detect_workspace_bytes(b["nrec"], b["nrows"])
    work = torch.full((wb,), fill, dtype=torch.uint8, device=dev)
    d_keys, d_rows, d_need = _d(keys, dev), _d(b["t_flat"], dev), _d(b["n_flat"], dev)
    d_det = torch.full((len(b["t_flat"]),), DET_SENTINEL, dtype=torch.int32, device=dev)
    rc = L.dgrp_row_detect_batch(d_keys.data_ptr(), b["nrec"], i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), d_rows.data_ptr(),
                                 i64ptr(t["to"]), d_need.data_ptr(), d_det.data_ptr(), work.data_ptr(), wb, stream)
    torch.cuda.synchronize()
    return rc, d_det.cpu().numpy()


@pytest.fixture(scope="module")
def ran(L, dev, batch):
    """Both entries on the batch, once."""
    rc, keys = _paint(L, dev, batch)
    assert rc == 0, last_error()
    rc, det = _detect(L, dev, batch, keys)
    assert rc == 0, last_error()
    return keys, det


def test_the_batch_is_what_it_says(batch):
    det, to = batch["det"], batch["tabs"]["to"]
    assert len(det) == to[-1] - T0
    assert {-1, 0, 1, 499, 500, 1000} <= set(det.tolist()) and len(set(det.tolist())) > 20
    assert len(batch["t_flat"]) > 5100 and set(batch["pred_int"].tolist()) >= set(SPECIAL)
    assert {1, 2, 3, 4, 63} <= set((batch["want_keys"][batch["want_keys"] != KEY_SENTINEL] >> 10).tolist())


def test_keys_are_the_statement_and_sentinels_stay(batch, ran):
    keys, _det = ran
    np.testing.assert_array_equal(keys, batch["want_keys"])               # the gaps between the records hold their sentinel


def test_detection_scores_are_the_statement_and_sentinels_stay(batch, ran):
    _keys, det = ran
    to = batch["tabs"]["to"]
    np.testing.assert_array_equal(det[to[0]:to[-1]], batch["det"])
    assert (det[:to[0]] == DET_SENTINEL).all() and (det[to[-1]:] == DET_SENTINEL).all()


@pytest.mark.parametrize("m", [0, 1, 500, 1000])
def test_the_old_entries_agree_at_a_threshold(L, dev, batch, ran, m):
    """Rows with score >= m painted by dgrp_paint_rows_batch, the annotation rows counted against that track by
    dgrp_row_hits_batch: an element has its bases exactly when its detection score is at least m."""
    _keys, det = ran
    t, nrec = batch["tabs"], batch["nrec"]
    po, to = t["po"], t["to"]
    kept_rows, ro = [], [0]
    for r in range(nrec):
        rows, sc = batch["p_flat"][po[r]:po[r + 1]], batch["pred_int"][po[r] - P0:po[r + 1] - P0]
        kept_rows.append(rows[sc >= m])
        ro.append(ro[-1] + len(kept_rows[-1]))
    ro = np.array(ro, np.int64)
    flat = np.concatenate(kept_rows)
    d_rows = _d(flat, dev)
    wb = L.dgrp_eval_workspace_bytes(nrec, max(len(flat), len(batch["t_flat"])))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    d_lab = torch.zeros(batch["size"], dtype=torch.int8, device=dev)
    assert L.dgrp_paint_rows_batch(d_lab.data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), d_rows.data_ptr(), i64ptr(ro),
                                   work.data_ptr(), wb, None) == 0, last_error()
    d_true = _d(batch["t_flat"], dev)
    d_hits = torch.zeros(len(batch["t_flat"]), dtype=torch.int64, device=dev)
    assert L.dgrp_row_hits_batch(d_lab.data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), d_true.data_ptr(), i64ptr(to),
                                 d_hits.data_ptr(), work.data_ptr(), wb, None) == 0, last_error()
    torch.cuda.synchronize()
    hits, need, d = d_hits.cpu().numpy()[to[0]:to[-1]], batch["n_flat"][to[0]:to[-1]], det[to[0]:to[-1]]
    asks = need > 0                                                      # (need <= 0 is -1 by definition, whatever the hits)
    assert asks.sum() > 5000
    np.testing.assert_array_equal((hits >= need)[asks], (d >= m)[asks])
    assert (d[~asks] == -1).all()


def test_two_calls_and_any_workspace_fill_give_the_same_bytes(L, dev, batch, ran):
    keys, det = ran
    for fill in (0x00, 0xFF):
        rc, keys2 = _paint(L, dev, batch, fill)
        assert rc == 0, last_error()
        rc, det2 = _detect(L, dev, batch, keys2, fill)
        assert rc == 0, last_error()
        assert keys2.tobytes() == keys.tobytes() and det2.tobytes() == det.tobytes()


def test_on_a_side_stream_behind_a_late_producer(L, dev, batch, ran):
    """stream_harness: the inputs are poison until copies behind a delay on a side stream put the real ones in place; both entries
    synchronise that stream once (their row check) and order everything else behind it."""
    keys, det = ran
    H = Harness(dev)
    assert H.choose_side(L) is not None, H.control
    b, nrec = batch, batch["nrec"]
    wb = L.dgrp_row_detect_workspace_bytes(nrec, b["nrows"])
    tabs = {k: np.array(v) for k, v in b["tabs"].items()}
    rows_p = np.array(b["p_flat"])
    rows_p["label"] = 1 + rows_p["label"] % 5                            # valid rows of other classes
    sc_p = np.array(b["s_flat"])
    sc_p["sum"] //= 2
    track_p = np.where(b["track0"] == 0, np.uint16(3 << 10 | 7), np.uint16(0x1234)).astype(np.uint16)

    def paint(bf, wk, st, t):
        return L.dgrp_paint_row_keys_batch(bf["keys"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), bf["rows"].data_ptr(),
                                           i64ptr(t["po"]), bf["sc"].data_ptr(), wk.data_ptr(), wb, st), None
    raw = lambda a: np.array(a).view(np.uint8).reshape(-1)
    late, *_ = H.run(paint, {"keys": (raw(b["track0"]), raw(track_p)), "rows": (raw(b["p_flat"]), raw(rows_p)), "sc": (raw(b["s_flat"]), raw(sc_p))},
                     {"keys": None}, work_bytes=wb, sync=True, drained=False, tables=tabs)
    assert late["keys"].tobytes() == keys.tobytes()
    true_p = np.array(b["t_flat"])
    true_p["label"] = 1 + true_p["label"] % 5
    need_p = np.array(b["n_flat"]) + 1
    keys_p = np.where(keys == 0, np.uint16(2 << 10 | 900), np.uint16(0)).astype(np.uint16)

    def detect(bf, wk, st, t):
        return L.dgrp_row_detect_batch(bf["keys"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), bf["rows"].data_ptr(),
                                       i64ptr(t["to"]), bf["need"].data_ptr(), bf["det"].data_ptr(), wk.data_ptr(), wb, st), None
    late, *_ = H.run(detect, {"keys": (raw(keys), raw(keys_p)), "rows": (raw(b["t_flat"]), raw(true_p)), "need": (raw(b["n_flat"]), raw(need_p))},
                     {"det": np.full(len(b["t_flat"]), DET_SENTINEL, np.int32)}, work_bytes=wb, sync=True, drained=False, tables=tabs)
    assert late["det"].tobytes() == det.tobytes()


def test_no_record_and_no_rows_need_no_device_memory(L, dev):
    """nrec == 0, and records without a row: nothing is launched, so NULL device pointers and no workspace are fine and the outputs
    keep their sentinels."""
    z = np.zeros(1, np.int64)
    assert L.dgrp_paint_row_keys_batch(None, 0, None, None, None, None, i64ptr(z), None, None, 0, None) == 0, last_error()
    assert L.dgrp_row_detect_batch(None, 0, None, None, None, None, i64ptr(z), None, None, None, 0, None) == 0, last_error()
    off, ln, org, ro = (np.array(v, np.int64) for v in ([4, 30], [20, 9], [100, 7], [5, 5, 5]))
    d_keys = torch.full((64,), 0x1EEF, dtype=torch.int16, device=dev)
    d_det = torch.full((8,), DET_SENTINEL, dtype=torch.int32, device=dev)
    assert L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), 2, i64ptr(off), i64ptr(ln), i64ptr(org), None, i64ptr(ro), None, None, 0, None) == 0, last_error()
    assert L.dgrp_row_detect_batch(d_keys.data_ptr(), 2, i64ptr(off), i64ptr(ln), i64ptr(org), None, i64ptr(ro), None, d_det.data_ptr(), None, 0,
                                   None) == 0, last_error()
    torch.cuda.synchronize()
    assert (d_keys.cpu().numpy() == 0x1EEF).all() and (d_det.cpu().numpy() == DET_SENTINEL).all()
    # rows, but none with a base inside its record: every detection score is -1, the track is not read
    rows = _seg([(0, 50, 1), (400, 500, 2), (3, 3, 1)])
    ro = np.array([0, 2, 3], np.int64)
    wb = L.dgrp_row_detect_workspace_bytes(2, 3)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    d_need = torch.ones(3, dtype=torch.int64, device=dev)
    d_det = torch.full((5,), DET_SENTINEL, dtype=torch.int32, device=dev)
    d_rows = _d(rows, dev)
    assert L.dgrp_row_detect_batch(None, 2, i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro), d_need.data_ptr(),
                                   d_det.data_ptr(), work.data_ptr(), wb, None) == 0, last_error()
    torch.cuda.synchronize()
    assert d_det.cpu().numpy().tolist() == [-1, -1, -1, DET_SENTINEL, DET_SENTINEL]


def _refused(L, dev, rows, scores_of, wb_cut=0, which="paint"):
    """One record [100, 300) at elements 8..208 of a sentinel track: -> (rc, message, the outputs are untouched)"""
    off, ln, org = (np.array([v], np.int64) for v in (8, 200, 100))
    pr = _seg(rows)
    ro = np.array([0, len(pr)], np.int64)
    from deepgrp_amd.evaluation import clipped_lengths
    sc = scores_of(clipped_lengths(pr, 100, 200))
    wb = L.dgrp_row_detect_workspace_bytes(1, len(pr))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    d_keys = torch.full((220,), 0x1EEF, dtype=torch.int16, device=dev)
    d_det = torch.full((len(pr) + 2,), DET_SENTINEL, dtype=torch.int32, device=dev)
    d_rows, d_sc = _d(pr, dev), _d(sc, dev)
    if which == "paint":
        rc = L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), 1, i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro),
                                         d_sc.data_ptr(), work.data_ptr(), wb - wb_cut, None)
    else:
        d_need = torch.ones(len(pr), dtype=torch.int64, device=dev)
        rc = L.dgrp_row_detect_batch(d_keys.data_ptr(), 1, i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro),
                                     d_need.data_ptr(), d_det.data_ptr(), work.data_ptr(), wb - wb_cut, None)
    msg = last_error()
    torch.cuda.synchronize()
    return rc, msg, bool((d_keys.cpu().numpy() == 0x1EEF).all() and (d_det.cpu().numpy() == DET_SENTINEL).all())


def test_refusals_name_their_cause_and_write_nothing(L, dev):
    scored = lambda clen: _scores_for(clen, np.full(len(clen), 640, np.int64))
    good = [(110, 120, 1), (120, 150, 2), (180, 400, 63)]
    rc, msg, clean = _refused(L, dev, good, scored)
    assert rc == 0 and not clean, msg                                    # the control: these rows are painted
    rc, msg, clean = _refused(L, dev, [(110, 130, 1), (125, 150, 2), (180, 190, 3)], scored)
    assert rc == EINVAL and clean and "row 1 [125, 150)" in msg and "starts below the end of the row in front of it" in msg
    rc, msg, clean = _refused(L, dev, [(150, 160, 1), (110, 120, 1)], scored)
    assert rc == EINVAL and clean and "row 1 [110, 120)" in msg and "ascend and do not overlap" in msg
    rc, msg, clean = _refused(L, dev, [(110, 120, 1), (130, 140, 64)], scored)
    assert rc == EINVAL and clean and "label 64" in msg and "1 <= label <= 63" in msg
    rc, msg, clean = _refused(L, dev, [(110, 120, 1), (130, 125, 2)], scored)
    assert rc == EINVAL and clean and "0 <= start <= end" in msg

    def one_unscored(clen):
        sc = scored(clen)
        sc[1] = (0, 0, 0, 0, 0)
        return sc
    rc, msg, clean = _refused(L, dev, good, one_unscored)
    assert rc == EINVAL and clean and "row 1 [120, 150)" in msg and "no score" in msg
    rc, msg, clean = _refused(L, dev, [(0, 50, 1), (110, 120, 1), (500, 600, 2)], scored)
    assert rc == 0 and not clean, msg                                    # rows outside the record are unscored, and ignored
    for which in ("paint", "detect"):
        rc, msg, clean = _refused(L, dev, good, scored, wb_cut=1, which=which)
        assert rc == ENOMEM and clean and "workspace too small" in msg, (which, msg)
    rc, msg, clean = _refused(L, dev, [(110, 120, 1), (130, 140, 64)], scored, which="detect")
    assert rc == EINVAL and clean and "label 64" in msg and "1 <= label <= 63" in msg
