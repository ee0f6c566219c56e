"""`Accumulator.add` and `Accumulator.probe` driven directly with the four reports of `evaluate` attached, on one hand-made work
item where the reports' code paths branch: a record with annotation rows and predicted rows (one of each clipped entirely outside the
record, one of each straddling its end), one with predicted rows only, one with annotation rows only, one with neither; then an item
of records without a base, then an empty one.  Every expected count comes from the numpy statements the report modules hold
(reference_hist, reference_detect, reference_keys, reference_strata_hist, reference_crosstab, reference_row_classes,
reference_bounds, reference_bound_hist) and from plain numpy for the core; every comparison is integer equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, THETA, W = 5, 0.5, 8
NAMES = ["chrA", "chrB", "chrC", "chrD"]
ORIGINS, LENGTHS = [100, 7, 0, 40], [700, 300, 500, 200]              # 1700 bases
ROW0 = [2, 705, 1005, 1511]                                              # the records' rows of the probabilities, gaps between them
FAMILIES = ["DNA/hAT", "LINE/L1", "Simple_repeat"]
TRUE = {"chrA": [(150, 300, 1), (280, 400, 2), (790, 900, 3), (900, 1000, 1), (0, 50, 2), (600, 640, 4), (420, 430, 1)],
        "chrC": [(0, 500, 2), (100, 120, 1), (490, 600, 3)]}
MILLIDIV = {"chrA": [30, 120, -1, 250, 50, 310, 99], "chrC": [10, 55, 300]}
# predict's rows ascend and do not overlap; (600, 619, 4) covers 19 of the 40 bases of (600, 640, 4): one short of theta
PRED = {"chrA": [(0, 60, 2), (160, 290, 1), (300, 380, 2), (500, 520, 3), (600, 619, 4), (625, 640, 1), (780, 850, 3), (2000, 2100, 4)],
        "chrB": [(10, 50, 1), (50, 120, 2), (300, 400, 4)]}
WANT = {"chrA": [0, 1000, 499, 500, 0, 700, 1, 0], "chrB": [250, 1000, 37]}
OFF = {"chrA": ([(100, 200, 0), (350, 700, 0), (500, 510, 0)], [66, 64, 65]), "chrB": ([(0, 30, 0), (40, 200, 0)], [65, 64])}


def _rows(spans):
    from deepgrp_amd.pipeline import SEGMENT_DTYPE
    a = np.zeros(len(spans), SEGMENT_DTYPE)
    for i, (s, e, l) in enumerate(spans):
        a[i] = (s, e, l, 0)
    return a


def _clip(rows, o, n):
    a = np.clip(rows["start"].astype(np.int64), o, o + n) - o
    e = np.clip(rows["end"].astype(np.int64), o, o + n) - o
    return a, np.maximum(e, a)


def _track(rows, o, n):
    """The label track `evaluate` scores: the smallest label among the rows that cover a base, 0 where none does."""
    t = np.zeros(n, np.int8)
    for (a, e), l in zip(zip(*_clip(rows, o, n)), rows["label"]):
        t[a:e] = np.where(t[a:e] == 0, l, np.minimum(t[a:e], l))
    return t


def _scores_for(clen, want):
    """ROW_SCORE_DTYPE entries whose BED score is `want`; rows without a base inside their record stay all zero, unscored."""
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE
    sc = np.zeros(len(clen), ROW_SCORE_DTYPE)
    for i, (b, w) in enumerate(zip(clen, want)):
        if b > 0:
            sc[i] = ((int(w) * (int(b) << 24) + 999) // 1000, b, b // 2, 5, 0)
    return sc


def _row_counts(rows, other, o, n):
    """(clipped length, hits against the other track, inside, found) of the rows of one record."""
    a, e = _clip(rows, o, n)
    hits = np.array([int((other[x:y] == l).sum()) for x, y, l in zip(a, e, rows["label"])], np.int64).reshape(len(rows))
    clen = e - a
    ok = clen > 0
    return clen, hits, ok, ok & (hits.astype(np.float64) >= THETA * clen)


def _state(acc):
    out = {k: np.array(getattr(acc, k)).copy() for k in ("cnf", "elements", "found", "segments", "supported")}
    for r in acc.reports:
        for k, v in vars(r).items():
            if isinstance(v, np.ndarray):
                out[r.key + "." + k] = v.copy()
    return out


@pytest.fixture(scope="module")
def run():
    """The three calls, made once; what every test below reads."""
    from deepgrp_amd import annotation, boundaries, curves, offtarget, strata
    from deepgrp_amd.evaluation import Accumulator
    from deepgrp_amd.pipeline import require_gpu
    dev = require_gpu()
    ann = annotation.Rows({k: _rows(v) for k, v in TRUE.items()})
    ann.millidiv = {k: np.array(v, np.int32) for k, v in MILLIDIV.items()}
    ann.offtarget_rows = {k: _rows(v[0]) for k, v in OFF.items()}
    ann.offtarget_keys = {k: np.array(v[1], np.uint32) for k, v in OFF.items()}
    ann.families = list(FAMILIES)
    reports = [curves.Curves(C, 32, elements=True), strata.Strata(C, (50, 100, 200), (20, 100), 16),
               offtarget.Offtarget(C, FAMILIES), boundaries.Boundaries(C, W)]
    joined = boundaries.Boundaries(C, W, join=120)
    for r in reports + [joined]:
        r.bind(ann, C)
    acc, acc_joined = Accumulator(C, THETA, reports), Accumulator(C, THETA, [joined])
    empty = _rows([])
    true = [ann.get(nm, empty) for nm in NAMES]
    pred = [_rows(PRED.get(nm, [])) for nm in NAMES]
    scores = np.concatenate([_scores_for(np.subtract(*_clip(p, o, n)[::-1]), WANT.get(nm, [])) for nm, p, o, n in zip(NAMES, pred, ORIGINS, LENGTHS)])
    rng = np.random.default_rng(11)
    probs = rng.random((ROW0[-1] + LENGTHS[-1] + 4, C), dtype=np.float32)
    probs /= probs.sum(axis=1, keepdims=True)
    probs[ROW0[0] + 100] = (0.0, 1.0, 0.0, 0.0, 0.0)                      # exactly 0 and exactly 1, on an annotated base of class 1
    assert probs.min() == 0.0 and probs.max() == 1.0 and probs.dtype == np.float32
    keys = [("header " + nm, nm, o, n) for nm, o, n in zip(NAMES, ORIGINS, LENGTHS)]
    probe = acc.probe(ann)
    probed = probe(torch.from_numpy(probs).to(dev), ROW0, LENGTHS, ORIGINS, keys)
    acc.add(ORIGINS, LENGTHS, pred, true, scores, probed, NAMES)
    acc_joined.add(ORIGINS, LENGTHS, pred, true, scores, None, NAMES)
    torch.cuda.synchronize()
    out = dict(acc=acc, reports=dict((r.key, r) for r in reports), joined=joined, probed=probed, ann=ann, true=true, pred=pred, scores=scores,
               probs=probs, after_one=_state(acc), counts_one=(acc.records, acc.bases, acc.records_annotated, acc.rows_used, acc.outside))
    # records without a base, as the runner hands them on: no probabilities, every row outside
    names0 = ["chrA", "chrD", "chrC"]
    probed0 = probe(None, [0, 0, 0], [0, 0, 0], [5, 6, 7], [("h", nm, 0, 0) for nm in names0])
    acc.add([5, 6, 7], [0, 0, 0], [empty] * 3, [ann.get(nm, empty) for nm in names0], np.zeros(0, scores.dtype), probed0, names0)
    out.update(probed0=probed0, after_two=_state(acc), counts_two=(acc.records, acc.bases, acc.records_annotated, acc.rows_used, acc.outside))
    probed_none = probe(None, [], [], [], [])
    acc.add([], [], [], [], None, probed_none, [])
    out.update(probed_none=probed_none, after_three=_state(acc),
               counts_three=(acc.records, acc.bases, acc.records_annotated, acc.rows_used, acc.outside))
    # the numpy side, shared by the tests
    out["t_tracks"] = [_track(t, o, n) for t, o, n in zip(true, ORIGINS, LENGTHS)]
    out["p_tracks"] = [_track(p, o, n) for p, o, n in zip(pred, ORIGINS, LENGTHS)]
    out["t_counts"] = [_row_counts(t, pt, o, n) for t, pt, o, n in zip(true, out["p_tracks"], ORIGINS, LENGTHS)]
    out["p_counts"] = [_row_counts(p, tt, o, n) for p, tt, o, n in zip(pred, out["t_tracks"], ORIGINS, LENGTHS)]
    out["item_probs"] = np.concatenate([probs[r0:r0 + n] for r0, n in zip(ROW0, LENGTHS)])
    return out


def _flat(per_record, k):
    return np.concatenate([x[k] for x in per_record])


def test_the_core_counts(run):
    acc = run["acc"]
    cnf = np.zeros((C, C), np.int64)
    np.add.at(cnf, (np.concatenate(run["t_tracks"]).astype(np.int64), np.concatenate(run["p_tracks"]).astype(np.int64)), 1)
    assert cnf.sum() == sum(LENGTHS) and (run["after_one"]["cnf"] == cnf).all()
    for rows, counts, total, good in ((run["true"], run["t_counts"], "elements", "found"), (run["pred"], run["p_counts"], "segments", "supported")):
        lab = np.concatenate([r["label"] for r in rows]).astype(np.int64)
        ok, hit = _flat(counts, 2), _flat(counts, 3)
        assert (run["after_one"][total] == np.bincount(lab[ok], minlength=C)).all()
        assert (run["after_one"][good] == np.bincount(lab[hit], minlength=C)).all()
    assert run["after_one"]["found"].sum() > 0 and run["after_one"]["supported"].sum() > 0
    assert (_flat(run["p_counts"], 1)[4], _flat(run["p_counts"], 0)[4]) == (19, 19) and _flat(run["t_counts"], 1)[5] == 19  # one short of theta:
    assert not _flat(run["t_counts"], 3)[5] and _flat(run["p_counts"], 3)[4]                    # the element is not found, the row is supported
    assert run["counts_one"] == (4, 1700, 2, 10, 2)                      # two annotation rows of chrA lie outside it
    assert acc.probe(run["ann"]) is not None


def test_records_without_a_base_and_an_empty_item_reach_no_report(run):
    from deepgrp_amd.evaluation import Accumulator, report
    assert run["probed0"] == {"curves": None, "strata": None} and run["probed_none"] == {"curves": None, "strata": None}
    assert run["counts_two"] == (7, 1700, 4, 20, 12) and run["counts_three"] == run["counts_two"]
    for later in ("after_two", "after_three"):
        assert run[later].keys() == run["after_one"].keys()
        for k, v in run["after_one"].items():
            assert (run[later][k] == v).all(), k
    assert list(report(run["acc"], {}))[-4:] == ["curves", "strata", "offtarget", "boundaries"]
    assert Accumulator(C, THETA).probe(run["ann"]) is None
    assert Accumulator(C, THETA, [run["reports"]["offtarget"], run["reports"]["boundaries"]]).probe(run["ann"]) is None


def test_curves(run):
    from deepgrp_amd import curves
    cv = run["reports"]["curves"]
    assert set(run["probed"]) == {"curves", "strata"}
    hist, flag = curves.reference_hist(run["item_probs"], np.concatenate(run["t_tracks"]), cv.bins)
    assert flag == 0 and run["probed"]["curves"][1] == 0 and (run["probed"]["curves"][0] == hist).all() and (cv.hist == hist).all()
    assert hist.sum() == C * sum(LENGTHS) and hist[1, 1, cv.bins - 1] >= 1 and hist[0, 0, 0] >= 1     # the exact 1 and an exact 0
    lab = np.concatenate([p["label"] for p in run["pred"]]).astype(np.int64)
    want = np.concatenate([np.array(WANT.get(nm, []), np.int64) for nm in NAMES])
    seg, sup = curves.row_counts(lab, want, _flat(run["p_counts"], 2), _flat(run["p_counts"], 3), C)
    assert (cv.seg == seg).all() and (cv.sup == sup).all() and seg.sum() == 9 and 0 < sup.sum() < 9
    need = [np.where(c[0] > 0, np.ceil(THETA * c[0].astype(np.float64)), 0).astype(np.int64) for c in run["t_counts"]]
    _keys, d = curves.reference_detect(ORIGINS, LENGTHS, run["pred"], [WANT.get(nm, []) for nm in NAMES], run["true"], need)
    det = np.zeros((C, curves.SCORES + 1), np.int64)
    t_lab, ok = np.concatenate([t["label"] for t in run["true"]]).astype(np.int64), _flat(run["t_counts"], 2)
    np.add.at(det, (t_lab[ok], d.astype(np.int64)[ok] + 1), 1)
    assert (cv.det == det).all() and det.sum() == 8 and det[:, 0].sum() >= 1 and det[1, 1001] == 1     # not found at all; found up to 1000


def test_strata(run):
    from deepgrp_amd import strata
    st = run["reports"]["strata"]
    per_record = [strata.strata_of(t, MILLIDIV.get(nm), st.div_edges, st.len_edges) for nm, t in zip(NAMES, run["true"])]
    assert per_record[0].tolist() == [2, 8, 14, 11, 4, 10, 3]            # div_bin * 3 + len_bin, by hand: NA is bin 4, 200+ bin 3
    keys = np.concatenate(strata.reference_keys(ORIGINS, LENGTHS, run["true"], per_record))
    hist, flag = strata.reference_strata_hist(run["item_probs"], keys, st.S, st.bins)
    assert flag == 0 and run["probed"]["strata"][1] == 0 and (run["probed"]["strata"][0] == hist).all() and (st.hist == hist).all()
    assert hist.sum() == int((np.concatenate(run["t_tracks"]) > 0).sum()) and hist[1, 2, st.bins - 1] >= 1
    lab, s = np.concatenate([t["label"] for t in run["true"]]).astype(np.int64), np.concatenate(per_record).astype(np.int64)
    clen, hits, ok, hit = (_flat(run["t_counts"], k) for k in range(4))
    counts = np.zeros((4, C, st.S), np.int64)
    np.add.at(counts[0], (lab[ok], s[ok]), 1)
    np.add.at(counts[1], (lab[hit], s[hit]), 1)
    np.add.at(counts[2], (lab[ok], s[ok]), clen[ok])
    np.add.at(counts[3], (lab[ok], s[ok]), hits[ok])
    assert (st.counts == counts).all() and counts[0].sum() == 8 and counts[1].sum() > 0


def test_offtarget(run):
    from deepgrp_amd import offtarget
    ot = run["reports"]["offtarget"]
    empty = _rows([])
    rows = [np.concatenate([t, run["ann"].offtarget_rows.get(nm, empty)]) for nm, t in zip(NAMES, run["true"])]
    keys = [np.concatenate([t["label"].astype(np.uint32), run["ann"].offtarget_keys.get(nm, np.zeros(0, np.uint32))]) for nm, t in zip(NAMES, run["true"])]
    tracks = offtarget.reference_keys(ORIGINS, LENGTHS, rows, keys)
    flat = np.concatenate(tracks)
    uns = [p[c[2] & ~c[3]] for p, c in zip(run["pred"], run["p_counts"])]
    hist = np.zeros((2, C, ot.K), np.int64)
    hist[0], f0 = offtarget.reference_crosstab(np.concatenate(run["p_tracks"]), flat, C, ot.K)
    hist[1], f1 = offtarget.reference_crosstab(np.concatenate([_track(u, o, n) for u, o, n in zip(uns, ORIGINS, LENGTHS)]), flat, C, ot.K)
    hist[1, 0] = 0
    assert f0 == 0 and f1 == 0 and (ot.hist == hist).all()
    assert hist[0].sum() == sum(LENGTHS) and hist[1].sum() > 0 and hist[0, :, 64:67].sum() > 0 and hist[0, :, -1].sum() > 0
    table = np.zeros((C, 6), np.int64)
    for p, c, track, o, n in zip(run["pred"], run["p_counts"], tracks, ORIGINS, LENGTHS):
        for (a, e), l, ok, good in zip(zip(*_clip(p, o, n)), p["label"], c[2], c[3]):
            table[l, 0] += ok
            table[l, 1] += good
            if ok and not good:
                table[l, 2 + int(np.argmax(offtarget.reference_row_classes(track[a:e], int(l))))] += 1
    assert (ot.rows == table).all() and table[:, 0].sum() == 9 and table[:, 2:].sum() == table[:, 0].sum() - table[:, 1].sum() > 0


@pytest.mark.parametrize("join", [None, 120])
def test_boundaries(run, join):
    from deepgrp_amd import boundaries
    bd = run["reports"]["boundaries"] if join is None else run["joined"]
    units = run["true"] if join is None else [boundaries.join_rows(t, join) for t in run["true"]]
    assert join is None or len(units[0]) == len(run["true"][0]) - 1      # (150, 300, 1) and (420, 430, 1) are 120 apart: one unit
    for view, (rows, tracks) in enumerate(((units, run["p_tracks"]), (run["pred"], run["t_tracks"]))):
        clen = np.concatenate([np.subtract(*_clip(q, o, n)[::-1]) for q, o, n in zip(rows, ORIGINS, LENGTHS)])
        need = np.where(clen > 0, np.ceil(THETA * clen.astype(np.float64)), 0).astype(np.int64)
        bounds = boundaries.reference_bounds(ORIGINS, LENGTHS, tracks, rows, W)
        frag, edge, tally, flag = boundaries.reference_bound_hist(ORIGINS, LENGTHS, rows, bounds, need, C, W)
        assert flag == 0 and (bd.frag[view] == frag).all() and (bd.edge[view] == edge).all() and (bd.tally[view] == tally).all()
        assert frag.sum() == int((clen > 0).sum()) and tally[:, 0].sum() > 0 and edge.sum() > 0
