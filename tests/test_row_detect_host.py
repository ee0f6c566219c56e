"""`evaluate --curves --curve_elements` on the CPU: the numpy statement of the detection score on hand-worked cases, the element
curves, their file and summary on a small histogram, the flag's refusals and the plan, the staged write with and without the third
file, and need = ceil(theta * clen) against the comparison `evaluation.count` makes."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_H5 = os.path.join(GOLDEN, "model_u60_T342_att.h5")
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


def _rows(*rows):
    a = np.zeros(len(rows), SEG)
    for i, (s, e, lab) in enumerate(rows):
        a[i] = (s, e, lab, 0)
    return a


def _detect(origin, length, pred, scores, true, theta):
    """One record through reference_detect with need = need_of(theta, clipped length): -> (key track, detection scores)."""
    from deepgrp_amd import curves
    from deepgrp_amd.evaluation import clipped_lengths
    t = _rows(*true)
    need = curves.need_of(theta, clipped_lengths(t, origin, length))
    keys, d = curves.reference_detect([origin], [length], [_rows(*pred)], [np.array(scores, np.int64)], [t], [need])
    return keys[0], d


# ------------------------------------------------------------------------- the statement
def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_row_detect_workspace_bytes", "dgrp_paint_row_keys_batch", "dgrp_row_detect_batch"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    q = _lib.lib().dgrp_row_detect_workspace_bytes
    sizes = [q(3, n) for n in (0, 1, 100, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and q(-1, 5) == 0 and q(1, -5) == 0
    # behind the tables of the other row entries: a counter, an interval and a threshold per row (20 bytes)
    assert all(q(3, n) >= _lib.lib().dgrp_eval_workspace_bytes(3, n) + 20 * n for n in (1, 100, 10 ** 6))


def test_half_covered_by_300_and_half_by_800():
    pred, scores = [(100, 150, 2), (150, 200, 2)], [300, 800]
    key, d = _detect(100, 100, pred, scores, [(100, 200, 2)], 0.5)
    assert d.tolist() == [800]                                         # the 50 bases of the 800 row are half of it
    assert key[:50].tolist() == [2 << 10 | 300] * 50 and key[50:].tolist() == [2 << 10 | 800] * 50
    _key, d = _detect(100, 100, pred, scores, [(100, 200, 2)], 1.0)
    assert d.tolist() == [300]                                         # all of it needs both rows
    _key, d = _detect(100, 100, pred, scores, [(100, 200, 2)], 0.51)
    assert d.tolist() == [300]                                         # 51 bases: one more than the 800 row has


def test_wrong_class_uncovered_and_score_bounds():
    _key, d = _detect(0, 100, [(0, 100, 3)], [900], [(0, 100, 2), (0, 100, 3), (0, 100, 4)], 0.5)
    assert d.tolist() == [-1, 900, -1]                                 # neither the class below nor the one above counts
    _key, d = _detect(0, 100, [(0, 40, 1), (60, 100, 1)], [0, 1000], [(0, 40, 1), (60, 100, 1), (40, 60, 1), (0, 100, 1)], 1.0)
    assert d.tolist() == [0, 1000, -1, -1]
    key, d = _detect(0, 10, [], [], [(0, 10, 1)], 1e-9)
    assert d.tolist() == [-1] and not key.any()
    _key, d = _detect(0, 100, [(10, 11, 63)], [1000], [(0, 100, 63)], 1e-9)
    assert d.tolist() == [1000]                                        # one base is enough at the smallest theta


def test_clipped_element_and_clipped_rows():
    # the record is [1000, 1100); the element [950, 1050) has 50 bases inside, the row [900, 1020) paints 20 of them
    pred, scores = [(900, 1020, 1), (1020, 1030, 1)], [700, 200]
    key, d = _detect(1000, 100, pred, scores, [(950, 1050, 1)], 0.5)
    assert d.tolist() == [200]                                         # 25 of 50 needed: 20 at 700, 30 at 200
    assert key[:20].tolist() == [1 << 10 | 700] * 20 and key[20:30].tolist() == [1 << 10 | 200] * 10 and not key[30:].any()
    _key, d = _detect(1000, 100, pred, scores, [(950, 1050, 1)], 0.4)
    assert d.tolist() == [700]                                         # 20 of 50


def test_an_element_outside_its_record_is_minus_one_and_not_counted():
    from deepgrp_amd import curves
    true = [(0, 50, 1), (100, 100, 1), (300, 400, 1), (120, 130, 1)]
    _key, d = _detect(100, 100, [(100, 200, 1)], [640], true, 0.5)
    assert d.tolist() == [-1, -1, -1, 640]
    # what Curves._detect counts: only the rows with a base inside their record
    from deepgrp_amd.evaluation import clipped_lengths
    ok = clipped_lengths(_rows(*true), 100, 100) > 0
    c = curves.Curves(2, 4, elements=True)
    np.add.at(c.det, (np.ones(4, np.int64)[ok], d.astype(np.int64)[ok] + 1), 1)
    assert c.det.sum() == 1 and c.det[1, 641] == 1
    # need <= 0 is -1 whatever the track holds
    t = _rows((100, 200, 1))
    _k, d = curves.reference_detect([100], [100], [_rows((100, 200, 1))], [np.array([640])], [t], [np.array([0])])
    assert d.tolist() == [-1]


def test_two_records_keep_their_own_tracks():
    from deepgrp_amd import curves
    pred = [_rows((10, 20, 1)), _rows((10, 20, 2))]
    true = [_rows((10, 20, 1), (10, 20, 2)), _rows((10, 20, 1), (10, 20, 2))]
    keys, d = curves.reference_detect([10, 0], [10, 30], pred, [np.array([5]), np.array([6])], true, [np.array([10, 10])] * 2)
    assert d.tolist() == [5, -1, -1, 6] and d.dtype == np.int32
    assert [k.dtype for k in keys] == [np.uint16] * 2 and [len(k) for k in keys] == [10, 30]


# ------------------------------------------------------------------------- need
@pytest.mark.parametrize("theta", [1e-9, 0.3, 1 / 3, 0.5, 1.0])
def test_need_is_counts_comparison(theta):
    """For every clipped length 1..2000 and every integer hit count 0..clen: hits >= need is exactly the float64 comparison of
    evaluation.count."""
    from deepgrp_amd import curves
    clen = np.arange(1, 2001, dtype=np.int64)
    need = curves.need_of(theta, clen)
    assert need.dtype == np.int64 and (need >= 1).all() and (need <= clen).all()
    hits = np.arange(0, 2001, dtype=np.int64)[None, :]
    count_rule = hits.astype(np.float64) >= theta * clen.astype(np.float64)[:, None]
    np.testing.assert_array_equal(hits >= need[:, None], count_rule)
    assert curves.need_of(theta, np.array([0, 5, 0])).tolist()[::2] == [0, 0]


# ------------------------------------------------------------------------- curves, file, summary
def _small():
    """Two repeat classes.  Class 1: 4 elements with detection scores -1, 300, 800, 800 and rows of scores 300 (supported),
    500 (not), 800 (supported).  Class 2: no element, one row.  -> (det, seg, sup)"""
    det = np.zeros((3, 1002), np.int64)
    seg = np.zeros((3, 1001), np.int64)
    sup = np.zeros((3, 1001), np.int64)
    for d in (-1, 300, 800, 800):
        det[1, d + 1] += 1
    seg[1, [300, 500, 800]] = 1
    sup[1, [300, 800]] = 1
    seg[2, 100] = 1
    return det, seg, sup


def test_element_curves_on_a_small_histogram():
    from deepgrp_amd import curves
    det, seg, sup = _small()
    cv = curves.element_curves(det, seg, sup)
    assert cv["elements"].tolist() == [0, 4, 0]
    f = cv["found"][1]
    assert f[0] == 3 and f[300] == 3 and f[301] == 2 and f[800] == 2 and f[801] == 0 and f.shape == (1001,)
    assert (np.diff(f) <= 0).all()
    assert cv["recall"][1, 0] == 0.75 and cv["recall"][1, 801] == 0.0 and np.isnan(cv["recall"][2]).all() and np.isnan(cv["recall"][0]).all()
    assert cv["precision"][1, 0] == 2 / 3 and cv["precision"][1, 301] == 0.5 and cv["precision"][1, 501] == 1.0 and np.isnan(cv["precision"][1, 801])
    p, r = 2 / 3, 0.75
    assert cv["F1"][1, 0] == 2 * p * r / (p + r)
    assert cv["F1"][1, 501] == 2 * 1.0 * 0.5 / 1.5
    assert np.isnan(cv["F1"][1, 801])                                  # no row left: precision has no denominator
    assert np.isnan(cv["F1"][2]).all()                                 # no element: recall has none
    # precision 0 and recall 0 together: P + R = 0 is a denominator too
    det2, seg2, sup2 = np.zeros((2, 1002), np.int64), np.zeros((2, 1001), np.int64), np.zeros((2, 1001), np.int64)
    det2[1, 0], seg2[1, 10] = 1, 1
    cv2 = curves.element_curves(det2, seg2, sup2)
    assert cv2["recall"][1, 0] == 0.0 and cv2["precision"][1, 0] == 0.0 and np.isnan(cv2["F1"][1, 0])


def test_elements_file_byte_for_byte():
    from deepgrp_amd import curves
    det, seg, sup = _small()
    text = curves.elements_tsv(det, seg, sup)
    lines = text.splitlines()
    assert text.endswith("\n") and len(lines) == 1 + 2 * 1001
    assert lines[0] == "#class\tmin_score\telements\tfound\trecall\tsegments\tsupported\tprecision\tF1"
    p, r = 2 / 3, 0.75
    assert lines[1] == "\t".join(["1", "0", "4", "3", "0.75", "3", "2", repr(p), repr(2 * p * r / (p + r))])
    assert lines[1 + 501] == "\t".join(["1", "501", "4", "2", "0.5", "1", "1", "1.0", repr(2 * 0.5 / 1.5)])
    assert lines[1 + 1000] == "1\t1000\t4\t0\t0.0\t0\t0\tnan\tnan"
    assert lines[1 + 1001] == "2\t0\t0\t0\tnan\t1\t0\t0.0\tnan"
    rows = curves.rows_tsv(seg, sup).splitlines()
    for a, b in zip(lines[1:], rows[1:]):                              # segments, supported and precision are rows.tsv's
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:2] == fb[:2] and fa[5:8] == fb[2:5]


def test_summary_takes_the_lowest_score_on_a_tie():
    from deepgrp_amd import curves
    det, seg, sup = _small()
    s = curves.element_summary(det, seg, sup)
    # F1 at m = 0..300: P = 2/3, R = 3/4 -> 0.7058...; at 301..500: P = 1/2, R = 1/2 -> 0.5; at 501..800: P = 1, R = 1/2 -> 2/3
    assert s["recall_at_0"][1] == 0.75 and s["best_min_score"][1] == 0 and s["best_f1"][1] == 2 * (2 / 3) * 0.75 / (2 / 3 + 0.75)
    assert all(np.isnan(s[k][c]) for k in s for c in (0, 2))
    # a later plateau that is the maximum: its first score is named
    det[1] = 0
    det[1, 801] = 4                                                    # every element found up to 800
    s = curves.element_summary(det, seg, sup)
    assert s["best_min_score"][1] == 501 and s["best_f1"][1] == 1.0    # 501..800: the one row left is supported, recall 1
    c = curves.Curves(3, 4, elements=True)
    c.det, c.seg, c.sup = det, seg, sup
    js = c.summary()
    assert sorted(js) == ["auroc", "average_precision", "best_f1", "best_threshold", "bins", "elements"]
    assert js["elements"] == dict(recall_at_0=[None, 1.0, None], best_f1=[None, 1.0, None], best_min_score=[None, 501, None])
    assert "elements" not in curves.Curves(3, 4).summary()
    assert c.elements_tsv() == curves.elements_tsv(det, seg, sup) and c.element_curves()["found"][1, 800] == 4


# ------------------------------------------------------------------------- the write
def test_write_stages_two_files_without_and_three_with(tmp_path, monkeypatch):
    from deepgrp_amd import curves
    from deepgrp_amd.outfiles import StagedFile
    log = logging.getLogger("test")
    made = []
    init = StagedFile.__init__
    monkeypatch.setattr(StagedFile, "__init__", lambda self, final, mode="wb": (made.append(os.path.basename(final)), init(self, final, mode))[1])
    two = tmp_path / "two"
    two.mkdir()
    plan2 = curves.CurvePlan(str(two / "run"), 4, str(two / "run.bases.tsv"), str(two / "run.rows.tsv"))
    assert plan2.elements_path is None
    c = curves.Curves(3, 4, elements=False)
    c.write(plan2, log)
    assert made == ["run.bases.tsv", "run.rows.tsv"] and sorted(os.listdir(two)) == ["run.bases.tsv", "run.rows.tsv"]
    three = tmp_path / "three"
    three.mkdir()
    plan3 = curves.CurvePlan(str(three / "run"), 4, str(three / "run.bases.tsv"), str(three / "run.rows.tsv"), str(three / "run.elements.tsv"))
    c = curves.Curves(3, 4, elements=True)
    c.det, c.seg, c.sup = _small()
    del made[:]
    c.write(plan3, log)
    assert made == ["run.bases.tsv", "run.rows.tsv", "run.elements.tsv"]
    assert sorted(os.listdir(three)) == ["run.bases.tsv", "run.elements.tsv", "run.rows.tsv"]
    assert (three / "run.elements.tsv").read_text() == curves.elements_tsv(c.det, c.seg, c.sup)
    assert (three / "run.rows.tsv").read_text() == curves.rows_tsv(c.seg, c.sup)
    before = {f: (three / f).read_bytes() for f in os.listdir(three)}
    c.det[1, 5] += 1
    monkeypatch.setattr(curves, "elements_tsv", lambda *a: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        c.write(plan3, log)
    monkeypatch.setattr(curves, "elements_tsv", lambda *a: "x\n")
    monkeypatch.setattr(StagedFile, "finish", lambda self: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        c.write(plan3, log)
    assert {f: (three / f).read_bytes() for f in os.listdir(three)} == before      # none of the three changed, no temporary file
    with pytest.raises(ValueError):
        c.write(plan2, log)                                            # counted, but the plan has no third name
    assert sorted(os.listdir(two)) == ["run.bases.tsv", "run.rows.tsv"]


# ------------------------------------------------------------------------- command line
def test_flag_parses_and_plan_names_the_third_file(tmp_path):
    from deepgrp_amd import curves
    from deepgrp_amd.__main__ import CommandLineParser
    prefix = str(tmp_path / "run")
    a = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curves", prefix, "--curve_elements"]).args
    assert a.curve_elements is True
    assert curves.plan(a) == curves.CurvePlan(prefix, 1000, prefix + ".bases.tsv", prefix + ".rows.tsv", prefix + ".elements.tsv")
    b = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curves", prefix]).args
    assert b.curve_elements is False
    assert curves.plan(b) == curves.CurvePlan(prefix, 1000, prefix + ".bases.tsv", prefix + ".rows.tsv") and curves.plan(b).elements_path is None
    assert curves.CurvePlan._fields[-1] == "elements_path"
    with pytest.raises(SystemExit) as e:
        curves.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curve_elements"]).args)
    assert "--curve_elements needs --curves" in str(e.value)
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--curve_elements"])       # on evaluate only
    # the third name is an output like the other two: it may not be an input
    fa = tmp_path / "run.elements.tsv"
    fa.write_text(">x\nACGT\n")
    with pytest.raises(SystemExit) as e:
        curves.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", str(fa), "--curves", prefix, "--curve_elements"]).args)
    assert "overwrite" in str(e.value) and "run.elements.tsv" in str(e.value)
    assert curves.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", str(fa), "--curves", prefix]).args) is not None


CHILD = ("import sys\n"
         "from deepgrp_amd.__main__ import main\n"
         "try:\n"
         "    main(sys.argv[1:])\n"
         "except SystemExit as e:\n"
         "    import deepgrp_amd._lib as l\n"
         "    print('LOADED' if (l._lib is not None or 'torch' in sys.modules or 'h5py' in sys.modules) else 'CLEAN')\n"
         "    raise\n")


def test_the_refusal_comes_before_the_model_is_read(tmp_path):
    ann = tmp_path / "a.bed"
    ann.write_text("chr1\t0\t10\t1\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, "evaluate", MODEL_H5, str(ann), str(tmp_path / "x.fa"), "--curve_elements"], env=env,
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert "--curve_elements needs --curves" in r.stderr and r.stdout.strip() == "CLEAN"
    assert sorted(os.listdir(tmp_path)) == ["a.bed"]
