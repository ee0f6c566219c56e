"""`evaluate --curves` on the CPU: the new entry's symbols and host refusals, the curve maths against brute-force statements, the row
curves on hand-made rows, the command line's refusals before anything is loaded, and the two files byte for byte."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_H5 = os.path.join(GOLDEN, "model_u60_T342_att.h5")       # 5 classes
EINVAL = -1
P = 0x10000                    # a non-NULL, 16-byte aligned pointer value that is never dereferenced: an earlier check fails


# ------------------------------------------------------------------------- the entry, without a GPU
def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_prob_hist_workspace_bytes", "dgrp_prob_hist_batch"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().dgrp_abi_version() == 1                  # an addition: the version stays


def test_workspace_query_is_monotone_and_0_outside_the_envelope():
    from deepgrp_amd._lib import lib
    L = lib()
    q = L.dgrp_prob_hist_workspace_bytes
    for Cn, bins in ((1, 2), (5, 1000), (64, 4096)):
        sizes = [q(n, Cn, bins) for n in (0, 1, 3, 40, 4096, 10 ** 6)]
        assert sizes == sorted(sizes) and sizes[0] > 0, sizes
    for n in (0, 40):
        by_c = [q(n, c, 1000) for c in (1, 2, 5, 16, 17, 64)]
        by_b = [q(n, 5, b) for b in (2, 10, 1000, 4096)]
        assert by_c == sorted(by_c) and by_b == sorted(by_b) and by_c[0] > 0 and by_b[0] > 0
    for bad in ((-1, 5, 1000), (1, 0, 1000), (1, 65, 1000), (1, 5, 1), (1, 5, 4097), (2 ** 62, 5, 1000)):
        assert q(*bad) == 0, bad


def _tab(*v):
    return (C.c_int64 * len(v))(*v)


_D = object()


def _args(probs=P, Cn=5, nrec=1, row0=_D, n=_D, truth=P, off=_D, bins=1000, hist=P, bad=P, work=P, work_bytes=1 << 40):
    """A call that would be accepted, but for the arguments given (one record of 10 bases; None: a NULL table)."""
    row0 = _tab(0) if row0 is _D else row0
    n = _tab(10) if n is _D else n
    off = _tab(0) if off is _D else off
    return (probs, Cn, nrec, row0, n, truth, off, bins, hist, bad, work, work_bytes, None)


REFUSALS = [
    (dict(Cn=0), "1 <= classes <= 64"), (dict(Cn=65), "1 <= classes <= 64"),
    (dict(bins=1), "2 <= bins <= 4096"), (dict(bins=4097), "2 <= bins <= 4096"),
    (dict(nrec=-1), "bad arguments"), (dict(hist=None), "bad arguments"), (dict(bad=None), "bad arguments"),
    (dict(row0=None), "bad arguments"), (dict(n=None), "bad arguments"), (dict(off=None), "bad arguments"),
    (dict(hist=P + 4), "8-byte aligned"),
    (dict(n=_tab(-1)), "negative offset, length or origin (record 0)"), (dict(row0=_tab(-64)), "negative offset, length or origin (record 0)"),
    (dict(off=_tab(-1)), "negative offset, length or origin (record 0)"),
    (dict(nrec=2, row0=_tab(0, 64), n=_tab(10, -3), off=_tab(0, 10)), "(record 1)"),
    (dict(n=_tab(1 << 40)), "too long"),
    (dict(probs=None), "NULL pointer"), (dict(truth=None), "NULL pointer"), (dict(work=None), "NULL pointer"),
    (dict(probs=P + 2), "4-byte aligned"),
    (dict(work_bytes=0), "workspace too small"), (dict(work_bytes=-1), "workspace too small"),
]


@pytest.mark.parametrize("change,fragment", REFUSALS, ids=[f"{i}-{'-'.join(c)}" for i, (c, _f) in enumerate(REFUSALS)])
def test_bad_arguments_are_refused_before_any_device_work(change, fragment):
    from deepgrp_amd._lib import lib
    L = lib()
    a = _args(**change)
    assert L.dgrp_prob_hist_batch(*a) == EINVAL
    msg = L.dgrp_last_error().decode()
    assert msg.startswith("dgrp_prob_hist_batch: ") and fragment in msg, msg


def test_the_workspace_bound_is_the_query():
    from deepgrp_amd._lib import lib
    L = lib()
    need = L.dgrp_prob_hist_workspace_bytes(1, 5, 1000)
    assert L.dgrp_prob_hist_batch(*_args(work_bytes=need - 1)) == EINVAL
    assert "workspace too small" in L.dgrp_last_error().decode()


# ------------------------------------------------------------------------- curve maths
def _random_case(n, Cn, seed, drop_pos=None, drop_neg=None):
    rng = np.random.default_rng(seed)
    p = rng.random((n, Cn), dtype=np.float32)
    p[rng.random((n, Cn)) < 0.2] = 0                             # ties and an occupied bottom bin
    p[rng.random((n, Cn)) < 0.1] = 1
    t = rng.integers(0, Cn, n).astype(np.int8)
    if drop_pos is not None and n:
        t[t == drop_pos] = (drop_pos + 1) % Cn                   # a class without a positive base
    if drop_neg is not None:
        t[:] = drop_neg                                          # a class without a negative base
    return p, t


CASES = [(5000, 5, 1000, {}), (5000, 2, 2, {}), (3001, 2, 10, {}), (777, 5, 10, {}), (1, 5, 1000, {}), (0, 5, 10, {}), (0, 2, 2, {}),
         (2000, 5, 10, dict(drop_pos=3)), (2000, 2, 1000, dict(drop_neg=1)), (500, 5, 2, dict(drop_neg=0))]


@pytest.mark.parametrize("n,Cn,bins,kw", CASES, ids=[f"n{c[0]}-C{c[1]}-b{c[2]}-{'-'.join(c[3]) or 'plain'}" for c in CASES])
def test_curves_equal_brute_force_counts(n, Cn, bins, kw):
    from deepgrp_amd import curves
    p, t = _random_case(n, Cn, 17 * n + Cn + bins, **kw)
    hist, flag = curves.reference_hist(p, t, bins)
    assert flag == 0 and hist.shape == (Cn, 2, bins) and (hist.sum(axis=(1, 2)) == n).all()
    pbin = np.minimum((p * np.float32(bins)).astype(np.int64), bins - 1)
    cv = curves.base_curves(hist)
    summ = curves.summaries(hist)
    for c in range(Cn):
        pos = t == c
        tp = [int(((pbin[:, c] >= k) & pos).sum()) for k in range(bins)]
        fp = [int(((pbin[:, c] >= k) & ~pos).sum()) for k in range(bins)]
        fn = [int(((pbin[:, c] < k) & pos).sum()) for k in range(bins)]
        tn = [int(((pbin[:, c] < k) & ~pos).sum()) for k in range(bins)]
        for name, want in (("TP", tp), ("FP", fp), ("FN", fn), ("TN", tn)):
            assert cv[name][c].tolist() == want, name
        div = lambda a, b: a / b if b else float("nan")
        tpr = [div(tp[k], tp[k] + fn[k]) for k in range(bins)] + [0.0]
        fpr = [div(fp[k], fp[k] + tn[k]) for k in range(bins)] + [0.0]
        ppv = [div(tp[k], tp[k] + fp[k]) for k in range(bins)]
        f1 = [div(2 * tp[k], 2 * tp[k] + fp[k] + fn[k]) for k in range(bins)]
        for name, want in (("TPR", tpr[:-1]), ("FPR", fpr[:-1]), ("PPV", ppv), ("F1", f1)):
            np.testing.assert_array_equal(cv[name][c], np.array(want, np.float64), err_msg=name)      # (NaN equals NaN here)
        # the summaries by a plain loop over the same integers
        npos, nneg = int(pos.sum()), int(n - pos.sum())
        if npos and nneg:
            area = sum((fpr[k] - fpr[k + 1]) * (tpr[k] + tpr[k + 1]) / 2 for k in range(bins))
            assert abs(summ["auroc"][c] - area) <= 1e-12
        else:
            assert math.isnan(summ["auroc"][c])
        if npos:
            ap = sum((tpr[k] - tpr[k + 1]) * ppv[k] for k in range(bins) if tp[k] + fp[k])
            assert abs(summ["average_precision"][c] - ap) <= 1e-12
        else:
            assert math.isnan(summ["average_precision"][c])
        known = [x for x in f1 if not math.isnan(x)]                 # (no positive base: F1 is 0 wherever a base is called)
        if known:
            assert summ["best_f1"][c] == max(known) and summ["best_threshold"][c] == f1.index(max(known)) / bins    # the lowest k on a tie
        else:
            assert math.isnan(summ["best_f1"][c]) and math.isnan(summ["best_threshold"][c])
    # every NaN path prints
    text = curves.bases_tsv(hist)
    assert text.count("\n") == 1 + Cn * bins
    if kw or n == 0:
        assert "\tnan" in text


def test_a_perfect_and_a_useless_class():
    from deepgrp_amd import curves
    hist = np.zeros((2, 2, 10), np.int64)
    hist[0, 1, 9], hist[0, 0, 0] = 50, 70                        # class 0: positives at the top, negatives at the bottom
    hist[1, 1, 4], hist[1, 0, 4] = 70, 50                        # class 1: all in one bin
    s = curves.summaries(hist)
    assert s["auroc"] == [1.0, 0.5] and s["average_precision"][0] == 1.0 and s["average_precision"][1] == 70 / 120
    assert s["best_f1"][0] == 1.0 and s["best_threshold"][0] == 0.1     # k = 1 .. 9 all reach F1 = 1: the lowest
    assert s["best_threshold"][1] == 0.0


def test_reference_hist_flags_and_leaves_out():
    from deepgrp_amd import curves
    p = np.full((6, 3), 0.5, np.float32)
    t = np.array([0, 1, 2, 0, 1, 2], np.int8)
    clean, flag = curves.reference_hist(p, t, 4)
    assert flag == 0 and clean.sum() == 18 and (clean[:, :, 2].sum(axis=1) == 6).all()
    for (i, c, v) in ((1, 1, np.nan), (2, 0, 1.0000001), (3, 2, -1e-9)):
        q = p.copy()
        q[i, c] = v
        h, flag = curves.reference_hist(q, t, 4)
        assert flag == 1 and h.sum() == 17 and h[c].sum() == 5
    for v in (3, -1):
        u = t.copy()
        u[4] = v
        h, flag = curves.reference_hist(p, u, 4)
        assert flag == 1 and h.sum() == 15 and (h.sum(axis=(1, 2)) == 5).all()
    q = p.copy()
    q[0, 0] = -0.0
    h, flag = curves.reference_hist(q, t, 4)
    assert flag == 0 and h[0, 1, 0] == 1


def test_bin_edges_of_exact_quotients():
    """Where j / bins is a float32, it opens bin j and its lower neighbour closes bin j - 1; 1.0 falls in the last bin."""
    from deepgrp_amd.curves import bin_index
    for bins in (2, 64, 4096):
        j = np.arange(1, bins, dtype=np.float32)
        edge = j / np.float32(bins)
        assert bin_index(edge, bins).tolist() == list(range(1, bins))
        assert bin_index(np.nextafter(edge, np.float32(0)), bins).tolist() == list(range(0, bins - 1))
        assert bin_index(np.float32(1), bins) == bins - 1 and bin_index(np.float32(-0.0), bins) == 0
        assert bin_index(np.float32(1e-45), bins) == 0


# ------------------------------------------------------------------------- row curves
def _scores(rows):
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE
    a = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for i, (s, b) in enumerate(rows):
        a[i]["sum"], a[i]["bases"] = s, b
    return a


def test_row_scores_are_the_bed_integers():
    from deepgrp_amd import bed, curves
    one = 1 << 24
    sc = _scores([(10 * one, 10), (one // 2, 1), (0, 7), (3 * one - 1, 3), (4995 * (one // 10000) * 2, 2), (12345678, 1)])
    got = curves.row_scores_of(sc)
    assert got.tolist() == [bed._half_up(int(s), int(b) << 24, 1000) for s, b in zip(sc["sum"], sc["bases"])]
    assert got[0] == 1000 and got[1] == 500 and got[2] == 0 and got[3] == 1000


def test_row_curves_on_hand_made_rows():
    """Three rows of class 1 at score 500 (a tie at m = 500), one at 501, one of class 2 at 0; one row with an empty clipped span, which
    counts nowhere; theta exactly at the boundary: hits == theta * length is supported, one hit less is not."""
    from deepgrp_amd import curves
    from deepgrp_amd.evaluation import count
    labels = np.array([1, 1, 1, 1, 2, 1], np.int64)
    clen = np.array([10, 10, 8, 4, 6, 0], np.int64)
    hits = np.array([5, 4, 4, 4, 2, 0], np.int64)                # 5 >= 5 yes; 4 >= 5 no; 4 >= 4 yes; 4 >= 2 yes; 2 >= 3 no
    score = np.array([500, 500, 500, 501, 0, 999], np.int64)
    total, good = np.zeros(3, np.int64), np.zeros(3, np.int64)
    kept, sup = count(0.5, labels, clen, hits, total, good)
    assert kept.tolist() == [True, True, True, True, True, False] and sup.tolist() == [True, False, True, True, False, False]
    assert total.tolist() == [0, 4, 1] and good.tolist() == [0, 3, 0]
    seg, su = curves.row_counts(labels, score, kept, sup, 3)
    seg_at, sup_at = curves.row_curves(seg, su)
    assert seg_at.shape == (3, 1001)
    assert seg_at[1, 0] == total[1] and sup_at[1, 0] == good[1] and seg_at[2, 0] == total[2] and sup_at[2, 0] == good[2]
    assert seg_at[1, 500] == 4 and seg_at[1, 501] == 1 and seg_at[1, 502] == 0 and sup_at[1, 500] == 3 and sup_at[1, 501] == 1
    assert seg_at[2, 0] == 1 and seg_at[2, 1] == 0 and seg_at[1, 999] == 0 and seg_at[0].sum() == 0
    lines = curves.rows_tsv(seg, su).splitlines()
    assert lines[0] == "#class\tmin_score\tsegments\tsupported\tprecision" and len(lines) == 1 + 2 * 1001
    assert lines[1 + 500] == "1\t500\t4\t3\t0.75" and lines[1 + 501] == "1\t501\t1\t1\t1.0" and lines[1 + 502] == "1\t502\t0\t0\tnan"
    assert lines[1 + 1001] == "2\t0\t1\t0\t0.0" and lines[1 + 1002] == "2\t1\t0\t0\tnan"


# ------------------------------------------------------------------------- files
def test_bases_file_byte_for_byte():
    from deepgrp_amd import curves
    hist = np.zeros((1, 2, 3), np.int64)
    hist[0, 1] = [1, 0, 3]
    hist[0, 0] = [4, 2, 0]
    assert curves.bases_tsv(hist) == ("#class\tthreshold\tTP\tFP\tFN\tTN\tTPR\tFPR\tPPV\tF1\n"
                                      "0\t0.0\t4\t6\t0\t0\t1.0\t1.0\t0.4\t0.5714285714285714\n"
                                      "0\t0.3333333333333333\t3\t2\t1\t4\t0.75\t0.3333333333333333\t0.6\t0.6666666666666666\n"
                                      "0\t0.6666666666666666\t3\t0\t1\t6\t0.75\t0.0\t1.0\t0.8571428571428571\n")
    for k in range(1000):
        assert float(repr(k / 1000)) == k / 1000 and len(repr(k / 1000)) <= 5      # thresholds print exactly and short


def test_write_stages_both_files_and_a_failure_leaves_nothing(tmp_path, monkeypatch):
    import logging

    from deepgrp_amd import curves
    c = curves.Curves(2, 4)
    c.hist[1, 1, 3] = 5
    c.hist[1, 0, 0] = 7
    c.seg[1, 800], c.sup[1, 800] = 2, 1
    plan = curves.CurvePlan(str(tmp_path / "run"), 4, str(tmp_path / "run.bases.tsv"), str(tmp_path / "run.rows.tsv"))
    c.write(plan, logging.getLogger("test"))
    assert sorted(os.listdir(tmp_path)) == ["run.bases.tsv", "run.rows.tsv"]
    assert (tmp_path / "run.bases.tsv").read_text() == curves.bases_tsv(c.hist) and (tmp_path / "run.rows.tsv").read_text() == curves.rows_tsv(c.seg, c.sup)
    s = c.summary()
    assert s["bins"] == 4 and s["auroc"] == [None, 1.0] and s["average_precision"][0] is None and s["best_threshold"][1] == 0.25
    before = {f: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path)}
    monkeypatch.setattr(curves, "rows_tsv", lambda *a: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        c.write(plan, logging.getLogger("test"))
    monkeypatch.undo()
    from deepgrp_amd.outfiles import StagedFile
    monkeypatch.setattr(StagedFile, "finish", lambda self: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        c.write(plan, logging.getLogger("test"))
    assert {f: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path)} == before      # no temporary file, the old files untouched


# ------------------------------------------------------------------------- command line
def test_curve_flags_parse():
    from deepgrp_amd.__main__ import CommandLineParser
    a = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curves", "out/run", "--curve_bins", "64"]).args
    assert a.curves == "out/run" and a.curve_bins == 64
    d = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa"]).args
    assert d.curves is None and d.curve_bins is None
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--curves", "x"])          # on evaluate only


CHILD = ("import sys\n"
         "from deepgrp_amd.__main__ import main\n"
         "try:\n"
         "    main(sys.argv[1:])\n"
         "except SystemExit as e:\n"
         "    import deepgrp_amd._lib as l\n"
         "    print('LOADED' if (l._lib is not None or 'torch' in sys.modules or 'h5py' in sys.modules) else 'CLEAN')\n"
         "    raise\n")


def _child(tmp_path, *flags, env=None):
    ann = tmp_path / "a.bed"
    ann.write_text("chr1\t0\t10\t1\n")
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    return subprocess.run([sys.executable, "-c", CHILD, "evaluate", MODEL_H5, str(ann), str(tmp_path / "x.fa"), *flags], env=e,
                          capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


@pytest.mark.parametrize("flags,words", [
    (["--curve_bins", "100"], ["--curve_bins needs --curves"]),
    (["--curves", "run", "--curve_bins", "1"], ["--curve_bins must lie in 2..4096, not 1"]),
    (["--curves", "run", "--curve_bins", "4097"], ["--curve_bins must lie in 2..4096, not 4097"]),
    (["--curves", "missing_dir/run"], ["--curves", "missing_dir", "does not exist"]),
    (["--curves", "sub/"], ["--curves", "prefix"]),
])
def test_refusals_come_before_the_model_is_read(tmp_path, flags, words):
    (tmp_path / "sub").mkdir()
    r = _child(tmp_path, *flags)
    assert r.returncode == 1, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert r.stdout.strip() == "CLEAN"
    assert sorted(os.listdir(tmp_path)) == ["a.bed", "sub"]


def test_file_names_come_from_the_prefix(tmp_path):
    from deepgrp_amd import curves
    from deepgrp_amd.__main__ import CommandLineParser
    (tmp_path / "out").mkdir()
    prefix = str(tmp_path / "out" / "hg38.v2")
    a = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curves", prefix]).args
    p = curves.plan(a)
    assert p == curves.CurvePlan(prefix, 1000, prefix + ".bases.tsv", prefix + ".rows.tsv")
    a = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa", "--curves", prefix, "--curve_bins", "4096"]).args
    assert curves.plan(a).bins == 4096
    assert curves.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa"]).args) is None
    fa = tmp_path / "out" / "hg38.v2.rows.tsv"
    fa.write_text(">x\nACGT\n")
    with pytest.raises(SystemExit) as e:
        curves.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", str(fa), "--curves", prefix]).args)
    assert "overwrite" in str(e.value)
