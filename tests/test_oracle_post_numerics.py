"""The oracle's score transform (orc_scores, deepgrp/prediction.py:51-57) and softmax path (orc_softmax_argmax, :62-65 and the
argmax of deepgrp/__main__.py:83) against live numpy, bit for bit, at every class count the library takes (1 to 64): the GPU
tests compare the kernels with numpy too (test_gpu_post_numerics.py), but every parity test of the pipeline trusts the oracle.

numpy sums a softmax row with pairwise_sum: a left fold below 8 columns, 8 interleaved accumulators from 8 on.  A left fold
there moves most sums by an ulp, and near ties of the maximum then take the wrong label."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from numpy_post import (F32_ONE, f32, mismatch_report, np_scores, np_softmax, score_rows, score_sweep_bits,
                        softmax_cases)

WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))


def _check_softmax(orc, a, what):
    sm, lab = orc.softmax_argmax(a)
    want, want_lab = np_softmax(a)
    bad = (sm.view(np.int32) != want.view(np.int32)).any(axis=1)
    assert not bad.any(), mismatch_report(f"{what}: softmax values", a, sm, want, bad)
    bad = lab != want_lab
    assert not bad.any(), mismatch_report(f"{what}: labels {lab[bad][:6]} numpy {want_lab[bad][:6]}", a, sm, want, bad)


@pytest.mark.parametrize("C", range(1, 65))
def test_softmax_argmax_every_class_count(orc, C):
    """orc.softmax_argmax against numpy's formula: values through an int32 view, labels equal.  Random rows (more than numpy's
    8192-element buffer), N(0, 4) rows, near ties of the maximum one ulp apart (the larger one later), exact ties (the first
    index wins) and rows whose peak underflows the other exponentials to subnormals and zeros."""
    for name, a in softmax_cases(C, 20000 if C <= 16 else 9000, seed=1).items():
        _check_softmax(orc, a, f"C={C} {name}")


def _scores_chunk(orc, bits, C, phase):
    rows = score_rows(f32(bits), C, phase)
    sc, cl = orc.scores(rows)
    want, want_cl = np_scores(rows)
    bad = (sc.view(np.int64) != want.view(np.int64)) | (cl != want_cl)
    return None if not bad.any() else mismatch_report(f"C={C} scores/classes (classes {cl[bad][:6]} numpy {want_cl[bad][:6]})",
                                                      rows, sc, want, bad)


@pytest.mark.parametrize("C", [1, 2, 8, 64])
def test_scores_sweep(orc, C):
    """orc.scores against apply_mss's score expression: row maxima at every 16th float32 pattern of [0, 1] and at every pattern
    around the 0.99 clamp, the sign change of the log and the maxima 1e-6 swamps (numpy_post.score_sweep_bits), each at a
    column that cycles through the row, alone, tied exactly or one ulp above a neighbour."""
    bits = score_sweep_bits()
    assert bits.min() == 0 and bits.max() == F32_ONE
    step = max(1 << 14, (1 << 22) // C)
    with ThreadPoolExecutor(WORKERS) as pool:
        errs = [e for e in pool.map(lambda s: _scores_chunk(orc, bits[s:s + step], C, s), range(0, bits.size, step)) if e]
    assert not errs, errs[0]


def test_numpy_math_vectorised(orc):
    """orc_np_expf and orc_np_logf through the array entry points, against np.exp / np.log on whole arrays (test_numpy_math in
    test_oracle_golden.py calls them one value at a time).  Rows (x, 0) with x <= -17.5 have the row sum 1 + exp(x) == 1, so
    their first softmax value is exp(x) itself; rows (0, p) score np.log(m / (1 - m)) with m = min(p + 1e-6, 0.99)."""
    lo, hi = int(np.float32(-17.5).view(np.uint32)), int(np.float32(-104.0).view(np.uint32))
    # every 7th pattern, and every pattern from -103.9 down: numpy's exp gives 0 from xmin = -103.97208404541015625 (0xc2cff1b5) on
    x = f32(np.concatenate([np.arange(lo, hi + 1, 7), np.arange(int(np.float32(-103.9).view(np.uint32)), hi + 1)]).astype(np.uint32))
    e = np.exp(x)
    assert (e + np.float32(1) == 1).all()
    a = np.stack([x, np.zeros_like(x)], axis=1)
    sm, lab = orc.softmax_argmax(a)
    bad = sm[:, 0].view(np.int32) != e.view(np.int32)
    assert not bad.any(), mismatch_report("exp", x, sm[:, 0], e, bad)
    assert (lab == 1).all()

    p = f32(np.arange(0, F32_ONE + 1, 61, dtype=np.uint32))
    m = np.minimum(p + np.float32(1e-6), np.float32(0.99))
    q = m / (np.float32(1) - m)
    sc, cl = orc.scores(np.stack([np.zeros_like(p), p], axis=1))
    want = np.log(q).astype(np.float64)
    bad = (sc.view(np.int64) != want.view(np.int64)) & (p > 0)
    assert not bad.any(), mismatch_report("log", q, sc, want, bad)
    assert (cl == (p > 0)).all()
