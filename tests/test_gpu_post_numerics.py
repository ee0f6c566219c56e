"""dgrp_scores and dgrp_softmax_labels (post_kernels.hip) against live numpy, bit for bit: the score transform over every float32
row maximum in [0, 1], the softmax over every float32 exponent argument in [-104, 0], and both at every class count 1-64 with
planted ties.  The kernels restate numpy's float32 log and exp (np_logf, np_expf), its pairwise row sum and its first-maximum
argmax; a restatement that is off by one rounding anywhere fails here, not as a rare differing TSV row.

The host reference runs in a pool of threads (numpy releases the GIL); chunks of 2^25 rows keep the device side under 1.2 GB."""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from numpy_post import (F32_ONE, f32, mismatch_report, np_scores, np_softmax, np_t_scores, score_rows, softmax_cases)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHUNK = 1 << 25
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))
WORK_BYTES = 4096                                  # dgrp_softmax_labels' block-maximum workspace


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


def _sp():
    return torch.cuda.current_stream().cuda_stream


def _check(rc):
    from deepgrp_amd._lib import check
    check(rc)


def _scores(L, d_p, n):
    """dgrp_scores on the first n rows of the device array d_p: host scores float64, classes int64."""
    c = d_p.shape[1]
    d_s = torch.empty(n, dtype=torch.float64, device=d_p.device)
    d_c = torch.empty(n, dtype=torch.int8, device=d_p.device)
    _check(L.dgrp_scores(d_p.data_ptr(), n, c, d_s.data_ptr(), d_c.data_ptr(), _sp()))
    return d_s.cpu().numpy(), d_c.cpu().numpy().astype(np.int64)


def _softmax(L, d_a, n, values=True):
    """dgrp_softmax_labels on the first n rows of d_a: host softmax float32 [n, C] (None without `values`), labels int64."""
    c = d_a.shape[1]
    d_sm = torch.empty((n, c), dtype=torch.float32, device=d_a.device) if values else None
    d_l = torch.empty(n, dtype=torch.int8, device=d_a.device)
    work = torch.empty(WORK_BYTES, dtype=torch.uint8, device=d_a.device)
    _check(L.dgrp_softmax_labels(d_a.data_ptr(), n, c, d_sm.data_ptr() if values else None, d_l.data_ptr(), work.data_ptr(),
                                 WORK_BYTES, _sp()))
    return (d_sm.cpu().numpy() if values else None), d_l.cpu().numpy().astype(np.int64)


def _run_chunks(chunks, device_step, host_check):
    """device_step(lo, n) -> results, in order on this thread; host_check(lo, n, results) -> error text or None, in the pool
    (at most WORKERS chunks of results held at once).  Returns the first error."""
    errs, pending = [], deque()
    with ThreadPoolExecutor(WORKERS) as pool:
        for lo, n in chunks:
            if len(pending) >= WORKERS:
                errs.append(pending.popleft().result())
            pending.append(pool.submit(host_check, lo, n, device_step(lo, n)))
        errs += [f.result() for f in pending]
    errs = [e for e in errs if e]
    return errs[0] if errs else None


def _chunks(lo, hi):
    """[lo, hi] (inclusive) in chunks of CHUNK."""
    return [(a, min(CHUNK, hi + 1 - a)) for a in range(lo, hi + 1, CHUNK)]


def test_scores_every_float32_maximum(L, dev):
    """Every float32 pattern from +0.0 to 1.0 as a row maximum, in rows (p, 0) -- class 0 wins, the -10 t branch -- and (0, p)
    -- class 1 wins for p > 0; p = 0 is a tie, which class 0 takes.  Scores through an int64 view, classes equal.  The
    reference is prediction.py:51-57 on the row maxima, with the classes of these two layouts (argmax is held to numpy on
    real rows at every class count below)."""
    d_p = [torch.zeros((CHUNK, 2), dtype=torch.float32, device=dev) for _ in range(2)]

    def device_step(lo, n):
        p = torch.arange(lo, lo + n, dtype=torch.int32, device=dev).view(torch.float32)
        out = []
        for col in (0, 1):
            d_p[col][:n, col] = p
            out.append(_scores(L, d_p[col], n))
        return out

    def host_check(lo, n, got):
        p = f32(np.arange(lo, lo + n, dtype=np.uint32))
        t = np_t_scores(p)
        for col, (sc, cl) in zip((0, 1), got):
            cls = (p > 0).astype(np.int64) if col == 1 else np.zeros(n, np.int64)
            want = np.where(cls > 0, t, -10 * t).astype(float)
            bad = (sc.view(np.int64) != want.view(np.int64)) | (cl != cls)
            if bad.any():
                return mismatch_report(f"layout {'(0, p)' if col else '(p, 0)'}: scores/classes (classes {cl[bad][:6]})",
                                       p, sc, want, bad)
        return None

    err = _run_chunks(_chunks(0, F32_ONE), device_step, host_check)
    assert err is None, err


def test_softmax_every_exp_argument(L, dev):
    """Rows (x, 0.0) for every float32 x from -0.0 down to -104, and a sample of the patterns below -104 down to -inf: the global
    maximum is 0, so the kernel's exp argument runs over the whole domain where np.exp(float32) is neither 1-rounded-from-tiny
    nor 0 (below about -17 the softmax value is exp(x) itself).  Values through an int32 view and labels equal numpy's."""
    d_a = torch.zeros((CHUNK, 2), dtype=torch.float32, device=dev)
    neg_zero, neg_104 = 0x80000000, int(np.float32(-104.0).view(np.uint32))

    def device_step(lo, n):
        x = torch.arange(lo - (1 << 32), lo + n - (1 << 32), dtype=torch.int32, device=dev)   # the same 32 bits, signed
        d_a[:n, 0] = x.view(torch.float32)
        return _softmax(L, d_a, n)

    def host_check(lo, n, got):
        sm, lab = got
        a = np.zeros((n, 2), np.float32)
        a[:, 0] = f32(np.arange(lo, lo + n, dtype=np.uint32))
        want, want_lab = np_softmax(a)
        bad = (sm.view(np.int32) != want.view(np.int32)).any(axis=1) | (lab != want_lab)
        return mismatch_report("softmax of (x, 0)", a, sm, want, bad) if bad.any() else None

    err = _run_chunks(_chunks(neg_zero, neg_104), device_step, host_check)
    assert err is None, err

    below = np.arange(neg_104 + 1, 0xFF800000, 4093, dtype=np.uint32)
    a = np.zeros((below.size + 2, 2), np.float32)
    a[:, 0] = f32(np.concatenate([below, [0xFF7FFFFF, 0xFF800000]]))          # ..., -FLT_MAX, -inf
    sm, lab = _softmax(L, torch.from_numpy(a).to(dev), a.shape[0])
    want, want_lab = np_softmax(a)
    bad = (sm.view(np.int32) != want.view(np.int32)).any(axis=1) | (lab != want_lab)
    assert not bad.any(), mismatch_report("softmax of (x, 0), x < -104", a, sm, want, bad)


@pytest.mark.parametrize("C", range(1, 65))
def test_softmax_every_class_count(L, dev, C):
    """dgrp_softmax_labels at C classes against numpy: random probabilities (2^20 rows up to 16 classes, 2^16 beyond), N(0, 4)
    rows, near ties one ulp apart (the larger later), exact ties (the first wins), peaks that underflow the rest of the row.
    Values through an int32 view, labels equal; the labels-only launch (the pipeline's) gives the same labels."""
    for name, a in softmax_cases(C, 1 << 20 if C <= 16 else 1 << 16, seed=2).items():
        d_a = torch.from_numpy(a).to(dev)
        sm, lab = _softmax(L, d_a, a.shape[0])
        want, want_lab = np_softmax(a)
        bad = (sm.view(np.int32) != want.view(np.int32)).any(axis=1)
        assert not bad.any(), mismatch_report(f"C={C} {name}: softmax values", a, sm, want, bad)
        bad = lab != want_lab
        assert not bad.any(), mismatch_report(f"C={C} {name}: labels {lab[bad][:6]} numpy {want_lab[bad][:6]}", a, sm, want, bad)
        _, lab_only = _softmax(L, d_a, a.shape[0], values=False)
        np.testing.assert_array_equal(lab_only, lab)


@pytest.mark.parametrize("C", range(1, 65))
def test_scores_every_class_count(L, dev, C):
    """dgrp_scores at C classes against numpy: row maxima at random float32 patterns of [0, 1] and around the 0.99 clamp, at a
    column that cycles through the row, alone, tied exactly or one ulp above a neighbour (numpy_post.score_rows); and random
    probability rows.  Scores through an int64 view, classes equal."""
    rng = np.random.default_rng(C)
    clamp = int((np.float32(0.99) - np.float32(1e-6)).view(np.uint32))
    bits = np.concatenate([rng.integers(0, F32_ONE + 1, 1 << 16), np.arange(clamp - 300, clamp + 300), [0, 1, F32_ONE]])
    for name, a in (("planted", score_rows(f32(bits.astype(np.uint32)), C, phase=C)),
                    ("random", rng.random((1 << 16, C), dtype=np.float32))):
        sc, cl = _scores(L, torch.from_numpy(a).to(dev), a.shape[0])
        want, want_cl = np_scores(a)
        bad = (sc.view(np.int64) != want.view(np.int64)) | (cl != want_cl)
        assert not bad.any(), mismatch_report(f"C={C} {name}: scores/classes (classes {cl[bad][:6]} numpy {want_cl[bad][:6]})",
                                              a, sc, want, bad)


@pytest.mark.parametrize("C", [5, 8, 16, 17, 64])
def test_prediction_softmax_float32(C):
    """deepgrp_amd.prediction.softmax (the mirror of prediction.py:62-65) on float32 input: numpy's values bit for bit, up to the
    64 columns the kernel takes."""
    from deepgrp_amd import prediction as dgpredict
    rng = np.random.default_rng(100 + C)
    for a in (rng.random((30000, C), dtype=np.float32), softmax_cases(C, 1, seed=3)["near_tie"]):
        got = dgpredict.softmax(a)
        want, _ = np_softmax(a)
        assert got.dtype == np.float32 and got.shape == a.shape
        bad = (got.view(np.int32) != want.view(np.int32)).any(axis=1)
        assert not bad.any(), mismatch_report(f"C={C}: prediction.softmax", a, got, want, bad)
