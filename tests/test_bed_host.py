"""predict --bed_dir without a GPU: the host formatter dgrp_format_bed_rows against bed.reference_lines (Python integers), the
numpy statement bed.reference_scores against a hand-computed array, and every refusal of the command line before the model is read
or torch.cuda is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from deepgrp_amd import bed
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE

ENOMEM, EINVAL = -3, -1
ONE = 1 << 24


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


def test_symbols_exported_and_bound(L):
    from deepgrp_amd import _lib
    for name in ("dgrp_row_scores_workspace_bytes", "dgrp_row_scores_batch", "dgrp_format_bed_bound", "dgrp_format_bed_rows"):
        assert name in _lib.exported_symbols()
        assert getattr(L, name).argtypes is not None
    assert ROW_SCORE_DTYPE.itemsize == 32
    assert [ROW_SCORE_DTYPE.fields[k][1] for k in ("sum", "bases", "agree", "qmin", "pad")] == [0, 8, 16, 24, 28]
    assert L.dgrp_row_scores_workspace_bytes(3, 100) > 0 and L.dgrp_row_scores_workspace_bytes(-1, 0) == 0


def _segs(rows):
    a = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def _scores(rows):
    a = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for i, (s, b, g, m) in enumerate(rows):
        a[i] = (s, b, g, m, 0)
    return a


# (sum, bases, agree, qmin): the ends, the half-way points of score (bases 125: sum = 2^20 (2m + 1) is exactly (2m + 1) / 2000) and of
# mean (bases 625: sum = 2^19 (2m + 1) is exactly (2m + 1) / 20000), one below each, and the 128-bit path
HAND = [
    (0, 1, 0, 0),
    (ONE, 1, 1, ONE),
    (0, 1000, 0, 0),
    (1000 << 24, 1000, 1000, ONE),
    ((1 << 20) * 1, 125, 0, 0), ((1 << 20) * 1 - 1, 125, 0, 0),                      # 0.0005: score 1 / 0
    ((1 << 20) * 1199, 125, 60, 12345), ((1 << 20) * 1199 - 1, 125, 60, 12345),      # 0.5995: score 600 / 599
    ((1 << 20) * 1999, 125, 125, ONE - 1), ((1 << 20) * 1999 - 1, 125, 124, ONE - 1),  # 0.9995: score 1000 / 999
    ((1 << 19) * 1, 625, 1, 839), ((1 << 19) * 1 - 1, 625, 1, 838),                  # 0.00005: mean 0.0001 / 0.0000; qmin at its half
    ((1 << 19) * 12345, 625, 312, 1), ((1 << 19) * 12345 - 1, 625, 313, ONE // 2),   # 0.61725: mean 0.6173 / 0.6172
    (((1 << 32) - 1) << 24, (1 << 32) - 1, (1 << 32) - 1, ONE),                      # 2 k sum passes 64 bits
    ((((1 << 32) - 1) << 24) // 3, (1 << 32) - 1, (1 << 31), 5592405),
    (7, 3, 1, 2), (3 * ONE - 1, 3, 2, ONE - 1),
]


def _hand():
    rng = np.random.default_rng(3)
    rows = _segs([(int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40)), 1 + i % 63, i % 3) for i in range(len(HAND))])
    return rows, _scores(HAND)


def test_the_half_way_points_round_up():
    """The hand-made rows do sit where they are meant to: the statement in Python integers on the cases named above."""
    rows, scores = _hand()
    lines = bed.reference_lines([b"a", b"b", b"c"], False, rows, scores).split(b"\n")[:-1]
    cols = [ln.split(b"\t") for ln in lines]
    assert [int(c[4]) for c in cols[:10]] == [0, 1000, 0, 1000, 1, 0, 600, 599, 1000, 999]
    assert [c[6] for c in cols[10:14]] == [b"0.0001", b"0.0000", b"0.6173", b"0.6172"]
    assert [c[7] for c in cols[10:12]] == [b"0.0001", b"0.0000"]                    # 839 / 2^24 = 0.00005001, 838 / 2^24 = 0.00004995
    assert cols[14][4:] == [b"1000", b".", b"1.0000", b"1.0000", b"1.0000"]
    assert cols[15][4:] == [b"333", b".", b"0.3333", b"0.3333", b"0.5000"]
    assert all(c[5] == b"." and len(c) == 9 for c in cols)
    assert cols[0][:4] == [b"a", b"%d" % rows[0]["start"], b"%d" % rows[0]["end"], b"class1"]


@pytest.mark.parametrize("by_contig", [False, True])
@pytest.mark.parametrize("min_score", [0, 1, 600, 1000])
def test_formatter_against_python_integers(L, by_contig, min_score):
    rows, scores = _hand()
    names = ["chr1", b"a\xffb", ""]
    want = bed.reference_lines(names, by_contig, rows, scores, min_score)
    assert bed.format_rows(names, by_contig, rows, scores, min_score) == want
    kept = want.count(b"\n")
    assert {0: len(rows), 1000: 5}.get(min_score, kept) == kept and 0 < kept     # (1000: the four at 1, and 1 - 2^-24 / 3, which rounds to it)
    if by_contig:
        assert {ln.split(b"\t")[0] for ln in want.split(b"\n")[:-1]} <= {b"chr1", b"a\xffb", b""}
    else:
        assert all(ln.startswith(b"chr1\t") for ln in want.split(b"\n")[:-1])


def test_formatter_random_scores(L):
    rng = np.random.default_rng(11)
    n = 2000
    bases = rng.integers(1, 1 << 22, n)
    qmin = rng.integers(0, ONE + 1, n)
    total = np.array([int(b) * int(rng.integers(int(m), ONE + 1)) for b, m in zip(bases, qmin)], np.uint64)
    scores = np.zeros(n, ROW_SCORE_DTYPE)
    scores["sum"], scores["bases"], scores["qmin"] = total, bases, qmin
    scores["agree"] = [int(rng.integers(0, b + 1)) for b in bases]
    rows = np.zeros(n, SEGMENT_DTYPE)
    rows["start"] = rng.integers(0, 1 << 33, n)
    rows["end"] = rows["start"] + bases
    rows["label"] = rng.integers(1, 5, n)
    rows["contig"] = np.sort(rng.integers(0, 7, n))
    names = [f"contig_{i}" * (i + 1) for i in range(7)]
    for low in (0, 500):
        assert bed.format_rows(names, True, rows, scores, low) == bed.reference_lines(names, True, rows, scores, low)


def _call(L, names, rows, scores, cap, by_contig=0, min_score=0):
    raw = [nm.encode() for nm in names]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(x) for x in raw], out=off[1:])
    out = np.full(max(cap, 1), 0x7E, np.uint8)
    written = C.c_int64(-7)
    rc = L.dgrp_format_bed_rows(b"".join(raw), off.ctypes.data, len(raw), by_contig, rows.ctypes.data, scores.ctypes.data, len(rows), min_score,
                                out.ctypes.data, cap, C.byref(written))
    return rc, written.value, out


def test_bound_empty_input_and_refusals(L):
    rows, scores = _hand()
    names = ["x" * 37]
    cap = L.dgrp_format_bed_bound(len(rows), 37)
    assert L.dgrp_format_bed_bound(-1, 3) == 0 and L.dgrp_format_bed_bound(3, -1) == 0 and L.dgrp_format_bed_bound(0, 5) == 1
    # the longest line there can be fits the bound's share of one row
    worst_row = _segs([(-(1 << 63), -(1 << 63), -(1 << 31), 0)])
    worst = _scores([(ONE, 1, 1, ONE)])
    rc, n, _ = _call(L, names, worst_row, worst, L.dgrp_format_bed_bound(1, 37))
    assert rc == 0 and n <= L.dgrp_format_bed_bound(1, 37) - 1
    rc, n, out = _call(L, names, rows, scores, cap)
    assert rc == 0 and out[:n].tobytes() == bed.reference_lines(names, False, rows, scores)
    rc, n, out = _call(L, names, rows, scores, cap - 1)                               # one byte short: refused, nothing written
    assert rc == ENOMEM and b"dgrp_format_bed_bound" in L.dgrp_last_error() and (out == 0x7E).all()
    rc, n, _ = _call(L, names, rows[:0], scores[:0], 1)                               # empty input
    assert rc == 0 and n == 0
    assert bed.format_rows(names, False, rows[:0], scores[:0]) == b"" == bed.reference_lines(names, False, rows[:0], scores[:0])
    for bases in (0, -4):                                                            # a row without a scored base
        bad = scores.copy()
        bad["bases"][5] = bases
        rc, _n, _ = _call(L, names, rows, bad, cap)
        assert rc == EINVAL and b"row 5" in L.dgrp_last_error()
        with pytest.raises(ValueError):
            bed.reference_lines(names, False, rows, bad)
    by = rows.copy()
    by["contig"][3] = 1                                                              # names a record that is not there
    rc, _n, _ = _call(L, names, by, scores, cap, by_contig=1)
    assert rc == EINVAL


def test_reference_scores_on_a_hand_computed_array():
    nan = np.float32("nan")
    probs = np.array([[0.50, 0.25, 0.25],          # coordinate 10: first maximum 0
                      [0.25, 0.50, 0.25],          # 11: 1
                      [0.25, 0.25, 0.50],          # 12: 2
                      [0.40, 0.40, 0.20],          # 13: a tie, the first column wins
                      [nan, 1.00, 0.00],           # 14: a NaN in column 0 is never beaten
                      [0.00, nan, 2.0 ** -25]],    # 15: a NaN later never wins; 2^-25 is half a unit and rounds up to 1
                     np.float32)
    assert list(bed.first_max(probs)) == [0, 1, 2, 0, 0, 2]
    q = lambda v: int(np.floor(float(np.float32(v)) * ONE + 0.5))
    rows = _segs([(10, 16, 1, 0), (11, 13, 2, 0), (0, 12, 1, 0), (14, 99, 2, 0), (16, 20, 1, 0), (12, 12, 2, 0), (13, 15, 1, 0)])
    got = bed.reference_scores(probs, 10, rows)
    want = _scores([(q(0.25) * 2 + q(0.5) + q(0.4) + ONE + 0, 6, 1, 0),             # the NaN counts 0
                    (q(0.25) + q(0.5), 2, 1, q(0.25)),
                    (q(0.25) + q(0.5), 2, 1, q(0.25)),                              # clipped at the front
                    (0 + 1, 2, 1, 0),                                               # clipped at the back
                    (0, 0, 0, 0), (0, 0, 0, 0),                                     # outside the record; start == end
                    (q(0.4) + ONE, 2, 0, q(0.4))])
    np.testing.assert_array_equal(got, want)
    assert q(0.25) == ONE // 4 and q(0.4) == 6710887                                 # float32(0.4) = 13421773 / 2^25: 6710886.5, half up
    specials = np.array([0.0, -0.0, -1.0, nan, np.inf, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 1e-45, 2.0 ** -24, 2.0 ** -25,
                         1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, (12345 + 0.5) / ONE], np.float32)
    assert list(bed.quantise(specials)) == [0, 0, 0, 0, ONE, ONE, ONE, ONE, 0, 1, 1, 2, 3, 12346]


# ---- the command line: every refusal is a SystemExit with its message before the model is read or the GPU is touched ----------------
@pytest.fixture
def no_gpu(monkeypatch):
    import torch

    def touched(*_a, **_k):
        raise AssertionError("torch.cuda was touched before the refusal")
    for name in ("is_available", "set_device", "current_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_cli_refusals(no_gpu, tmp_path, monkeypatch):
    model = str(tmp_path / "no_such_model.h5")                                       # reading it would raise, not exit
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    out = str(tmp_path / "beds")
    _refused(["predict", model, str(fa), "--bed_min_score", "5"], "--bed_min_score needs --bed_dir")
    _refused(["--bed_min_score", "5", model, str(fa)], "--bed_min_score needs --bed_dir")           # the README form
    for s in ("-1", "1001"):
        _refused(["predict", model, str(fa), "--bed_dir", out, "--bed_min_score", s], "--bed_min_score must lie in 0..1000")
    _refused(["predict", model, str(fa), "--bed_dir", out, "--split_contigs"], "--bed_dir runs in one process")
    (tmp_path / "sub").mkdir()
    twin = tmp_path / "sub" / "a.fa"
    twin.write_text(">r\nACGT\n")
    _refused(["predict", model, str(fa), str(twin), "--bed_dir", out], "would collide")
    _refused(["predict", model, str(fa), str(fa), "--bed_dir", out], "given twice")
    _refused(["--bed_dir", out, "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--bed_dir belongs to predict")
    _refused(["--bed_min_score", "3", "evaluate", model, str(tmp_path / "ann.bed"), str(fa)], "--bed_dir belongs to predict")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(["predict", model, str(fa), "--bed_dir", out], "--bed_dir runs in one process")
    assert not os.path.exists(out)                                                   # and no refusal left a directory behind


def test_plan_names_and_bed_files(tmp_path):
    import argparse
    d = str(tmp_path / "out")
    args = argparse.Namespace(bed_dir=d, FASTA=["-", str(tmp_path / "x.fa.gz"), str(tmp_path / "y.gz.npz")], bed_min_score=7)
    p = bed.plan(args)
    assert p.min_score == 7 and [os.path.basename(p.paths[f]) for f in args.FASTA] == ["stdin.bed", "x.fa.gz.bed", "y.gz.npz.bed"]
    assert bed.plan(argparse.Namespace(FASTA=["a"])) is None
    rows, scores = _hand()
    files = bed.BedFiles(p, "-")
    files.write(["n"], False, rows, scores)
    assert len(os.listdir(d)) == 1 and not os.path.exists(p.paths["-"])
    files.commit()
    assert os.listdir(d) == ["stdin.bed"]
    assert open(p.paths["-"], "rb").read() == bed.reference_lines(["n"], False, rows, scores, 7)
    files = bed.BedFiles(p, args.FASTA[1])
    files.write(["n"], False, rows, scores)
    files.abort()
    assert os.listdir(d) == ["stdin.bed"]
