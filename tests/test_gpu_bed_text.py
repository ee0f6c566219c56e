"""dgrp_bed_text_batch (the BED lines written on the device, predict --bed_gzip) against bed.reference_lines (Python integers) AND
against the host formatter dgrp_format_bed_rows, byte for byte, on synthetic rows and scores: the ends of the sums, the half-way
points of all four quotients and one unit below each, the extremes of every column, --bed_min_score, 0 / 1 / 5 000 rows, a capacity
one byte short, the refusals, a short workspace and a side stream -- every call between sentinel pages in front of and behind the
text and the workspace."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import EINVAL, ENOMEM, ONE, random_scores, scores_of, segs, text_call  # noqa: E402
from deepgrp_amd import bed  # noqa: E402

BIG = (1 << 40) - 1
NAMES = [b"x", b"N" * 300, b"chr\xff1 "]

# (sum, bases, agree, qmin).  R(num, den, k) = floor((2 k num + den) / (2 den)); a half-way point is a quotient k num / den = m + 1/2:
#   score  k = 1000:  bases 2000, sum = (2 s + 1) 2^24  ->  s + 1/2          mean  k = 10000: bases 20000, sum = (2 m + 1) 2^24  ->  m + 1/2
#   agree  k = 10000: bases 20000, agree = 2 m + 1      ->  m + 1/2          min   k = 10000: qmin = 2^19 (2 j + 1) / 625 with 625 | 2 j + 1
SCORES = [
    (ONE, 1, 1, ONE), (0, 1, 0, 0), (777, 1, 0, 777),                                           # bases = 1
    (5000 << 24, 5000, 5000, ONE), (0, 5000, 0, 0),                                             # the largest and the smallest sum
    (BIG << 24, BIG, BIG, ONE), ((BIG << 24) // 7 * 3 + 12345, BIG, BIG // 3, 99),              # bases = 2^40 - 1
    ((2 * 0 + 1) << 24, 2000, 0, 0), (((2 * 0 + 1) << 24) - 1, 2000, 0, 0),                     # score 0.5 -> 1, below -> 0
    ((2 * 599 + 1) << 24, 2000, 7, 5), (((2 * 599 + 1) << 24) - 1, 2000, 7, 5),                 # 599.5 -> 600 / 599
    ((2 * 999 + 1) << 24, 2000, 2000, ONE - 1), (((2 * 999 + 1) << 24) - 1, 2000, 1999, ONE - 1),     # 999.5 -> 1000 / 999
    ((2 * 0 + 1) << 24, 20000, 1, 0), (((2 * 0 + 1) << 24) - 1, 20000, 0, 0),                   # mean 0.5 -> 0.0001 / 0.0000; agree the same
    ((2 * 6172 + 1) << 24, 20000, 2 * 6172 + 1, 1 << 19), (((2 * 6172 + 1) << 24) - 1, 20000, 2 * 6172, (1 << 19) - 1),   # 6172.5; min 312.5
    ((2 * 9999 + 1) << 24, 20000, 19999, (1 << 19) * 3), (((2 * 9999 + 1) << 24) - 1, 20000, 19998, (1 << 19) * 3 - 1),   # 9999.5; min 937.5
    (12345678, 3, 2, ONE), (3 * ONE - 1, 3, 3, 0),
]
# (start, end, label): 1, 2, 9, 10 and 19 digits; labels 1, 9, 10, 63
SPANS = [(0, 7, 1), (5, 42, 9), (10, 99, 10), (99, 100, 63), (123456789, 999999999, 1), (999999999, 1000000000, 9),
         (1000000000, 9999999999, 10), (1 << 62, (1 << 63) - 1, 63), (10 ** 18, 10 ** 18 + 1, 1)]


def _corpus():
    rows = segs([SPANS[i % len(SPANS)] + (i % 3,) for i in range(len(SCORES))])
    return rows, scores_of(SCORES)


def _check(names, by_contig, rows, scores, min_score):
    want = bed.reference_lines(names, by_contig, rows, scores, min_score)
    assert bed.format_rows(names, by_contig, rows, scores, min_score) == want
    rc, n, text, work = text_call(names, by_contig, rows, scores, min_score)
    assert rc == 0 and n == len(want)
    assert text.body(n).cpu().numpy().tobytes() == want
    assert text.guards_intact() and work.guards_intact()
    assert bool((text.body()[n:] == 0xA5).all())                                      # and nothing behind the text
    return want


def test_the_corpus_sits_where_it_is_meant_to():
    rows, scores = _corpus()
    cols = [ln.split(b"\t") for ln in bed.reference_lines(NAMES, False, rows, scores).split(b"\n")[:-1]]
    assert [int(c[4]) for c in cols[:13]] == [1000, 0, 0, 1000, 0, 1000, 429, 1, 0, 600, 599, 1000, 999]
    assert [c[6] for c in cols[13:19]] == [b"0.0001", b"0.0000", b"0.6173", b"0.6172", b"1.0000", b"0.9999"]
    assert [c[7] for c in cols[15:19]] == [b"0.0313", b"0.0312", b"0.0938", b"0.0937"]
    assert [c[8] for c in cols[13:19]] == [b"0.0001", b"0.0000", b"0.6173", b"0.6172", b"1.0000", b"0.9999"]
    assert cols[5][4:] == [b"1000", b".", b"1.0000", b"1.0000", b"1.0000"] and cols[1][4:] == [b"0", b".", b"0.0000", b"0.0000", b"0.0000"]
    assert sorted({len(c[1]) for c in cols} | {len(c[2]) for c in cols}) == [1, 2, 3, 9, 10, 19]
    assert {c[3] for c in cols} == {b"class1", b"class9", b"class10", b"class63"}


@pytest.mark.parametrize("by_contig", [False, True])
@pytest.mark.parametrize("min_score", [0, 1, 600, 1000])
def test_extremes_and_half_way_points(by_contig, min_score):
    rows, scores = _corpus()
    want = _check(NAMES, by_contig, rows, scores, min_score)
    kept = want.count(b"\n")
    assert 0 < kept and (kept == len(rows)) == (min_score == 0)
    if by_contig:
        assert {ln.split(b"\t")[0] for ln in want.split(b"\n")[:-1]} <= set(NAMES)


def test_sizes():
    rng = np.random.default_rng(17)
    rc, n, text, work = text_call(NAMES, True, segs([]), scores_of([]), 0)            # no rows: no device work
    assert rc == 0 and n == 0 and text.untouched() and work.untouched()
    rows, scores = _corpus()
    for i in (0, 6, 15):                                                              # one row
        assert _check(NAMES, True, rows[i:i + 1], scores[i:i + 1], 0).count(b"\n") == 1
    n = 5000                                                                          # more than one scan tile of 2 048, 20 workgroups
    big = np.zeros(n, rows.dtype)
    big["start"] = np.sort(rng.integers(0, 1 << 33, n))
    big["end"] = big["start"] + rng.integers(1, 1 << 20, n)
    big["label"] = rng.integers(1, 64, n)
    big["contig"] = np.sort(rng.integers(0, 3, n))
    sc = random_scores(n, rng, filtered=0.2)
    for low in (0, 500):
        want = _check(NAMES, True, big, sc, low)
        assert (want.count(b"\n") == n) == (low == 0) and want.count(b"\n") > n // 2


def test_every_row_filtered_gives_no_byte():
    rows, scores = _corpus()
    scores = scores.copy()
    scores["sum"] = 0
    rc, n, text, work = text_call(NAMES, True, rows, scores, 1)
    assert rc == 0 and n == 0 and text.untouched() and work.guards_intact()
    assert bed.reference_lines(NAMES, True, rows, scores, 1) == b""


def test_capacity_one_byte_short():
    rows, scores = _corpus()
    want = bed.reference_lines(NAMES, True, rows, scores, 0)
    rc, n, text, work = text_call(NAMES, True, rows, scores, 0, cap=len(want) - 1)
    assert rc == 0 and n == len(want) and text.untouched() and work.guards_intact()   # the length, and nothing written
    rc, n, text, work = text_call(NAMES, True, rows, scores, 0, cap=len(want))        # the exact capacity is enough
    assert rc == 0 and text.body().cpu().numpy().tobytes() == want and text.guards_intact()


def test_refusals_leave_the_text_untouched():
    from deepgrp_amd._lib import lib
    rows, scores = _corpus()
    for bases in (0, -3):
        bad = scores.copy()
        bad["bases"][len(bad) - 2] = bases
        rc, _n, text, work = text_call(NAMES, True, rows, bad, 0)
        assert rc == EINVAL and b"no scored base" in lib().dgrp_last_error() and text.untouched() and work.guards_intact()
    for contig in (3, -1):
        bad = rows.copy()
        bad["contig"][4] = contig
        rc, _n, text, work = text_call(NAMES, True, bad, scores, 0)
        assert rc == EINVAL and b"outside the names" in lib().dgrp_last_error() and text.untouched() and work.guards_intact()
        assert text_call(NAMES, False, bad, scores, 0)[0] == 0                        # without by_contig the column is not read
    bad = scores.copy()
    bad["sum"][3] += 1                                                                # a mean above 1: outside the 64-bit envelope
    rc, _n, text, work = text_call(NAMES, True, rows, bad, 0)
    assert rc == EINVAL and b"envelope" in lib().dgrp_last_error() and text.untouched()
    rc, _n, text, work = text_call(NAMES, True, rows, scores, 0, short_work=1)
    assert rc == ENOMEM and b"workspace" in lib().dgrp_last_error() and text.untouched() and work.untouched()


def test_a_side_stream_gives_the_same_bytes():
    rows, scores = _corpus()
    want = bed.reference_lines(NAMES, True, rows, scores, 600)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc, n, text, work = text_call(NAMES, True, rows, scores, 600)
        got = text.body(n).cpu().numpy().tobytes()
    assert rc == 0 and got == want and text.guards_intact() and work.guards_intact()


def test_pipeline_method_matches_the_host_formatter():
    """ContigPipeline.bed_text_batch: its capacity guess is below the bound, so long lines take the retry."""
    from deepgrp_amd.pipeline import ContigPipeline
    rows, scores = _corpus()
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
    for names in (NAMES, [b"n"]):
        for low in (0, 600):
            got = ContigPipeline.bed_text_batch(names, len(names) > 1, d_rows, d_scores, low).cpu().numpy().tobytes()
            assert got == bed.format_rows(names, len(names) > 1, rows, scores, low)
