"""dgrp_rmout_text_batch (the lines of a RepeatMasker listing written on the device, predict --bed_rmout) against
rmout.reference_lines (Python integers and bytes), byte for byte, every call between sentinel pages in front of and behind the text
and the workspace, with poison behind the text: 0 / 1 / 256 / 257 / 5 000 rows (more than one scan tile of 2 048), by_contig on and
off, a batch with a record without a row, min_score 0 / 1 / 600 / 1000 (emitted rows between filtered ones, first and last row
filtered, all rows filtered), IDs that gain a digit (9 -> 10, 99 -> 100) and id0 above 10^9, join gaps -1 / 0 / 5 / 2^40 with runs
that cross the 2 048 edge, *h_ids against rmout.reference_ids, starts and ends at 0, 9, 99 999 999, 2^32 and 2^40, `(0)` left,
record and class names of 1 and 255 bytes, a capacity one byte short, two calls that give the same bytes, every refusal alone, and
a late producer on a side stream (tests/stream_harness.py)."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import EINVAL, ENOMEM, ONE, random_scores, scores_of, segs  # noqa: E402
from rmout_device import tables, text_call  # noqa: E402
from test_gpu_bed_text import SCORES  # noqa: E402
from deepgrp_amd import rmout  # noqa: E402

TOP = 1 << 40
NAMES = [b"x", b"n" * 255, b"scaffold_17|arrow"]
ENDS = [TOP, TOP + 5, (1 << 32) + 1]
PAIRS = [(b"A", b"S"), (b"AluY", b"SINE/Alu"), (b"k" * 255, b"LTR/ERVL-MaLR"), (b"L1", b"f" * 255)]
# (start, end, label): start + 1 gains a digit at 9 and 99 999 999; starts and ends at 0, 9, 99 999 999, 2^32 and 2^40
SPANS = [(0, 9, 1), (9, 42, 4), (99_999_999, 100_000_000, 3), (99_999_999, 1 << 32, 2), (1 << 32, (1 << 32) + 1, 4), (1 << 32, TOP - 1, 1),
         (TOP - 1, TOP, 2)]


def _corpus():
    """The scores of tests/test_gpu_bed_text.py (the ends and half-way points of the score) on SPANS, records ascending."""
    n = len(SCORES)
    rows = segs([SPANS[i % len(SPANS)] + (3 * i // n,) for i in range(n)])
    for i in range(n):                                                                # record 2 ends at 2^32 + 1
        if rows["contig"][i] == 2 and rows["end"][i] > ENDS[2]:
            rows["start"][i], rows["end"][i] = ENDS[2] - 1, ENDS[2]
    return rows, scores_of(SCORES)


def _check(names, by_contig, rows, scores, min_score, rec_end, pairs, join=-1, id0=0):
    want, lines, ids = rmout.reference_lines(names, by_contig, rows, scores, min_score, rec_end, pairs, join, id0)
    rc, n, got_lines, got_ids, text, work = text_call(names, by_contig, rows, scores, min_score, rec_end, pairs, join, id0)
    assert rc == 0 and (n, got_lines, got_ids) == (len(want), lines, ids)
    got = text.body(n).cpu().numpy().tobytes()
    if got != want:
        a, b = got.split(b"\n"), want.split(b"\n")
        k = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
        raise AssertionError((k, a[k][-140:], b[k][-140:]))
    assert text.guards_intact() and work.guards_intact()
    assert bool((text.body()[n:] == 0xA5).all())                                      # and nothing behind the text
    return want, lines, ids


def test_the_example_of_the_format():
    rows = segs([(99, 350, 3, 0), (1000, 1010, 1, 0), (0, 5, 4, 1)])
    sc = scores_of([(int(0.93 * ONE) * 251, 251, 240, int(0.41 * ONE)), (ONE * 10, 10, 10, ONE), (int(0.5004 * ONE) * 5, 5, 3, ONE // 2)])
    want, lines, ids = _check([b"chr1", b"scaf2"], True, rows, sc, 0, [2000, 5], rmout.pairs_of_repeats(range(1, 5)), -1, 8)
    assert (lines, ids) == (3, 3)
    assert want.split(b"\n")[0] == (b"  930   0.0  0.0  0.0  chr1                   100       350      (1650) +  Alu          SINE/Alu"
                                    b"              1    251    (0)      9")
    assert want.split(b"\n")[2].split()[7] == b"(0)"


@pytest.mark.parametrize("by_contig", [False, True])
@pytest.mark.parametrize("min_score", [0, 1, 600, 1000])
def test_layout_filter_and_field_extremes(by_contig, min_score):
    rows, scores = _corpus()
    names, ends = (NAMES, ENDS) if by_contig else (NAMES[1:2], [TOP])
    if not by_contig:
        rows = rows.copy()
        rows["contig"] = 7                                                            # (not read without by_contig)
    want, lines, ids = _check(names, by_contig, rows, scores, min_score, ends, PAIRS, 5, 0)
    assert 0 < lines and (lines == len(rows)) == (min_score == 0) and 0 < ids <= lines
    if min_score == 0:
        cols = [ln.split() for ln in want.split(b"\n")[:-1]]
        assert {c[5] for c in cols} >= {b"1", b"10", b"100000000", str((1 << 32) + 1).encode(), str(TOP).encode()}
        assert {c[6] for c in cols} >= {b"9", b"100000000", str(1 << 32).encode(), str(TOP).encode()}
        assert b"(0)" in {c[7] for c in cols} and [int(c[0]) for c in cols[:13]] == [1000, 0, 0, 1000, 0, 1000, 429, 1, 0, 600, 599, 1000, 999]
        assert {len(c[9]) for c in cols} >= {1, 255} and {len(c[10]) for c in cols} >= {1, 255}
        if by_contig:
            assert {len(c[4]) for c in cols} == {1, 255, len(NAMES[2])}
    else:
        emitted = [int(ln.split()[0]) for ln in want.split(b"\n")[:-1]]
        assert min(emitted) >= min_score


@pytest.mark.parametrize("nrows", [0, 1, 256, 257, 5000])
def test_sizes(nrows):
    rng = np.random.default_rng(23 + nrows)
    if nrows == 0:                                                                    # no rows: no device work
        rc, n, lines, ids, text, work = text_call(NAMES, True, segs([]), scores_of([]), 0, ENDS, PAIRS, 5, 5, cap=64)
        assert rc == 0 and (n, lines, ids) == (0, 0, 0) and text.untouched() and work.untouched()
        return
    big = np.zeros(nrows, segs([]).dtype)
    big["start"] = np.sort(rng.integers(0, (1 << 32) - (1 << 20), nrows))
    big["end"] = big["start"] + rng.integers(1, 1 << 20, nrows)
    big["label"] = rng.integers(1, 5, nrows)
    big["contig"] = np.sort(rng.integers(0, 3, nrows))
    sc = random_scores(nrows, rng, filtered=0.2)
    for low, join, id0 in ((0, -1, 0), (500, 1 << 19, 97)):
        want, lines, ids = _check(NAMES, True, big, sc, low, ENDS, PAIRS, join, id0)
        assert (lines == nrows) == (low == 0 or nrows == 1 and lines == 1)
    if nrows == 5000:
        assert lines > 2048 and 0 < ids < lines                                       # ordinals and IDs cross a tile of the scan


@pytest.mark.parametrize("id0", [0, 8, 97, 10 ** 9 + 5, 1 << 62])
def test_ids_gain_digits_between_filtered_rows(id0):
    """A filtered first row, a filtered last row and filtered rows between emitted ones: they do not count."""
    n = 12
    rows = segs([(10 * i, 10 * i + 5, 1 + i % 4, 0) for i in range(n)])
    sc = scores_of([(0, 7, 0, 0) if i in (0, 3, 4, 8, n - 1) else (7 * ONE, 7, 7, ONE) for i in range(n)])
    want, lines, ids = _check([b"r"], False, rows, sc, 1, [200], rmout.pairs_of_repeats(range(1, 5)), -1, id0)
    assert lines == ids == n - 5
    got = [int(ln.split()[-1]) for ln in want.split(b"\n")[:-1]]
    assert got == list(range(id0 + 1, id0 + 1 + lines))
    lens = {len(ln) for ln in want.split(b"\n")[:-1]}
    assert lens == {132} if id0 < 10 ** 5 else min(lens) > 132                        # 9 -> 10 and 99 -> 100 stay inside the 6 columns


@pytest.mark.parametrize("join", [-1, 0, 5, 1 << 40])
def test_join_gaps_and_runs_across_the_tile_edge(join):
    """4 500 rows of two records: runs of one label whose gaps are 0, 5, 6 and large, with filtered rows inside runs; a run spans
    rows 2 040 .. 2 060 (the edge of the first scan tile) and another the record edge."""
    rng = np.random.default_rng(5)
    n = 4500
    gaps = rng.choice([0, 5, 6, 1000], n)
    label = 1 + (np.arange(n) // 7) % 4
    gaps[2035:2065], label[2035:2065] = 0, 2
    rows = np.zeros(n, segs([]).dtype)
    pos = 0
    for i in range(n):
        if i == 3000:
            pos = 0
        rows["start"][i] = pos + int(gaps[i])
        rows["end"][i] = rows["start"][i] + 3
        pos = int(rows["end"][i])
    rows["label"], rows["contig"] = label, (np.arange(n) >= 3000)
    label[2995:3005] = 3                                                              # one label across the record edge
    rows["label"] = label
    drop = rng.random(n) < 0.15
    drop[2030:2070] = False                                                           # (a filtered row is a gap of its own 3 bases)
    sc = scores_of([(0, 7, 0, 0) if k else (7 * ONE, 7, 7, ONE) for k in drop])
    want, lines, ids = _check([b"a", b"b"], True, rows, sc, 1, [1 << 30, 1 << 30], PAIRS, join, 99_990)
    emitted = [bool(int(s["sum"])) for s in sc]
    assert (ids == lines) == (join < 0)
    got = [int(ln.split()[-1]) for ln in want.split(b"\n")[:-1]]
    assert (got, ids) == rmout.reference_ids(rows, emitted, True, join, 99_990)
    if join >= 0:
        edge = [g for g, i in zip(got, np.flatnonzero(emitted)) if 2040 <= i <= 2060]
        assert len(set(edge)) == 1 and len(edge) > 10                                # one ID over the tile edge
        at = {int(i): g for g, i in zip(got, np.flatnonzero(emitted))}
        last0, first1 = max(i for i in at if i < 3000), min(i for i in at if i >= 3000)
        assert at[first1] == at[last0] + 1                                            # and never one over the record edge
    if join == 1 << 40:
        assert ids < lines // 3


def test_a_batch_with_a_record_without_a_row():
    rows = segs([(0, 5, 1, 0), (7, 9, 2, 0), (3, 4, 1, 2), (5, 6, 2, 3)])             # record 1 has no row
    sc = scores_of([(5 * ONE, 5, 5, ONE), (ONE, 2, 1, 0), (ONE // 2, 1, 1, ONE // 2), (ONE, 1, 1, ONE)])
    want, lines, ids = _check([b"a", b"norows", b"c", b"d"], True, rows, sc, 0, [9, 1, 4, 7], PAIRS, 0, 3)
    assert lines == ids == 4 and b"norows" not in want and [ln.split()[7] for ln in want.split(b"\n")[:-1]] == [b"(4)", b"(0)", b"(0)", b"(1)"]


def test_every_row_filtered_gives_no_byte():
    rows, scores = _corpus()
    scores = scores.copy()
    scores["sum"] = 0
    rc, n, lines, ids, text, work = text_call(NAMES, True, rows, scores, 1, ENDS, PAIRS, 5, 4, cap=64)
    assert rc == 0 and (n, lines, ids) == (0, 0, 0) and text.untouched() and work.guards_intact()


def test_capacity_one_byte_short_and_two_calls_alike():
    rows, scores = _corpus()
    want, lines, ids = rmout.reference_lines(NAMES, True, rows, scores, 0, ENDS, PAIRS, 5, 8)
    rc, n, got_lines, got_ids, text, work = text_call(NAMES, True, rows, scores, 0, ENDS, PAIRS, 5, 8, cap=len(want) - 1)
    assert rc == 0 and (n, got_lines, got_ids) == (len(want), lines, ids) and text.untouched() and work.guards_intact()
    texts = []
    for _ in range(2):                                                                # the exact capacity is enough, and twice the same
        rc, n, _l, _i, text, work = text_call(NAMES, True, rows, scores, 0, ENDS, PAIRS, 5, 8, cap=len(want))
        assert rc == 0 and text.guards_intact()
        texts.append(text.body().cpu().numpy().tobytes())
    assert texts[0] == texts[1] == want


def test_refusals_leave_the_text_untouched():
    from deepgrp_amd._lib import lib
    rows, scores = _corpus()
    cap = len(rmout.reference_lines(NAMES, True, rows, scores, 0, ENDS, PAIRS)[0]) + 64

    def refused(words, rows=rows, scores=scores, ends=ENDS, names=NAMES, by_contig=True, **k):
        rc, n, lines, ids, text, work = text_call(names, by_contig, rows, scores, 0, ends, PAIRS, cap=cap, **k)
        assert rc == EINVAL and words in lib().dgrp_last_error() and text.untouched() and work.guards_intact(), (words, lib().dgrp_last_error())

    for bases in (0, -3):
        bad = scores.copy()
        bad["bases"][len(bad) - 2] = bases
        refused(b"no scored base", scores=bad)
    bad = scores.copy()
    bad["sum"][3] += 1                                                                # a mean above 1: outside the 64-bit envelope
    refused(b"envelope", scores=bad)
    for contig in (3, -1):
        bad = rows.copy()
        bad["contig"][len(bad) - 1 if contig == 3 else 0] = contig
        refused(b"outside the names", rows=bad)
    bad = rows.copy()                                                                 # a name, but no record end: 4 names, 3 records
    bad["contig"][len(bad) - 1] = 3
    refused(b"outside the records", rows=bad, names=NAMES + [b"more"])
    for label in (0, 5, -1):
        bad = rows.copy()
        bad["label"][6] = label
        refused(b"outside the class names", rows=bad)
    for start, end in ((-1, 5), (7, 7), (9, 8)):
        bad = rows.copy()
        bad["start"][0], bad["end"][0] = start, end
        refused(b"start < 0 or start >= end", rows=bad)
    bad = rows.copy()
    bad["end"][0] = ENDS[0] + 1
    refused(b"ends behind its record's end", rows=bad)
    bad = rows.copy()
    bad["contig"][5] = 1                                                              # records 0 0 0 0 0 1 0 ...
    refused(b"do not ascend", rows=bad)
    for k, words in ((dict(id0=-1), b"id0"), (dict(join=-2), b"join_gap")):
        rc, _n, _l, _i, text, work = text_call(NAMES, True, rows, scores, 0, ENDS, PAIRS, cap=cap, **k)
        assert rc == EINVAL and words in lib().dgrp_last_error() and text.untouched() and work.untouched()
    rc, _n, _l, _i, text, work = text_call(NAMES, True, rows, scores, 0, [TOP, 0, TOP], PAIRS, cap=cap)
    assert rc == EINVAL and b"2^62" in lib().dgrp_last_error() and text.untouched() and work.untouched()
    rc, _n, _l, _i, text, work = text_call(NAMES, True, rows, scores, 0, ENDS, PAIRS, cap=cap, short_work=1)
    assert rc == ENOMEM and b"workspace" in lib().dgrp_last_error() and text.untouched() and work.untouched()


def test_pipeline_method_takes_the_retry():
    """ContigPipeline.rmout_text_batch: its capacity guess is short for class names of 255 bytes, so the first case takes the retry."""
    from deepgrp_amd.pipeline import ContigPipeline
    rows, scores = _corpus()
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
    for pairs in ([(b"w" * 255, b"v" * 255)] * 4, rmout.pairs_of_repeats((4, 3, 2, 1))):
        for low, join, id0 in ((0, -1, 0), (600, 5, 99)):
            d_text, lines, ids = ContigPipeline.rmout_text_batch(NAMES, True, d_rows, d_scores, low, ENDS, pairs, join, id0)
            assert (d_text.cpu().numpy().tobytes(), lines, ids) == rmout.reference_lines(NAMES, True, rows, scores, low, ENDS, pairs, join, id0)


def test_a_late_producer_on_a_side_stream():
    """One synchronisation (the read-back of totals and flags), the write kernel behind it: the inputs are read behind the stream's
    earlier work, the host tables may be dropped on return, and the text is complete behind the call on that stream."""
    import ctypes as C

    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import require_gpu
    from stream_harness import Harness
    L = lib()
    H = Harness(require_gpu())
    assert H.choose_side(L) is not None, H.control
    rows, scores = _corpus()
    want, lines, ids = rmout.reference_lines(NAMES, True, rows, scores, 600, ENDS, PAIRS, 5, 97)
    poison_rows, poison_scores = rows.copy(), scores.copy()
    poison_rows["start"] += 3
    poison_rows["end"] += 3
    poison_rows["label"] = 1 + poison_rows["label"] % 4
    poison_scores["sum"] //= 2
    raw, blob, off, cblob, coff = tables(NAMES, PAIRS)
    cap = len(want) + 100
    wb = int(L.dgrp_rmout_text_workspace_bytes(len(rows), len(raw), len(blob), len(PAIRS), len(cblob), len(ENDS)))

    def call(b, wk, st, t):
        got, ln, nid = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
        rc = L.dgrp_rmout_text_batch(blob, t["off"].ctypes.data, len(raw), 1, cblob, t["coff"].ctypes.data, len(PAIRS), b["rows"].data_ptr(),
                                     b["scores"].data_ptr(), len(rows), 600, len(ENDS), t["ends"].ctypes.data, 5, 97, b["text"].data_ptr(),
                                     cap, C.byref(got), C.byref(ln), C.byref(nid), wk.data_ptr(), wb, st)
        return rc, (got.value, ln.value, nid.value)
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    late, host, _idle, host_idle = H.run(call, {"rows": (as_bytes(rows), as_bytes(poison_rows)), "scores": (as_bytes(scores), as_bytes(poison_scores))},
                                         {"text": np.full(cap, 0x5A, np.uint8)}, work_bytes=wb, sync=True, drained=False,
                                         tables={"off": off.copy(), "coff": coff.copy(), "ends": np.array(ENDS, np.int64)})
    assert host == host_idle == (len(want), lines, ids)
    assert late["text"][:len(want)].tobytes() == want and (late["text"][len(want):] == 0x5A).all()
