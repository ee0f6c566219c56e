"""dgrp_gff_text_batch (the GFF3 feature lines written on the device, predict --bed_gff3) against gff.reference_lines (Python
integers and bytes), byte for byte, every call between sentinel pages in front of and behind the text and the workspace: 0 / 1 / 256 /
257 / 5 000 rows (more than one scan tile of 2 048), ordinals that gain a digit (9 -> 10, 99 -> 100) and ordinals above 10^9,
emitted rows between filtered ones, a batch with a record without a row, the extremes of start and end, labels and class-name
tables at 2, 5 and 16 classes, names of 1 and 255 bytes, an escaped record name of 765 bytes, the ends and half-way points of the
four figures (the scores of tests/test_gpu_bed_text.py), a capacity one byte short, every refusal, and a late producer on a side
stream (tests/stream_harness.py)."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import EINVAL, ENOMEM, ONE, random_scores, scores_of, segs  # noqa: E402
from gff_device import tables, text_call  # noqa: E402
from test_gpu_bed_text import SCORES  # noqa: E402
from deepgrp_amd import gff  # noqa: E402

TOP = 1 << 29
NAMES = [b"x", b"\xff" * 255, b"scaf;x=1 %"]                                          # the second escapes to 3 * 255 bytes
# (start, end, label): start + 1 gains a digit at 9 and 99 999 999; ends up to 2^29
SPANS = [(0, 7, 1), (8, 9, 4), (9, 42, 2), (99_999_999, 100_000_000, 3), (99_999_998, TOP, 4), (10, TOP - 1, 1), (TOP - 1, TOP, 2)]
CNAMES4 = [b"A", b"SINE/Alu", b"k" * 255, b"odd;=&,%\t\x7fname"]


def _corpus():
    rows = segs([SPANS[i % len(SPANS)] + (i % 3,) for i in range(len(SCORES))])
    return rows, scores_of(SCORES)


def _check(names, by_contig, rows, scores, min_score=0, class_names=None, id0=0):
    want, lines = gff.reference_lines(names, by_contig, rows, scores, min_score, class_names, id0)
    rc, n, got_lines, text, work = text_call(names, by_contig, rows, scores, min_score, class_names, id0)
    assert rc == 0 and n == len(want) and got_lines == lines
    got = text.body(n).cpu().numpy().tobytes()
    if got != want:
        a, b = got.split(b"\n"), want.split(b"\n")
        k = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
        raise AssertionError((k, a[k][-120:], b[k][-120:]))
    assert text.guards_intact() and work.guards_intact()
    assert bool((text.body()[n:] == 0xA5).all())                                      # and nothing behind the text
    return want, lines


def test_the_example_of_the_format():
    rows = segs([(99, 350, 3, 0), (1000, 1010, 1, 0), (0, 5, 4, 1)])
    sc = scores_of([(int(0.93 * ONE) * 251, 251, 240, int(0.41 * ONE)), (ONE * 10, 10, 10, ONE), (int(0.5004 * ONE) * 5, 5, 3, ONE // 2)])
    want, lines = _check([b"chr1", b"scaf;x=1"], True, rows, sc, 0, [b"HSATII", b"b", b"SINE/Alu"] + [b"d"], 8)
    assert lines == 3 and want.split(b"\n")[0] == (b"chr1\tdeepgrp\trepeat_region\t100\t350\t0.9300\t.\t.\t"
                                                   b"ID=r9;Name=SINE/Alu;label=3;score=930;min=0.4100;agree=0.9562")
    assert want.split(b"\n")[2].startswith(b"scaf%3Bx%3D1\tdeepgrp\trepeat_region\t1\t5\t0.5004\t.\t.\tID=r11;Name=d;label=4;")


@pytest.mark.parametrize("by_contig", [False, True])
@pytest.mark.parametrize("min_score", [0, 1, 600, 1000])
def test_extremes_and_half_way_points(by_contig, min_score):
    """The four figures at their ends and half-way points, with the extremes of start, end, names and class names around them."""
    rows, scores = _corpus()
    want, lines = _check(NAMES, by_contig, rows, scores, min_score, CNAMES4, 0)
    assert 0 < lines and (lines == len(rows)) == (min_score == 0)
    if min_score == 0:
        cols = [ln.split(b"\t") for ln in want.split(b"\n")[:-1]]
        assert {c[3] for c in cols} >= {b"1", b"9", b"10", b"100000000", b"99999999"} and str(TOP).encode() in {c[4] for c in cols}
        attrs = [dict(kv.split(b"=", 1) for kv in c[8].split(b";")) for c in cols]
        assert [int(a[b"score"]) for a in attrs[:13]] == [1000, 0, 0, 1000, 0, 1000, 429, 1, 0, 600, 599, 1000, 999]
        assert [c[5] for c in cols[13:19]] == [b"0.0001", b"0.0000", b"0.6173", b"0.6172", b"1.0000", b"0.9999"]
        assert [a[b"min"] for a in attrs[15:19]] == [b"0.0313", b"0.0312", b"0.0938", b"0.0937"]
        assert [a[b"agree"] for a in attrs[13:19]] == [b"0.0001", b"0.0000", b"0.6173", b"0.6172", b"1.0000", b"0.9999"]
        assert [a[b"ID"] for a in attrs] == [b"r%d" % (j + 1) for j in range(len(rows))]
        if by_contig:
            assert {len(c[0]) for c in cols} == {1, 765, len(gff.escape_seqid(NAMES[2]))}


@pytest.mark.parametrize("nrows", [0, 1, 256, 257, 5000])
def test_sizes(nrows):
    rng = np.random.default_rng(17 + nrows)
    if nrows == 0:                                                                    # no rows: no device work
        rc, n, lines, text, work = text_call(NAMES, True, segs([]), scores_of([]), 0, CNAMES4, 5, cap=64)
        assert rc == 0 and n == 0 and lines == 0 and text.untouched() and work.untouched()
        return
    big = np.zeros(nrows, segs([]).dtype)
    big["start"] = np.sort(rng.integers(0, TOP - (1 << 20), nrows))
    big["end"] = big["start"] + rng.integers(1, 1 << 20, nrows)
    big["label"] = rng.integers(1, 5, nrows)
    big["contig"] = np.sort(rng.integers(0, 3, nrows))
    sc = random_scores(nrows, rng, filtered=0.2)
    for low, id0 in ((0, 0), (500, 97)):
        want, lines = _check(NAMES, True, big, sc, low, CNAMES4 if low else None, id0)
        assert (lines == nrows) == (low == 0 or nrows == 1 and lines == 1)
    if nrows == 5000:
        assert lines > 2048                                                           # the ordinals cross a tile of the scan


@pytest.mark.parametrize("id0", [0, 8, 97, 10 ** 9 - 2])
def test_ordinals_gain_digits_between_filtered_rows(id0):
    """A filtered first row, a filtered last row and filtered rows between emitted ones: they do not count, and the line whose
    ordinal gains a digit is one byte longer than the line in front of it."""
    n = 12
    rows = segs([(10 * i, 10 * i + 5, 1 + i % 4, 0) for i in range(n)])
    sc = scores_of([(0, 7, 0, 0) if i in (0, 3, 4, 8, n - 1) else (7 * ONE, 7, 7, ONE) for i in range(n)])
    want, lines = _check([b"r"], False, rows, sc, 1, None, id0)
    assert lines == n - 5
    ids = [int(ln.split(b"ID=r")[1].split(b";")[0]) for ln in want.split(b"\n")[:-1]]
    assert ids == list(range(id0 + 1, id0 + 1 + lines))
    if id0:
        assert len({len(str(j)) for j in ids}) == 2


def test_a_batch_with_a_record_without_a_row():
    rows = segs([(0, 5, 1, 0), (7, 9, 2, 0), (3, 4, 1, 2), (5, 6, 2, 3)])             # record 1 has no row
    sc = scores_of([(5 * ONE, 5, 5, ONE), (ONE, 2, 1, 0), (ONE // 2, 1, 1, ONE // 2), (ONE, 1, 1, ONE)])
    want, lines = _check([b"a", b"norows", b"c", b"d"], True, rows, sc, 0, None, 3)
    assert lines == 4 and b"norows" not in want


@pytest.mark.parametrize("classes", [2, 5, 16])
def test_labels_and_class_names(classes):
    """Labels 1 and C - 1 with a table of C - 1 names (of 1 and 255 bytes among them) and without a table."""
    cn = [b"n%d" % k for k in range(1, classes)]
    cn[0], cn[-1] = b"Z", b"q" * 255
    if classes == 2:
        cn = [b"q" * 255]
    rows = segs([(5, 9, 1, 0), (20, 30, classes - 1, 0), (40, 50, 1, 0)])
    sc = scores_of([(3 * ONE, 4, 2, ONE // 2)] * 3)
    with_table, _ = _check([b"s"], False, rows, sc, 0, cn, 0)
    without, _ = _check([b"s"], False, rows, sc, 0, None, 0)
    assert b"Name=" + cn[-1] + b";label=%d;" % (classes - 1) in with_table and b"Name=class%d;label=%d;" % ((classes - 1,) * 2) in without


def test_every_row_filtered_gives_no_byte():
    rows, scores = _corpus()
    scores = scores.copy()
    scores["sum"] = 0
    rc, n, lines, text, work = text_call(NAMES, True, rows, scores, 1, None, 4, cap=64)
    assert rc == 0 and n == 0 and lines == 0 and text.untouched() and work.guards_intact()


def test_capacity_one_byte_short():
    rows, scores = _corpus()
    want, lines = gff.reference_lines(NAMES, True, rows, scores, 0, CNAMES4, 8)
    rc, n, got_lines, text, work = text_call(NAMES, True, rows, scores, 0, CNAMES4, 8, cap=len(want) - 1)
    assert rc == 0 and n == len(want) and got_lines == lines and text.untouched() and work.guards_intact()
    rc, n, got_lines, text, work = text_call(NAMES, True, rows, scores, 0, CNAMES4, 8, cap=len(want))          # the exact capacity is enough
    assert rc == 0 and text.body().cpu().numpy().tobytes() == want and text.guards_intact()


def test_refusals_leave_the_text_untouched():
    from deepgrp_amd._lib import lib
    rows, scores = _corpus()
    cap = len(gff.reference_lines(NAMES, True, rows, scores, 0, CNAMES4, 0)[0]) + 64

    def refused(words, rows=rows, scores=scores, class_names=CNAMES4, id0=0, by_contig=True):
        rc, _n, _l, text, work = text_call(NAMES, by_contig, rows, scores, 0, class_names, id0, cap=cap)
        assert rc == EINVAL and words in lib().dgrp_last_error() and text.untouched() and work.guards_intact(), (words, lib().dgrp_last_error())

    for bases in (0, -3):
        bad = scores.copy()
        bad["bases"][len(bad) - 2] = bases
        refused(b"no scored base", scores=bad)
    for contig in (3, -1):
        bad = rows.copy()
        bad["contig"][4] = contig
        refused(b"outside the names", rows=bad)
        assert text_call(NAMES, False, bad, scores, 0, CNAMES4, 0, cap=cap)[0] == 0     # without by_contig the column is not read
    bad = scores.copy()
    bad["sum"][3] += 1                                                                # a mean above 1: outside the 64-bit envelope
    refused(b"envelope", scores=bad)
    for label in (0, 5, -1):                                                          # outside 1..4 with a table of four names
        bad = rows.copy()
        bad["label"][6] = label
        refused(b"outside the class names", rows=bad)
        assert text_call(NAMES, True, bad, scores, 0, None, 0, cap=cap + 64)[0] == 0    # without a table every label is class<L>
    rc, _n, _l, text, work = text_call(NAMES, True, rows, scores, 0, CNAMES4, -1, cap=cap)
    assert rc == EINVAL and b"id0" in lib().dgrp_last_error() and text.untouched() and work.untouched()
    rc, _n, _l, text, work = text_call(NAMES, True, rows, scores, 0, CNAMES4, 0, cap=cap, short_work=1)
    assert rc == ENOMEM and b"workspace" in lib().dgrp_last_error() and text.untouched() and work.untouched()


def test_pipeline_method_takes_the_retry():
    """ContigPipeline.gff_text_batch: its capacity guess is short for class names of 255 bytes, so the second case takes the retry."""
    from deepgrp_amd.pipeline import ContigPipeline
    rows, scores = _corpus()
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
    for names, cn in ((NAMES, CNAMES4), ([b"n"], [b"w" * 255] * 4), ([b"n"], None)):
        for low, id0 in ((0, 0), (600, 99)):
            d_text, lines = ContigPipeline.gff_text_batch(names, len(names) > 1, d_rows, d_scores, low, cn, id0)
            assert (d_text.cpu().numpy().tobytes(), lines) == gff.reference_lines(names, len(names) > 1, rows, scores, low, cn, id0)


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
    want, lines = gff.reference_lines(NAMES, True, rows, scores, 600, CNAMES4, 97)
    poison_rows, poison_scores = rows.copy(), scores.copy()
    poison_rows["start"] += 3
    poison_rows["label"] = 1 + poison_rows["label"] % 4
    poison_scores["sum"] //= 2
    raw, blob, off, cblob, coff, nc = tables(NAMES, CNAMES4)
    cap = len(want) + 100
    wb = int(L.dgrp_gff_text_workspace_bytes(len(rows), len(raw), len(blob), nc, len(cblob)))

    def call(b, wk, st, t):
        got, ln = C.c_int64(-7), C.c_int64(-7)
        rc = L.dgrp_gff_text_batch(blob, t["off"].ctypes.data, len(raw), 1, cblob, t["coff"].ctypes.data, nc, b["rows"].data_ptr(),
                                   b["scores"].data_ptr(), len(rows), 600, 97, b["text"].data_ptr(), cap, C.byref(got), C.byref(ln),
                                   wk.data_ptr(), wb, st)
        return rc, (got.value, ln.value)
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    late, host, _idle, host_idle = H.run(call, {"rows": (as_bytes(rows), as_bytes(poison_rows)), "scores": (as_bytes(scores), as_bytes(poison_scores))},
                                         {"text": np.full(cap, 0x5A, np.uint8)}, work_bytes=wb, sync=True, drained=False,
                                         tables={"off": off.copy(), "coff": coff.copy()})
    assert host == host_idle == (len(want), lines)
    assert late["text"][:len(want)].tobytes() == want and (late["text"][len(want):] == 0x5A).all()
