"""dgrp_bed_index_batch (the tabix pieces of the device's BED text, predict --bed_index): its chunks, linear index and last ends equal
bed.reference_index_parts (Python integers); through tabix.IndexBuilder, with members deflated on the host from the device's text,
they give the payload tabix.reference_index reads off the finished file, and tabix.query answers what a scan of the lines answers.
The corpus: rows in and across a bin boundary of every level, a row ending at 2^29, filtered rows at the head of a record and
inside a run, records without a line, consecutive records of one name, a name that reappears (which IndexBuilder refuses), a line
over 1 800 windows with rows nested in it, 5 000 rows; every refusal and a chunk capacity too small leave the outputs untouched."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import EINVAL, ENOMEM, ONE, index_call, index_parts, random_scores, segs, text_call  # noqa: E402
from deepgrp_amd import bed, gz, tabix  # noqa: E402

MIN_SCORE = 500
TOP = 1 << 29


def _corpus():
    """-> names, rows, scores, rec_end.  Record 0: the bin levels and the long line; 1: only a filtered row; 2: no row; 3 and 4:
    consecutive records of one name; 5: a short tail record."""
    spans = []                                                                        # (start, end, filtered) of record 0
    spans += [(3, 9, True), (10, 20, True)]                                           # filtered rows at the head of the record
    spans += [(30, 40, False), (50, 60, True), (70, 80, False)]                       # a filtered row inside a run of one bin
    spans += [(1000, 1000 + 30_000_000, False)]                                       # 1 832 windows; what follows below 30 001 000 is nested
    for shift in (14, 17, 20, 23, 26):
        edge = 3 << shift
        spans += [(edge - 50, edge - 40, False), (edge - 5, edge + 5, False), (edge + 7, edge + 19, False), (edge + 19, edge + 30, True)]
    spans += [(40_000_000, 40_000_100, False), (TOP - 16_384, TOP - 1, False), (TOP - 100, TOP, False)]
    spans.sort(key=lambda t: t[0])
    rows = [(a, b, 1 + i % 5, 0) for i, (a, b, _f) in enumerate(spans)]
    filt = [f for _a, _b, f in spans]
    rows += [(100, 200, 2, 1)]                                                        # record 1: its only row is filtered
    filt += [True]
    rows += [(0, 16_384, 1, 3), (16_383, 16_385, 2, 3), (16_385, 140_000, 3, 3)]      # record 3 ("twin")
    filt += [False, False, False]
    rows += [(5, 20_000, 1, 4), (6, 8, 2, 4), (150_000, 150_001, 3, 4)]               # record 4 ("twin" again): its first line is long
    filt += [False, False, False]
    rows += [(7, 9, 1, 5)]
    filt += [False]
    rng = np.random.default_rng(4)
    sc = random_scores(len(rows), rng)
    sc["sum"] = [0 if f else max(int(s), int(b) * (ONE // 2 + ONE // 8)) for f, s, b in zip(filt, sc["sum"], sc["bases"])]
    sc["qmin"] = 0
    names = [b"chrA", b"quiet", b"norows", b"twin", b"twin", b"tail"]
    return names, segs(rows), sc, [TOP, 1000, 5000, 140_000, 150_001, 16_384]


def _file_and_payload(names, by_contig, rows, scores, min_score, rec_end):
    """The device's text and index pieces -> (the `.bed.gz` bytes, IndexBuilder's payload, the text)."""
    want_text = bed.reference_lines(names, by_contig, rows, scores, min_score)
    rc, n, text, _work = text_call(names, by_contig, rows, scores, min_score)
    assert rc == 0 and n == len(want_text)
    got_text = text.body(n).cpu().numpy().tobytes()
    assert got_text == want_text
    rc, nchunks, chunks, linear, last, work, wpref = index_call(names, by_contig, rows, scores, min_score, rec_end)
    assert rc == 0
    assert all(a.guards_intact() for a in (chunks, linear, last, work))
    c, lin, le = index_parts(chunks, nchunks, linear, last)
    want_c, want_lin, want_wpref, want_le = bed.reference_index_parts(names, by_contig, rows, scores, min_score, rec_end)
    assert np.array_equal(wpref, want_wpref)
    assert nchunks == len(want_c) and np.array_equal(c, want_c)
    bad = np.flatnonzero(lin != want_lin)
    assert bad.size == 0, (bad[:5], lin[bad[:5]], want_lin[bad[:5]])
    assert np.array_equal(le, want_le)
    members = gz.bgzf_compress(got_text, eof=False)
    sizes, text_len = tabix.member_sizes(members)
    builder = tabix.IndexBuilder()
    raw = [nm if isinstance(nm, bytes) else nm.encode() for nm in names]
    builder.add(0, sizes, text_len, raw, c, lin, wpref, le)
    return members + gz.BGZF_EOF, builder, got_text


def _queries_match_a_scan(data, payload, text, regions):
    ix = tabix.read_index(payload)
    lines = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    for name, beg, end in regions:
        scan = [b"\t".join(f) for f in lines if f[0] == name and int(f[1]) < end and int(f[2]) > beg]
        assert tabix.query(ix, data, name, beg, end) == scan, (name, beg, end)
    return ix


def test_corpus_index_is_the_reference_index():
    names, rows, scores, rec_end = _corpus()
    data, builder, text = _file_and_payload(names, True, rows, scores, MIN_SCORE, rec_end)
    payload = builder.payload()
    assert payload == tabix.reference_index(data)
    regions = [(b"chrA", 0, TOP), (b"chrA", 0, 1), (b"chrA", 35, 75), (b"chrA", 29_000_000, 29_000_001), (b"chrA", 30_001_000, 30_001_001),
               (b"chrA", TOP - 1, TOP), (b"twin", 16_384, 16_385), (b"twin", 0, 200_000), (b"tail", 0, 10), (b"quiet", 0, 1000)]
    regions += [(b"chrA", (3 << s) - 1, (3 << s) + 1) for s in (14, 17, 20, 23, 26)]
    ix = _queries_match_a_scan(data, payload, text, regions)
    assert ix["names"] == [b"chrA", b"twin", b"tail"]                                 # the records without a line are no sequences
    bins = set(ix["bins"][0])
    assert {0, 1 + (3 << 26 >> 26) - 1} & bins and len(bins) > 12                     # every level is present
    for first in (4681, 585, 73, 9, 1):
        assert any(first <= b < first * 8 + 1 for b in bins), first
    assert len(ix["linear"][0]) == TOP >> 14 and len(ix["linear"][1]) == (150_000 >> 14) + 1
    # the running maximum: the rows nested in the long line claim no window, so its windows all name the long line
    lin = ix["linear"][0]
    assert len(set(lin[1:1831].tolist())) == 1 and lin[1832] != lin[1830]


def test_one_record_without_by_contig():
    names, rows, scores, rec_end = _corpus()
    mine = rows["contig"] == 0
    data, builder, text = _file_and_payload([b"solo"], False, rows[mine], scores[mine], MIN_SCORE, [TOP])
    assert builder.payload() == tabix.reference_index(data)
    _queries_match_a_scan(data, builder.payload(), text, [(b"solo", 0, TOP), (b"solo", 49_000, 49_200), (b"solo", TOP - 50, TOP)])


def test_a_name_that_reappears_is_refused_by_the_builder():
    names, rows, scores, rec_end = _corpus()
    names = [b"chrA", b"quiet", b"norows", b"twin", b"chrA", b"tail"]
    with pytest.raises(tabix.IndexRefused, match="reappears"):
        _file_and_payload(names, True, rows, scores, MIN_SCORE, rec_end)              # (the device's pieces are checked on the way)
    text = bed.reference_lines(names, True, rows, scores, MIN_SCORE)
    with pytest.raises(tabix.IndexRefused, match="reappears"):
        tabix.reference_index(gz.bgzf_compress(text))


@pytest.mark.parametrize("min_score", [0, MIN_SCORE])
def test_five_thousand_rows(min_score):
    rng = np.random.default_rng(23)
    n, ends = 5000, [TOP, 3_000_000, 70_000_000]
    rows = np.zeros(n, segs([]).dtype)
    rows["contig"] = np.sort(rng.integers(0, 3, n))
    for r, e in enumerate(ends):
        m = rows["contig"] == r
        k = int(m.sum())
        start = np.sort(rng.integers(0, e - 1, k))
        width = np.where(rng.random(k) < 0.02, rng.integers(1, e, k), rng.integers(1, 30_000, k))
        rows["start"][m] = start
        rows["end"][m] = np.minimum(start + width, e)
    rows["label"] = rng.integers(1, 5, n)
    scores = random_scores(n, rng, filtered=0.3)
    names = [b"one", b"two", b"three"]
    data, builder, text = _file_and_payload(names, True, rows, scores, min_score, ends)
    assert len(tabix.member_sizes(data)[0]) > 3                                       # several members: virtual offsets cross them
    payload = builder.payload()
    assert payload == tabix.reference_index(data)
    _queries_match_a_scan(data, payload, text, [(b"one", 123_456_789, 123_556_789), (b"two", 0, 3_000_000), (b"three", 69_000_000, 70_000_000),
                                                (b"one", TOP - 20_000, TOP), (b"three", 16_384, 16_385)])


def _untouched(out):
    rc, _n, chunks, linear, last, work, _w = out
    return chunks.untouched() and linear.untouched() and last.untouched() and work.guards_intact()


def test_refusals_leave_the_outputs_untouched():
    from deepgrp_amd._lib import lib
    names, rows, scores, rec_end = _corpus()

    def refused(words, rows=rows, scores=scores, rec_end=rec_end, by_contig=True, names=names):
        out = index_call(names, by_contig, rows, scores, MIN_SCORE, rec_end)
        assert out[0] == EINVAL and words in lib().dgrp_last_error() and _untouched(out), (words, lib().dgrp_last_error())

    refused(b"2^29", rec_end=[TOP + 1] + rec_end[1:])
    refused(b"ends behind its record", rec_end=rec_end[:5] + [8])                     # the tail row ends at 9
    bad = rows.copy()
    bad["start"][0] = -1
    refused(b"start < 0 or start >= end", rows=bad)
    bad = rows.copy()
    bad["end"][1] = bad["start"][1]
    refused(b"start < 0 or start >= end", rows=bad)
    bad = rows.copy()
    bad["contig"][-1] = 3                                                             # record 3 behind record 4
    refused(b"do not ascend", rows=bad)
    bad = rows.copy()
    bad[[2, 3]] = bad[[3, 2]]                                                         # two rows of record 0 change places
    refused(b"starts descend", rows=bad)
    bad = rows.copy()
    bad["contig"][-1] = 6
    refused(b"outside the names", rows=bad)
    bad = scores.copy()
    bad["bases"][7] = 0
    refused(b"no scored base", scores=bad)
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, short_work=1)
    assert out[0] == ENOMEM and out[2].untouched() and out[3].untouched() and out[5].untouched()
    # a filtered row is still a row: it must lie inside its record and in order
    bad = rows.copy()
    assert scores["sum"][0] == 0
    bad["start"][0], bad["end"][0] = 25, 26                                           # behind its successor's start of 10
    refused(b"starts descend", rows=bad)


def test_chunk_capacity_too_small():
    names, rows, scores, rec_end = _corpus()
    want = len(bed.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end)[0])
    assert want > 10
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, chunk_cap=want - 1)
    assert out[0] == 0 and out[1] == want and _untouched(out)
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, chunk_cap=want)   # the exact capacity is enough
    assert out[0] == 0 and out[1] == want and out[2].guards_intact()
    # no rows: nothing to do; every row filtered: no chunk, a linear index of -1
    out = index_call(names, True, rows[:0], scores[:0], MIN_SCORE, rec_end)
    assert out[0] == 0 and out[1] == 0 and _untouched(out)
    none = scores.copy()
    none["sum"] = 0
    out = index_call(names, True, rows, none, MIN_SCORE, rec_end)
    _c, lin, le = index_parts(out[2], 0, out[3], out[4])
    assert out[0] == 0 and out[1] == 0 and (lin == -1).all() and (le == 0).all() and out[2].untouched()


def test_pipeline_method_and_a_side_stream():
    from deepgrp_amd.pipeline import ContigPipeline
    names, rows, scores, rec_end = _corpus()
    want = bed.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
        d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
        got = ContigPipeline.bed_index_batch(names, True, d_rows, d_scores, MIN_SCORE, rec_end)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    with pytest.raises(tabix.IndexRefused):
        ContigPipeline.bed_index_batch(names, True, d_rows, d_scores, MIN_SCORE, [TOP + 1] + rec_end[1:])
