"""dgrp_gff_index_batch (the tabix pieces of the device's GFF3 text, predict --bed_gff3 --bed_index): its chunks, linear index and last
ends equal gff.reference_index_parts (Python integers) on the corpus of tests/test_gpu_bed_index.py (nested and wide lines, rows in
and across a bin boundary of every level, a record without a line, consecutive records of one name, filtered rows at the head of a
record and inside a run) and on 5 000 rows, with ordinals that gain digits on the way; through tabix.IndexBuilder under the gff
preset, behind the header member, they give the payload gff.reference_index reads off the finished file, and gff.query answers
what a scan of the lines answers; the refusals and a chunk capacity too small leave the outputs untouched."""
import numpy as np
import pytest

from conftest import GOLDEN  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import EINVAL, ENOMEM, index_parts, random_scores, segs  # noqa: E402
from gff_device import index_call, text_call  # noqa: E402
from test_gpu_bed_index import MIN_SCORE, TOP, _corpus  # noqa: E402
from deepgrp_amd import gff, gz, tabix  # noqa: E402

CNAMES = [b"LTR", b"SINE/Alu", b"a;b", b"w" * 200, b"E"]                              # the corpus has labels 1..5
ID0 = 97                                                                              # the corpus's ordinals cross 99 -> 100


def _file_and_payload(names, by_contig, rows, scores, min_score, rec_end, class_names, id0):
    """The device's text and index pieces -> (the `.gff3.gz` bytes, IndexBuilder's payload, the text without the header)."""
    want_text, lines = gff.reference_lines(names, by_contig, rows, scores, min_score, class_names, id0)
    rc, n, got_lines, text, _work = text_call(names, by_contig, rows, scores, min_score, class_names, id0)
    assert rc == 0 and n == len(want_text) and got_lines == lines
    got_text = text.body(n).cpu().numpy().tobytes()
    assert got_text == want_text
    rc, nchunks, chunks, linear, last, work, wpref = index_call(names, by_contig, rows, scores, min_score, rec_end, class_names, id0)
    assert rc == 0
    assert all(a.guards_intact() for a in (chunks, linear, last, work))
    c, lin, le = index_parts(chunks, nchunks, linear, last)
    want_c, want_lin, want_wpref, want_le = gff.reference_index_parts(names, by_contig, rows, scores, min_score, rec_end, class_names, id0)
    assert np.array_equal(wpref, want_wpref)
    assert nchunks == len(want_c) and np.array_equal(c, want_c)
    bad = np.flatnonzero(lin != want_lin)
    assert bad.size == 0, (bad[:5], lin[bad[:5]], want_lin[bad[:5]])
    assert np.array_equal(le, want_le)
    head = gff.header_member(1)
    members = gz.bgzf_compress(got_text, eof=False)
    sizes, text_len = tabix.member_sizes(members)
    builder = tabix.IndexBuilder(gff.PRESET)
    builder.add(len(head), sizes, text_len, [gff.escape_seqid(nm) for nm in names], c, lin, wpref, le)
    return head + members + gz.BGZF_EOF, builder.payload(), got_text


def _queries_match_a_scan(data, payload, text, regions):
    ix = gff.read_index(payload)
    lines = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
    found = 0
    for name, beg, end in regions:
        scan = [b"\t".join(f) for f in lines if f[0] == name and int(f[3]) - 1 < end and int(f[4]) > beg]
        assert gff.query(ix, data, name, beg, end) == scan, (name, beg, end)
        found += len(scan)
    assert found > 0
    return ix


def test_corpus_index_is_the_reference_index():
    names, rows, scores, rec_end = _corpus()
    data, payload, text = _file_and_payload(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0)
    assert payload == gff.reference_index(data)
    assert payload[4:36] == np.array([3, 0, 1, 4, 5, ord("#"), 0, len(b"chrA\0twin\0tail\0")], "<i4").tobytes()
    regions = [(b"chrA", 0, TOP), (b"chrA", 0, 1), (b"chrA", 35, 75), (b"chrA", 29_000_000, 29_000_001), (b"chrA", 30_001_000, 30_001_001),
               (b"chrA", TOP - 1, TOP), (b"twin", 16_384, 16_385), (b"twin", 0, 200_000), (b"tail", 0, 10), (b"quiet", 0, 1000)]
    regions += [(b"chrA", (3 << s) - 1, (3 << s) + 1) for s in (14, 17, 20, 23, 26)]
    ix = _queries_match_a_scan(data, payload, text, regions)
    assert ix["names"] == [b"chrA", b"twin", b"tail"]                                 # the records without a line are no sequences
    first = min(c[0] for b in ix["bins"][0].values() for c in b)
    assert first == len(gff.header_member(1)) << 16                                   # the first chunk begins behind the header member
    lin = ix["linear"][0]
    assert len(lin) == TOP >> 14 and len(set(lin[1:1831].tolist())) == 1 and lin[1832] != lin[1830]     # the running maximum
    ids = [int(ln.split(b"ID=r")[1].split(b";")[0]) for ln in text.split(b"\n")[:-1]]
    assert ids == list(range(ID0 + 1, ID0 + 1 + len(ids))) and ids[-1] >= 100


def test_one_record_without_by_contig_and_an_escaped_name():
    names, rows, scores, rec_end = _corpus()
    mine = rows["contig"] == 0
    data, payload, text = _file_and_payload([b"so lo;1"], False, rows[mine], scores[mine], MIN_SCORE, [TOP], None, 0)
    assert payload == gff.reference_index(data)
    ix = _queries_match_a_scan(data, payload, text, [(b"so%20lo%3B1", 0, TOP), (b"so%20lo%3B1", 49_000, 49_200), (b"so%20lo%3B1", TOP - 50, TOP)])
    assert ix["names"] == [b"so%20lo%3B1"]                                            # the index names column 1 as it is written


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
    data, payload, text = _file_and_payload([b"one", b"two", b"three"], True, rows, scores, min_score, ends, CNAMES, 8)
    assert len(tabix.member_sizes(data)[0]) > 4                                       # several members: virtual offsets cross them
    assert payload == gff.reference_index(data)
    _queries_match_a_scan(data, payload, text, [(b"one", 123_456_789, 123_556_789), (b"two", 0, 3_000_000), (b"three", 69_000_000, 70_000_000),
                                                (b"one", TOP - 20_000, TOP), (b"three", 16_384, 16_385)])


def _untouched(out):
    rc, _n, chunks, linear, last, work, _w = out
    return chunks.untouched() and linear.untouched() and last.untouched() and work.guards_intact()


def test_refusals_leave_the_outputs_untouched():
    from deepgrp_amd._lib import lib
    names, rows, scores, rec_end = _corpus()

    def refused(words, rows=rows, scores=scores, rec_end=rec_end, class_names=CNAMES, id0=ID0):
        out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, class_names, id0)
        assert out[0] == EINVAL and words in lib().dgrp_last_error() and _untouched(out), (words, lib().dgrp_last_error())

    refused(b"2^29", rec_end=[TOP + 1] + rec_end[1:])
    refused(b"ends behind its record", rec_end=rec_end[:5] + [8])
    bad = rows.copy()
    bad["start"][0] = -1
    refused(b"start < 0 or start >= end", rows=bad)
    bad = rows.copy()
    bad["contig"][-1] = 3
    refused(b"do not ascend", rows=bad)
    bad = rows.copy()
    bad[[2, 3]] = bad[[3, 2]]
    refused(b"starts descend", rows=bad)
    bad = rows.copy()
    bad["contig"][-1] = 6
    refused(b"outside the names", rows=bad)
    bad = scores.copy()
    bad["bases"][7] = 0
    refused(b"no scored base", scores=bad)
    refused(b"outside the class names", class_names=CNAMES[:4])                       # the corpus has label 5
    refused(b"id0", id0=-1)
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0, short_work=1)
    assert out[0] == ENOMEM and out[2].untouched() and out[3].untouched() and out[5].untouched()


def test_chunk_capacity_too_small():
    names, rows, scores, rec_end = _corpus()
    want = len(gff.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0)[0])
    assert want > 10
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0, chunk_cap=want - 1)
    assert out[0] == 0 and out[1] == want and _untouched(out)
    out = index_call(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0, chunk_cap=want)
    assert out[0] == 0 and out[1] == want and out[2].guards_intact()
    out = index_call(names, True, rows[:0], scores[:0], MIN_SCORE, rec_end, CNAMES, ID0)
    assert out[0] == 0 and out[1] == 0 and _untouched(out)
    none = scores.copy()
    none["sum"] = 0
    out = index_call(names, True, rows, none, MIN_SCORE, rec_end, CNAMES, ID0)
    _c, lin, le = index_parts(out[2], 0, out[3], out[4])
    assert out[0] == 0 and out[1] == 0 and (lin == -1).all() and (le == 0).all() and out[2].untouched()


def test_pipeline_method_and_a_side_stream():
    from deepgrp_amd.pipeline import ContigPipeline
    names, rows, scores, rec_end = _corpus()
    want = gff.reference_index_parts(names, True, rows, scores, MIN_SCORE, rec_end, CNAMES, ID0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
        d_scores = torch.from_numpy(scores.view(np.uint8).copy()).cuda()
        got = ContigPipeline.gff_index_batch(names, True, d_rows, d_scores, MIN_SCORE, rec_end, CNAMES, ID0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    with pytest.raises(tabix.IndexRefused):
        ContigPipeline.gff_index_batch(names, True, d_rows, d_scores, MIN_SCORE, [TOP + 1] + rec_end[1:], CNAMES, ID0)
