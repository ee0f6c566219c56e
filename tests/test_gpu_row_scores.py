"""dgrp_row_scores_batch against bed.reference_scores, bit for bit (every statistic is an exact integer): records of 1 to 2 S + 37
bases (S = 8192, the positions of one workgroup) at rows with gaps between them, the padding filled with 0.75 so that a reader that
strays shows; rows disjoint, overlapping, unordered, clipped, outside, empty, 5000 one-base rows inside one slice (more rows than the
LDS stage holds: the direct path) and one row across three slices; values uniform, special (zero, negatives, NaN, infinity, 1 and
above, a denormal, half-way points), ties and NaN for the first-maximum rule; refusals; memory and workspace contract; the stream
contract with the late-producer harness.  About 165 000 bases in all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import FILLS, SEG, Harness, i64ptr, last_error      # noqa: E402

EINVAL, ENOMEM = -1, -3
S = 8192
LENGTHS = [1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 37]
STARTS = [0, 7, 1_000_003, 0, 7, 1_000_003, 0, 7]
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


@pytest.fixture(scope="module")
def H(L, dev):
    h = Harness(dev)
    h.choose_side(L)
    return h


def _specials():
    half = [(k + 0.5) / 2 ** 24 for k in (0, 1, 2, 5, 1000, 65535, 4194303, 8388606)]          # k < 2^23: exact in float32
    return np.array([0.0, -0.0, -1.0, np.nan, np.inf, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 1e-45] + half, np.float32)


def _case(C, seed):
    """-> probs [rows, C] with gaps of 0.75 between the records, row0, rows per record (lists of (start, end, label))."""
    rng = np.random.default_rng(seed)
    row0, p = [], 3
    for n in LENGTHS:
        row0.append(p)
        p += n + int(rng.integers(1, 70))
    probs = np.full((p + 5, C), 0.75, np.float32)
    per_record = []
    for r, (n, sp, at) in enumerate(zip(LENGTHS, STARTS, row0)):
        block = rng.random((n, C), dtype=np.float32)
        lab = lambda: int(rng.integers(1, C))
        rows = []
        if n >= 4000:
            sv = _specials()
            block[100:100 + sv.size, 1] = sv                                   # specials in a scored column
            block[300:400, :] = 0.25                                           # every column ties: the first one wins
            block[400:500, 0] = 2.0                                            # the label is never the maximum
            block[500:520, 0] = np.nan                                         # a NaN in column 0 is never beaten
            block[520:540, C - 1] = np.nan                                     # a NaN later never wins
            block[540:560, 1] = block[540:560, 0] = 0.9                        # columns 0 and 1 tie at the top
            rows += [(sp + 90, sp + 130, 1), (sp + 100, sp + 100 + sv.size, 1), (sp + 290, sp + 570, 1), (sp + 290, sp + 570, C - 1),
                     (sp + 495, sp + 545, C - 1), (sp + 103, sp + 104, 1), (sp + 108, sp + 109, 1)]
        if r != 2:                                                             # record 2 (64 bases) has no rows at all
            cuts = np.unique(rng.integers(0, n + 1, 24))
            disjoint = [(sp + int(a), sp + int(b), lab()) for a, b in zip(cuts[:-1], cuts[1:]) if rng.random() < 0.7]
            overlap = [(sp + int(a), sp + int(a) + int(rng.integers(0, max(n // 2, 2))), lab()) for a in rng.integers(0, n, 12)]
            edge = [(max(sp - 5, 0), sp + min(3, n), lab()), (sp + max(n - 2, 0), sp + n + 10, lab()), (0, sp + n + 500, lab()),   # clipped
                    (sp + n + 5, sp + n + 50, lab()), (sp + n, sp + n, lab()), (sp + n // 2, sp + n // 2, lab())]                  # outside, empty
            if sp:
                edge.append((0, sp, lab()))                                    # ends where the record begins
            rows += disjoint + overlap + edge
            rng.shuffle(rows)
        if n > 2 * S:
            ones = [(sp + int(a), sp + int(a) + 1, lab()) for a in rng.integers(0, n, 5000)]       # 5000 rows inside one slice
            rows = rows + ones + [(sp + 3, sp + 2 * S + 20, lab())]             # and one row across three slices
        probs[at:at + n] = block
        per_record.append(rows)
    return probs, np.array(row0, np.int64), per_record


def _tables(per_record, lead=3, tail=4):
    """The rows of all records flat, with `lead` rows in front of h_row_off[0] and `tail` behind h_row_off[nrec] that are not the call's."""
    flat = [(5, 9, 1)] * lead + [x for rows in per_record for x in rows] + [(5, 9, 1)] * tail
    a = np.zeros(len(flat), SEG)
    a["start"], a["end"], a["label"] = [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat]
    a["contig"] = -1
    off = lead + np.r_[0, np.cumsum([len(rows) for rows in per_record])]
    return a, off.astype(np.int64)


def _want(probs, row0, lengths, starts, seg, row_off):
    from deepgrp_amd import bed
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE
    want = np.frombuffer(bytes([SENTINEL]) * (len(seg) * 32), ROW_SCORE_DTYPE).copy()
    for r, (at, n, sp) in enumerate(zip(row0, lengths, starts)):
        a, b = int(row_off[r]), int(row_off[r + 1])
        want[a:b] = bed.reference_scores(probs[at:at + n], int(sp), seg[a:b])
    return want


def _run(L, dev, probs, row0, lengths, starts, seg, row_off, fill=0xA5, short=0, C=None):
    """One call on the current stream: -> (rc, scores as ROW_SCORE_DTYPE with the sentinel where nothing was written, probs after)."""
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE
    d_probs = torch.from_numpy(probs).to(dev)
    d_rows = torch.from_numpy(seg.view(np.uint8)).to(dev)
    d_scores = torch.full((len(seg) * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    ln, sp = np.ascontiguousarray(lengths, np.int64), np.ascontiguousarray(starts, np.int64)
    wb = int(L.dgrp_row_scores_workspace_bytes(len(ln), int(row_off[-1] - row_off[0]))) - short
    work = torch.full((max(wb, 1),), fill, dtype=torch.uint8, device=dev)
    rc = L.dgrp_row_scores_batch(d_probs.data_ptr(), probs.shape[1] if C is None else C, len(ln), i64ptr(row0), i64ptr(ln), i64ptr(sp),
                                 d_rows.data_ptr(), i64ptr(row_off), d_scores.data_ptr(), work.data_ptr(), wb,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_scores.cpu().numpy().view(ROW_SCORE_DTYPE), d_probs.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """C -> (probs, row0, seg, row_off, want), computed once."""
    out = {}
    for C in (2, 5, 16, 64):
        probs, row0, per_record = _case(C, 100 + C)
        seg, row_off = _tables(per_record)
        out[C] = (probs, row0, seg, row_off, _want(probs, row0, LENGTHS, STARTS, seg, row_off))
    return out


@pytest.mark.parametrize("C", [2, 5, 16, 64])
def test_scores_bit_for_bit(L, dev, cases, C):
    probs, row0, seg, row_off, want = cases[C]
    rc, got, after = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, row_off)
    assert rc == 0, last_error()
    for k in ("bases", "sum", "qmin", "agree", "pad"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))          # the sentinel outside [row_off[0], row_off[nrec]) included
    np.testing.assert_array_equal(after.view(np.uint32), probs.view(np.uint32))     # d_probs is read only
    inside = want[row_off[0]:row_off[-1]]
    assert (inside["bases"] == 0).any() and (inside["bases"] > 2 * S).any() and (inside["bases"] == 1).sum() >= 5000
    assert (inside["pad"] == 0).all() and int(row_off[3]) == int(row_off[2])          # a record without rows


@pytest.mark.parametrize("C", [5, 16])
def test_workspace_contents_do_not_matter(L, dev, cases, C):
    probs, row0, seg, row_off, want = cases[C]
    for fill in FILLS:
        rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, row_off, fill=fill)
        assert rc == 0, last_error()
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=f"fill {fill:#x}")


def test_refusals_write_nothing(L, dev, cases):
    C = 5
    probs, row0, seg, row_off, want = cases[C]
    untouched = np.full(len(seg) * 32, SENTINEL, np.uint8)
    at = int(row_off[5]) + 2                                                   # a row of record 5
    for what, field, value in (("label 0", "label", 0), ("label = C", "label", C), ("start > end", "start", int(seg["end"][at]) + 1),
                               ("negative start", "start", -1)):
        bad = seg.copy()
        bad[field][at] = value
        rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, bad, row_off)
        assert rc == EINVAL and f"row {at}".encode() in L.dgrp_last_error(), (what, last_error())
        np.testing.assert_array_equal(got.view(np.uint8), untouched, err_msg=what)
    ln = list(LENGTHS)
    ln[2] = 0                                                                  # h_n[r] = 0 (a record without rows, even)
    rc, got, _ = _run(L, dev, probs, row0, ln, STARTS, seg, row_off)
    assert rc == EINVAL
    np.testing.assert_array_equal(got.view(np.uint8), untouched)
    for badC in (1, 65):
        rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, row_off, C=badC)
        assert rc == EINVAL
        np.testing.assert_array_equal(got.view(np.uint8), untouched)
    down = row_off.copy()
    down[4] = down[3] - 1                                                      # row offsets that do not ascend
    rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, down)
    assert rc == EINVAL
    np.testing.assert_array_equal(got.view(np.uint8), untouched)
    rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, row_off, short=1)       # a workspace one byte short
    assert rc == ENOMEM
    np.testing.assert_array_equal(got.view(np.uint8), untouched)


def test_nothing_to_do(L, dev, cases):
    probs, row0, seg, row_off, _want_ = cases[5]
    untouched = np.full(len(seg) * 32, SENTINEL, np.uint8)
    rc, got, _ = _run(L, dev, probs, row0[:0], [], [], seg, row_off[:1])       # no record
    assert rc == 0
    np.testing.assert_array_equal(got.view(np.uint8), untouched)
    flat = np.full(len(LENGTHS) + 1, 3, np.int64)                              # records, but no rows
    rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, seg, flat)
    assert rc == 0
    np.testing.assert_array_equal(got.view(np.uint8), untouched)
    # rows that all miss their records: zeros for them, without a pass over the probabilities
    miss = seg.copy()
    miss["start"], miss["end"] = 5_000_000, 5_000_100
    rc, got, _ = _run(L, dev, probs, row0, LENGTHS, STARTS, miss, row_off)
    assert rc == 0
    assert not got.view(np.uint8)[int(row_off[0]) * 32:int(row_off[-1]) * 32].any()
    assert (got.view(np.uint8)[:int(row_off[0]) * 32] == SENTINEL).all() and (got.view(np.uint8)[int(row_off[-1]) * 32:] == SENTINEL).all()


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
def test_stream_contract(H, L, fill):
    """The row check synchronises the stream once; the scores are ordered behind it on the caller's stream: with the real inputs
    produced late on a side stream the result is the reference's, and the host tables may be dropped on return."""
    rng = np.random.default_rng(21)
    C, ln, sp = 5, [17, 4097, 900], [40, 1000, 7]
    row0 = np.array([5, 60, 4200], np.int64)
    probs = rng.random((5200, C), dtype=np.float32)
    poison = rng.random((5200, C), dtype=np.float32)
    per_record = [[(int(a), int(a) + int(rng.integers(0, 300)), int(rng.integers(1, C))) for a in rng.integers(max(o - 20, 0), o + n + 20, 25)]
                  + [(o, o, 2), (0, o + n + 500, 4)] for n, o in zip(ln, sp)]
    seg, row_off = _tables(per_record, lead=0, tail=0)
    other = seg.copy()
    other["label"] = 1 + other["label"] % (C - 1)
    nrows = len(seg)
    wb = int(L.dgrp_row_scores_workspace_bytes(len(ln), nrows))
    tabs = {"row0": row0, "n": np.array(ln, np.int64), "sp": np.array(sp, np.int64), "ro": row_off}

    def call(b, wk, st, t):
        return L.dgrp_row_scores_batch(b["probs"].data_ptr(), C, len(ln), i64ptr(t["row0"]), i64ptr(t["n"]), i64ptr(t["sp"]), b["rows"].data_ptr(),
                                       i64ptr(t["ro"]), b["sc"].data_ptr(), wk.data_ptr(), wb, st), None
    late, *_ = H.run(call, {"probs": (probs, poison), "rows": (seg.view(np.uint8), other.view(np.uint8))},
                     {"sc": np.full(nrows * 32, SENTINEL, np.uint8)}, work_bytes=wb, fill=fill, sync=True, drained=False, tables=tabs)
    want = _want(probs, row0, ln, sp, seg, row_off)
    np.testing.assert_array_equal(late["sc"], want.view(np.uint8))
