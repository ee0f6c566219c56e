"""The two device entries of `evaluate --boundaries` against their numpy statements: dgrp_row_bounds_batch
(boundaries.reference_bounds; its hits are dgrp_row_hits_batch's on the same call) and dgrp_bound_hist_batch
(boundaries.reference_bound_hist).  Every figure is an integer: equal means equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from deepgrp_amd import boundaries                                      # noqa: E402
from deepgrp_amd.curves import need_of                                  # noqa: E402
from stream_harness import SEG, Harness, i64ptr, last_error             # noqa: E402

EINVAL, ENOMEM = -1, -3
SLICE = 8192                          # EVAL_SLICE: the positions of the widened line one workgroup takes
LDS_ROWS = 1024                       # BOUNDS_LDS_ROWS: a slice crossing more rows adds to d_bounds directly
SENTINEL = -7


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _layout(lengths):
    ln = np.asarray(lengths, np.int64)
    off = np.zeros(len(ln) + 1, np.int64)
    np.cumsum(ln, out=off[1:])
    return ln, off


def _row_off(rows, skip=0):
    ro = np.full(len(rows) + 1, skip, np.int64)
    ro[1:] += np.cumsum([len(r) for r in rows])
    return ro


def _segs(rows):
    a = np.zeros(len(rows), SEG)
    for i, r in enumerate(rows):
        a[i] = tuple(r) + (0,)
    return a


def _as_bounds(raw):
    """int64 [rows, 5] as the library writes it -> BOUND_DTYPE [rows]"""
    return np.ascontiguousarray(raw).view(boundaries.BOUND_DTYPE).reshape(-1)


def _bounds(L, lengths, origins, tracks, rows, W, skip=0, wb=None, hits=True):
    """-> (rc, BOUND_DTYPE of the rows -- or the untouched sentinels --, dgrp_row_hits_batch's hits).  `skip` rows that no record
    owns lie in front (h_row_off[0] = skip): they are not read and their bounds are not written."""
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows, skip)
    junk = np.zeros(skip, SEG)
    junk["start"], junk["label"] = -5, 0
    flat = np.concatenate([junk] + list(rows))
    d_rows, d_track = _dev(flat.view(np.uint8)), _dev(np.concatenate(tracks).astype(np.int8))
    nrows = len(flat) - skip
    need = int(L.dgrp_row_bounds_workspace_bytes(len(ln), nrows))
    wb = need if wb is None else wb
    work = torch.full((max(need, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    d_b = torch.full((len(flat) + 2, 5), SENTINEL, dtype=torch.int64, device="cuda")
    rc = L.dgrp_row_bounds_batch(d_track.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro), W,
                                 d_b[1:].data_ptr(), work.data_ptr(), wb, _stream())
    torch.cuda.synchronize()
    whole = d_b.cpu().numpy()
    assert (whole[:1 + skip] == SENTINEL).all() and (whole[-1] == SENTINEL).all()
    got = _as_bounds(whole[1 + skip:-1])
    h = None
    if hits and rc == 0:
        d_hits = torch.zeros(len(flat), dtype=torch.int64, device="cuda")
        assert L.dgrp_row_hits_batch(d_track.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro),
                                     d_hits.data_ptr(), work.data_ptr(), need, _stream()) == 0, last_error()
        h = d_hits.cpu().numpy()[skip:]
    return rc, got, h


def _check(L, lengths, origins, tracks, rows, W, skip=0):
    rc, got, hits = _bounds(L, lengths, origins, tracks, rows, W, skip)
    assert rc == 0, last_error()
    want = boundaries.reference_bounds(origins, lengths, tracks, rows, W)
    for k in boundaries.BOUND_DTYPE.names:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} (W = {W}, records {lengths})")
    np.testing.assert_array_equal(got["hits"], hits)
    return got


# ================================================================================================ the worlds
def _tracks(rng, lengths, labels):
    """One buffer of runs of 1..12 bases of 0 and `labels`, cut into the records: the runs cross the borders, and the three bases on
    either side of every border hold one label, so that a flank which leaves its record finds what it looks for."""
    n = int(sum(lengths))
    t = np.zeros(n, np.int8)
    i = 0
    while i < n:
        k = int(rng.integers(1, 13))
        t[i:i + k] = int(rng.choice((0,) + tuple(labels)))
        i += k
    at = np.cumsum(lengths)[:-1]
    border = []
    for j, b in enumerate(at):
        lab = labels[j % len(labels)]
        t[max(b - 3, 0):b + 3] = lab
        border.append(lab)
    return np.split(t, at), border


def _rows(rng, o, n, t, labels, before=None, behind=None, extra=24):
    lab = lambda: int(labels[int(rng.integers(0, len(labels)))])
    first, last = int(t[0]) or lab(), int(t[-1]) or lab()
    q = [(o, o + 1, first), (o + n - 1, o + n, last),                              # the first and the last base
         (max(o - 2, 0), o + 1, first), (o + n - 1, o + n + 2, last),               # the same, clipped by the record
         (max(o - 5, 0), o + n + 5, lab()), (max(o - 5, 0), o + (n + 1) // 2, first), (o + n // 2, o + n + 9, last),   # sticking out
         (o + n + 10, o + n + 20, lab()), (0, max(o - 1, 0), lab()),                # wholly outside
         (o + 1, o + 1, lab()), (o, o, lab()), (o + n, o + n, lab()),               # empty
         (o + n // 4, o + 3 * n // 4 + 1, labels[0]), (o + n // 3, o + n // 2 + 1, labels[0]),        # nested
         (o + n // 3, o + n // 2 + 1, labels[0]), (o + n // 3, o + n // 2 + 1, labels[-1]),            # equal, and equal with another label
         (o + n // 2, o + n, labels[0]), (o, o + n, labels[-1])]                    # overlapping; the whole record
    if before is not None:                                                        # the label the record in front ends with, from the first base
        q += [(o, o + min(3, n), before), (o, o + 1, before)]
    if behind is not None:                                                        # the label the record behind begins with, to the last base
        q += [(o + max(n - 3, 0), o + n, behind), (o + n - 1, o + n, behind)]
    for _ in range(extra):
        a = int(rng.integers(max(o - 3, 0), o + n + 3))
        q.append((a, a + int(rng.integers(0, min(n, 400) + 4) if rng.random() < 0.5 else rng.integers(0, 14)), lab()))     # long ones, and short ones that are found
    return _segs([q[k] for k in rng.permutation(len(q))])


def _world(seed, lengths, labels=(1, 63, 127), extra=24):
    rng = np.random.default_rng(seed)
    origins = [int(rng.integers(0, 5000)) if r % 2 == 0 else 0 for r in range(len(lengths))]
    tracks, border = _tracks(rng, lengths, labels)
    rows = [_rows(rng, o, n, t, labels, border[r - 1] if r else None, border[r] if r + 1 < len(lengths) else None, extra)
            for r, (o, n, t) in enumerate(zip(origins, lengths, tracks))]
    return origins, tracks, rows


WORLDS = [[1], [2], [63], [64], [65], [8193], [64, 65], [1, 2, 1], [65, 8193, 300]]


@pytest.mark.parametrize("W", [0, 1, 64, 200, 4096])
@pytest.mark.parametrize("lengths", WORLDS, ids=str)
def test_bounds_equal_the_statement_and_the_hits(L, lengths, W):
    origins, tracks, rows = _world(sum(lengths) + len(lengths), lengths)
    got = _check(L, lengths, origins, tracks, rows, W)
    assert {int(x) for r in rows for x in r["label"]} >= {1, 63, 127}
    if len(lengths) > 1 and W > 0:
        # rows that end at a border whose other side holds their label: the flank stops at the record's end
        at = 0
        for r, (o, n, q) in enumerate(zip(origins, lengths, rows)):
            ends_here = np.flatnonzero((q["end"] >= o + n) & (q["start"] < o + n))
            starts_here = np.flatnonzero((q["start"] <= o) & (q["end"] > o))
            assert (got["trail"][at + ends_here] == 0).all() and (got["lead"][at + starts_here] == 0).all()
            at += len(q)
    if sum(lengths) > 100 and W > 0:
        assert (got["lead"] > 0).any() and (got["trail"] > 0).any() and (got["runs"] > 1).any() and (got["hits"] == 0).any()


def test_rows_in_front_that_no_record_owns_are_not_read(L):
    lengths = [65, 300]
    origins, tracks, rows = _world(5, lengths)
    _check(L, lengths, origins, tracks, rows, 64, skip=3)


def test_no_row_with_a_base_inside_its_record(L):
    """The pass has no position to walk: the two one-lane-per-row kernels alone write the outputs."""
    t = np.ones(70, np.int8)
    rows = [_segs([(0, 90, 1), (170, 400, 1), (120, 120, 1), (100, 100, 1), (170, 170, 1)])]
    got = _check(L, [70], [100], [t], rows, 64)
    assert not got["hits"].any() and not got["runs"].any() and not got["lead"].any() and not got["trail"].any()
    assert (got["first"] == -1).all() and (got["last"] == -1).all()


@pytest.mark.parametrize("kind", ["alternating", "all_equal"])
def test_one_row_of_100000_bases(L, kind):
    m, flank, o = 100_000, 150, 7
    n = m + 2 * flank
    t = (np.arange(n) % 2).astype(np.int8) if kind == "alternating" else np.ones(n, np.int8)
    rows = [_segs([(o + flank, o + flank + m, 1), (o + flank + 1, o + flank + m, 1)])]
    got = _check(L, [n], [o], [t], rows, 200)
    if kind == "alternating":
        assert got["runs"].tolist() == [m // 2, m // 2] and got["hits"].tolist() == [m // 2, m // 2]
        assert got["lead"].tolist() == [1, 0] and got["trail"].tolist() == [0, 0]
        assert got["first"].tolist() == [o + flank + 1] * 2 and got["last"].tolist() == [o + flank + m - 1] * 2
    else:
        assert got["runs"].tolist() == [1, 1] and got["hits"].tolist() == [m, m - 1]
        assert got["lead"].tolist() == [flank, flank + 1] and got["trail"].tolist() == [flank, flank]       # the record ends there, below W


@pytest.mark.parametrize("W,shift", [(0, 0), (0, 3), (5, 5), (200, 1000)])
def test_a_run_that_begins_at_a_slice_edge_and_one_that_straddles_it(L, W, shift):
    """Row 0 is [shift, n) with shift >= W: base b sits at position W + b - shift of the line."""
    n = 3 * SLICE + shift + 100
    at = lambda p: p - W + shift                                          # the base at line position p
    t = np.zeros(n, np.int8)
    t[at(SLICE):at(SLICE) + 9] = 1                                        # begins exactly at the second slice
    t[at(2 * SLICE) - 4:at(2 * SLICE) + 6] = 1                            # straddles the third
    t[at(3 * SLICE) - 1] = 1                                              # the last position of a slice, alone
    rows = [_segs([(shift, n, 1), (shift, n, 2), (at(2 * SLICE), at(2 * SLICE) + 1, 1)])]
    got = _check(L, [n], [0], [t], rows, W)
    assert got["runs"].tolist() == [3, 0, 1] and got["hits"].tolist() == [20, 0, 1]
    assert got["first"][0] == at(SLICE) and got["last"][0] == at(3 * SLICE) - 1
    assert got["lead"].tolist() == [0, 0, min(W, 4)] and got["trail"].tolist() == [0, 0, min(W, 5)]


@pytest.mark.parametrize("W", [0, 1, 64])
def test_5000_one_base_rows(L, W):
    """W = 0 and 1: a slice of 8192 positions holds more rows than the LDS table; W = 64: it holds 63."""
    rng = np.random.default_rng(W)
    n, o, count = 6000, 11, 5000
    assert SLICE // (1 + 2 * W) > LDS_ROWS or W == 64
    t = rng.integers(0, 4, n).astype(np.int8)
    t[1000:1200] = 2                                                       # long flanks for some
    q = np.zeros(count, SEG)
    q["start"] = o + 500 + np.arange(count)
    q["end"] = q["start"] + 1
    q["label"] = rng.integers(1, 4, count)
    q["label"][500:700] = 2
    got = _check(L, [n], [o], [t], [q[rng.permutation(count)]], W)
    assert (got["hits"] == 1).sum() > 1000 and (got["hits"] == 0).sum() > 1000
    assert got["lead"].max() == W and got["trail"].max() == W and got["runs"].max() == 1


def test_refusals_leave_the_bounds_untouched(L):
    lengths = [300]
    origins, tracks, rows = _world(9, lengths)
    for bad in ((-1, 9, 1), (9, 5, 1), (5, 9, 0), (5, 9, 128)):
        spoiled = [rows[0].copy()]
        spoiled[0][len(spoiled[0]) // 2] = bad + (0,)
        rc, got, _h = _bounds(L, lengths, origins, tracks, spoiled, 64)
        assert rc == EINVAL and "dgrp_row_bounds_batch" in last_error() and "label" in last_error(), bad
        assert (got.view(np.int64) == SENTINEL).all()
    for W in (4097, -1, 1 << 20):
        rc, got, _h = _bounds(L, lengths, origins, tracks, rows, W)
        assert rc == EINVAL and "W" in last_error() and (got.view(np.int64) == SENTINEL).all()
    need = int(L.dgrp_row_bounds_workspace_bytes(1, len(rows[0])))
    rc, got, _h = _bounds(L, lengths, origins, tracks, rows, 64, wb=need - 1)
    assert rc == ENOMEM and "workspace" in last_error() and (got.view(np.int64) == SENTINEL).all()
    rc, got, _h = _bounds(L, lengths, origins, tracks, [rows[0][:0]], 64)            # no rows: no device work
    assert rc == 0 and len(got) == 0


def test_two_calls_give_the_same_bytes(L):
    lengths = [65, 8193, 300]
    origins, tracks, rows = _world(21, lengths, extra=400)
    a = _bounds(L, lengths, origins, tracks, rows, 200, hits=False)
    b = _bounds(L, lengths, origins, tracks, rows, 200, hits=False)
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes()


# ================================================================================================ the tables
def _hist(L, lengths, origins, rows, bounds, need, C, W, wb=None):
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    flat = np.concatenate(rows)
    d_rows, d_b, d_need = _dev(flat.view(np.uint8)), _dev(bounds.view(np.int64).reshape(-1, 5)), _dev(np.asarray(need, np.int64))
    E = 2 * W + 1
    d_frag = torch.full((C * 17 + 2,), 5, dtype=torch.int64, device="cuda")
    d_edge = torch.full((C * 2 * E + 2,), 6, dtype=torch.int64, device="cuda")
    d_tally = torch.full((C * 2 + 2,), 7, dtype=torch.int64, device="cuda")
    d_bad = torch.full((3,), 9, dtype=torch.int32, device="cuda")
    need_wb = int(L.dgrp_bound_hist_workspace_bytes(len(ln)))
    wb = need_wb if wb is None else wb
    work = torch.full((max(need_wb, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.dgrp_bound_hist_batch(len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro), d_b.data_ptr(), d_need.data_ptr(),
                                 C, W, d_frag[1:].data_ptr(), d_edge[1:].data_ptr(), d_tally[1:].data_ptr(), d_bad[1:].data_ptr(),
                                 work.data_ptr(), wb, _stream())
    torch.cuda.synchronize()
    f, e, t, b = d_frag.cpu().numpy(), d_edge.cpu().numpy(), d_tally.cpu().numpy(), d_bad.cpu().numpy()
    assert f[0] == f[-1] == 5 and e[0] == e[-1] == 6 and t[0] == t[-1] == 7 and b[0] == b[2] == 9
    return rc, f[1:-1].reshape(C, 17), e[1:-1].reshape(C, 2, E), t[1:-1].reshape(C, 2), int(b[1])


def _hist_world(C, W, seed, labels=None):
    lengths = [65, 8193, 300]
    labels = labels or sorted({1, max(C // 2, 1), C - 1})
    origins, tracks, rows = _world(seed, lengths, tuple(labels), extra=700)
    bounds = boundaries.reference_bounds(origins, lengths, tracks, rows, W)
    clen = np.concatenate([np.maximum(np.clip(q["end"], o, o + n) - np.clip(q["start"], o, o + n), 0) for q, o, n in zip(rows, origins, lengths)])
    need = need_of(0.5, clen)
    need[::7] = 0                                                           # need 0: never found
    return lengths, origins, rows, bounds, need


@pytest.mark.parametrize("W", [0, 1, 200, 4096])
@pytest.mark.parametrize("C", [2, 5, 64])
def test_tables_equal_the_statement(L, C, W):
    lengths, origins, rows, bounds, need = _hist_world(C, W, 10 * C + W % 7)
    rc, frag, edge, tally, flag = _hist(L, lengths, origins, rows, bounds, need, C, W)
    assert rc == 0, last_error()
    want = boundaries.reference_bound_hist(origins, lengths, rows, bounds, need, C, W)
    for g, w, name in zip((frag, edge, tally), want[:3], ("frag", "edge", "tally")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert flag == want[3] == 0
    found = int(tally[:, 0].sum())
    assert found > 50 and frag.sum() > found                                # rows that are not found
    assert 0 < edge[:, 0].sum() < found and 0 < edge[:, 1].sum() < found    # sides the record clipped
    assert frag[0].sum() == 0 and (frag.sum(axis=1) > 0).sum() == len({1, max(C // 2, 1), C - 1})
    if W:
        assert edge[:, :, :W].sum() > 0 and edge[:, :, W + 1:].sum() > 0 and edge[:, :, W].sum() > 0


def test_a_label_beyond_the_classes_sets_the_flag_and_is_not_counted(L):
    C, W = 3, 64
    lengths, origins, rows, bounds, need = _hist_world(C, W, 77, labels=[1, 2, 3, 100])
    rc, frag, edge, tally, flag = _hist(L, lengths, origins, rows, bounds, need, C, W)
    want = boundaries.reference_bound_hist(origins, lengths, rows, bounds, need, C, W)
    assert rc == 0 and flag == want[3] == 1
    for g, w in zip((frag, edge, tally), want[:3]):
        np.testing.assert_array_equal(g, w)
    inside = sum(int(((np.clip(q["end"], o, o + n) > np.clip(q["start"], o, o + n)) & (q["label"] < C)).sum()) for q, o, n in zip(rows, origins, lengths))
    assert frag.sum() == inside


def test_the_tables_are_zeroed_where_nothing_is_counted_and_refusals(L):
    lengths, origins, rows, bounds, need = _hist_world(5, 10, 3)
    none = [q[:0] for q in rows]
    rc, frag, edge, tally, flag = _hist(L, lengths, origins, none, bounds[:0], need[:0], 5, 10)      # outputs that held 5, 6, 7 and 9
    assert rc == 0 and not frag.any() and not edge.any() and not tally.any() and flag == 0
    rc, frag, edge, tally, flag = _hist(L, lengths, origins, rows, bounds, np.zeros_like(need), 5, 10)
    assert rc == 0 and frag.sum() > 0 and not edge.any() and not tally.any() and flag == 0           # need 0 everywhere: nothing is found
    d1 = torch.zeros(64, dtype=torch.int64, device="cuda")
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    args = lambda C, W, wb: (len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d1.data_ptr(), i64ptr(ro), d1.data_ptr(), d1.data_ptr(), C, W,
                             d1.data_ptr(), d1.data_ptr(), d1.data_ptr(), d1.data_ptr(), d1.data_ptr(), wb, _stream())
    for C, W in ((1, 10), (65, 10), (5, -1), (5, 4097)):
        assert L.dgrp_bound_hist_batch(*args(C, W, 1 << 20)) == EINVAL and "dgrp_bound_hist_batch" in last_error()
    rc = _hist(L, lengths, origins, rows, bounds, need, 5, 10, wb=int(L.dgrp_bound_hist_workspace_bytes(3)) - 1)[0]
    assert rc == ENOMEM and "workspace" in last_error()


def test_both_entries_in_a_row_equal_both_statements(L):
    """As `evaluate` calls them: the second reads what the first wrote on the device."""
    lengths, W, C = [65, 8193, 300], 200, 5
    origins, tracks, rows = _world(31, lengths, (1, 2, 4), extra=300)
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    flat = np.concatenate(rows)
    clen = np.concatenate([np.maximum(np.clip(q["end"], o, o + n) - np.clip(q["start"], o, o + n), 0) for q, o, n in zip(rows, origins, lengths)])
    need = need_of(0.5, clen)
    d_rows, d_track, d_need = _dev(flat.view(np.uint8)), _dev(np.concatenate(tracks)), _dev(need)
    wb = max(int(L.dgrp_row_bounds_workspace_bytes(3, len(flat))), int(L.dgrp_bound_hist_workspace_bytes(3)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    d_b = torch.empty((len(flat), 5), dtype=torch.int64, device="cuda")
    d_frag, d_edge = torch.empty((C, 17), dtype=torch.int64, device="cuda"), torch.empty((C, 2, 2 * W + 1), dtype=torch.int64, device="cuda")
    d_tally, d_bad = torch.empty((C, 2), dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    assert L.dgrp_row_bounds_batch(d_track.data_ptr(), 3, i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro), W, d_b.data_ptr(),
                                   work.data_ptr(), wb, _stream()) == 0, last_error()
    assert L.dgrp_bound_hist_batch(3, i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(ro), d_b.data_ptr(), d_need.data_ptr(), C, W,
                                   d_frag.data_ptr(), d_edge.data_ptr(), d_tally.data_ptr(), d_bad.data_ptr(), work.data_ptr(), wb, _stream()) == 0, last_error()
    bounds = boundaries.reference_bounds(origins, lengths, tracks, rows, W)
    want = boundaries.reference_bound_hist(origins, lengths, rows, bounds, need, C, W)
    assert _as_bounds(d_b.cpu().numpy()).tobytes() == bounds.tobytes()
    for g, w in zip((d_frag, d_edge, d_tally), want[:3]):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    assert int(d_bad.item()) == 0


# ================================================================================================ stream order
@pytest.mark.parametrize("fill", [0xA5, 0xFF], ids=lambda f: f"fill{f:02X}")
def test_bounds_synchronise_once_and_are_stream_ordered_behind_it(H, L, fill):
    lengths, W = [65, 8193], 64
    origins, tracks, rows = _world(6, lengths, (1, 2, 3))
    flat, track = np.concatenate(rows), np.concatenate(tracks)
    p_flat = flat.copy()
    p_flat["start"], p_flat["end"], p_flat["label"] = 0, 10 ** 6, 1
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    wb = int(L.dgrp_row_bounds_workspace_bytes(2, len(flat)))
    call = lambda b, w, s, t: (L.dgrp_row_bounds_batch(b["track"].data_ptr(), 2, i64ptr(t["off"]), i64ptr(t["ln"]), i64ptr(t["org"]), b["rows"].data_ptr(),
                                                       i64ptr(t["ro"]), W, b["bounds"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"rows": (flat.view(np.uint8), p_flat.view(np.uint8)), "track": (track, np.where(track == 1, 2, 1).astype(np.int8))},
                     {"bounds": np.full((len(flat), 5), SENTINEL, np.int64)}, work_bytes=wb, fill=fill, sync=True, drained=False,
                     tables={"off": off, "ln": ln, "org": org, "ro": ro})
    assert _as_bounds(late["bounds"]).tobytes() == boundaries.reference_bounds(origins, lengths, tracks, rows, W).tobytes()


@pytest.mark.parametrize("W", [64, 4096])
def test_tables_are_stream_ordered(H, L, W):
    C = 5
    lengths, origins, rows, bounds, need = _hist_world(C, W, 12)
    flat = np.concatenate(rows)
    p_flat = flat.copy()
    p_flat["label"] = np.where(flat["label"] == 1, 2, 1)
    raw = bounds.view(np.int64).reshape(-1, 5)
    p_raw = raw.copy()
    p_raw[:, 1] += 1                                                        # one run more for every row
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    wb = int(L.dgrp_bound_hist_workspace_bytes(3))
    call = lambda b, w, s, t: (L.dgrp_bound_hist_batch(3, i64ptr(t["off"]), i64ptr(t["ln"]), i64ptr(t["org"]), b["rows"].data_ptr(), i64ptr(t["ro"]),
                                                       b["bounds"].data_ptr(), b["need"].data_ptr(), C, W, b["frag"].data_ptr(), b["edge"].data_ptr(),
                                                       b["tally"].data_ptr(), b["bad"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"rows": (flat.view(np.uint8), p_flat.view(np.uint8)), "bounds": (raw, p_raw), "need": (need, need + 1)},
                     {"frag": np.full((C, 17), 5, np.int64), "edge": np.full((C, 2, 2 * W + 1), 6, np.int64), "tally": np.full((C, 2), 7, np.int64),
                      "bad": np.full(1, 9, np.int32)}, work_bytes=wb, tables={"off": off, "ln": ln, "org": org, "ro": ro})
    want = boundaries.reference_bound_hist(origins, lengths, rows, bounds, need, C, W)
    for k, w in zip(("frag", "edge", "tally"), want[:3]):
        np.testing.assert_array_equal(late[k], w, err_msg=k)
    assert late["bad"][0] == 0
