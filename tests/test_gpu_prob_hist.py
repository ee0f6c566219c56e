"""dgrp_prob_hist_batch against curves.reference_hist, bit for bit (every count is an integer): class counts and bin counts either side
of the kernel's LDS grouping, records of 0 to 4097 bases at rows padded to multiples of 64 (as run_batch_probs pads them) with 0.75 in
the padding so that a reader that strays shows, truth bytes back to back; value families (uniform, all 0, all 1, every bin edge with
both float32 neighbours, denormals, -0.0, 70 000 elements in one cell, a trained-model-like mix); the flag; a side stream; two calls;
sentinel pages around the histogram and the workspace.  About 600 000 bases in all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import Arena                                           # noqa: E402
from stream_harness import i64ptr, last_error                           # noqa: E402

EINVAL = -1
PAD = np.float32(0.75)
SIX = [0, 1, 63, 64, 65, 4097]


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _lengths(nrec):
    if nrec == 1:
        return [4097]
    if nrec == 3:
        return [0, 4097, 63]
    return [SIX[(r * 5 + 1) % 6] for r in range(nrec)]                  # 40 records: every length of SIX, several times, mixed


def _layout(lengths, C, values, truth, lead=11):
    """values [sum(lengths), C] and truth [sum(lengths)] laid out as a batch: -> (probs with padded rows, row0, truth buffer with `lead`
    foreign bytes in front, off)."""
    ln = np.asarray(lengths, np.int64)
    row0 = np.zeros(len(ln), np.int64)
    if len(ln):
        np.cumsum((ln[:-1] + 63) // 64 * 64, out=row0[1:])
    rows = int(((ln + 63) // 64 * 64).sum()) if len(ln) else 0
    probs = np.full((rows + 1, C), PAD, np.float32)
    off = lead + np.r_[0, np.cumsum(ln)[:-1]].astype(np.int64) if len(ln) else np.zeros(0, np.int64)
    at = 0
    for r, n in enumerate(ln):
        probs[row0[r]:row0[r] + n] = values[at:at + n]
        at += int(n)
    tbuf = np.concatenate([np.full(lead, 77, np.int8), np.asarray(truth, np.int8), np.full(5, 77, np.int8)])
    return probs, row0, tbuf, off


def _run(L, dev, probs, row0, lengths, tbuf, off, bins, extra_work=0, arenas=None):
    """One call on the current stream: -> (rc, hist [C, 2, bins], flag, (hist arena, work arena))."""
    C = probs.shape[1]
    ln = np.ascontiguousarray(lengths, np.int64)
    d_probs = torch.from_numpy(probs).to(dev)
    d_truth = torch.from_numpy(tbuf).to(dev)
    wb = int(L.dgrp_prob_hist_workspace_bytes(len(ln), C, bins)) + extra_work
    assert wb > 0
    hist, work = arenas or (Arena(C * 2 * bins * 8), Arena(wb))
    d_bad = torch.full((3,), 7, dtype=torch.int32, device=dev)
    rc = L.dgrp_prob_hist_batch(d_probs.data_ptr(), C, len(ln), i64ptr(row0), i64ptr(ln), d_truth.data_ptr(), i64ptr(off), bins, hist.ptr,
                                d_bad[1:].data_ptr(), work.ptr, wb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    bad = d_bad.cpu().numpy()
    assert bad[0] == 7 and bad[2] == 7
    assert np.array_equal(d_probs.cpu().numpy(), probs, equal_nan=True) and np.array_equal(d_truth.cpu().numpy(), tbuf)
    return rc, hist.body().cpu().numpy().view(np.int64).reshape(C, 2, bins).copy(), int(bad[1]), (hist, work)


def _check(L, dev, lengths, C, bins, values, truth, flag=0, **kw):
    from deepgrp_amd.curves import reference_hist
    want, want_flag = reference_hist(values, truth, bins)
    assert want_flag == flag
    probs, row0, tbuf, off = _layout(lengths, C, values, truth)
    rc, got, bad, arenas = _run(L, dev, probs, row0, lengths, tbuf, off, bins, **kw)
    assert rc == 0, last_error()
    assert bad == flag
    np.testing.assert_array_equal(got, want)
    assert all(a.guards_intact() for a in arenas)
    if not flag:
        assert (got.sum(axis=(1, 2)) == len(truth)).all()
    return got


def _uniform(n, C, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, C), dtype=np.float32), rng.integers(0, C, n).astype(np.int8)


def _group(C, bins):
    """The classes of one workgroup, as include/deepgrp_hip.h states the rule."""
    g = C
    while g > 1 and g * (8 * bins + 512) + 4096 > 163840:
        g -= 1
    return g


def test_the_grouping_rule_the_shapes_below_straddle():
    assert _group(18, 1000) == 18 and _group(19, 1000) == 18 and _group(4, 4096) == 4 and _group(5, 4096) == 4
    assert _group(64, 4096) == 4 and _group(64, 2) == 64 and _group(16, 1000) == 16


# C = 5 / 1000 (the model's), 64 / 4096 (sixteen groups), 17 / 2 (one group, two bins), 18 / 1000 and 4 / 4096 (the largest single
# groups), 19 / 1000 and 5 / 4096 (the first that are cut: groups of 18 + 1 and 4 + 1), 17 / 4096 (a last group of one class)
@pytest.mark.parametrize("C,bins,nrec", [(5, 1000, 1), (5, 1000, 3), (5, 1000, 40), (2, 2, 3), (2, 1000, 40), (2, 4096, 1), (16, 1000, 3),
                                         (16, 4096, 40), (17, 2, 40), (17, 4096, 3), (18, 1000, 40), (19, 1000, 3), (4, 4096, 3),
                                         (5, 4096, 40), (64, 2, 3), (64, 1000, 1), (64, 4096, 3)])
def test_uniform_bit_for_bit(L, dev, C, bins, nrec):
    lengths = _lengths(nrec)
    values, truth = _uniform(sum(lengths), C, 1000 * C + bins + nrec)
    _check(L, dev, lengths, C, bins, values, truth)


def _edges(bins):
    """j / bins and both float32 neighbours for every j, those inside [0, 1]."""
    j = np.arange(bins + 1, dtype=np.float64)
    mid = (j / bins).astype(np.float32)
    v = np.concatenate([np.nextafter(mid, np.float32(-1)), mid, np.nextafter(mid, np.float32(2))])
    return v[(v >= 0) & (v <= 1)]


def _family(name, C, bins):
    """-> (lengths, values, truth)"""
    rng = np.random.default_rng(sum(map(ord, name)) + bins)
    if name == "edges":
        v = _edges(bins)
        n = max(-(-v.size * 2 // C), 200)
        values = np.resize(v, n * C).reshape(n, C)                      # every edge value twice, in shifting columns
        return [n - 70, 70], values, rng.integers(0, C, n).astype(np.int8)
    if name == "hot":
        n = 70_000                                                      # more than any 16-bit counter holds, in one cell per class
        values = np.zeros((n, C), np.float32)
        values[:, 2 % C] = 0.5
        return [n], values, np.full(n, 2 % C, np.int8)
    n = 9000
    truth = rng.integers(0, C, n).astype(np.int8)
    if name == "zeros":
        values = np.zeros((n, C), np.float32)
    elif name == "ones":
        values = np.ones((n, C), np.float32)
    elif name == "negative_zero":
        values = np.full((n, C), -0.0, np.float32)
    elif name == "denormals":
        values = (rng.integers(1, 1 << 23, (n, C)).astype(np.uint32)).view(np.float32)
        assert (values > 0).all() and (values < np.finfo(np.float32).tiny).all()
    elif name == "trained":
        # 98 % within 1e-4 of 0 or 1, the class of the truth mostly near 1; the rest uniform
        near = rng.random((n, C), dtype=np.float32) * np.float32(1e-4)
        values = near.copy()
        call = np.where(rng.random(n) < 0.9, truth, rng.integers(0, C, n))
        values[np.arange(n), call] = np.float32(1) - near[np.arange(n), call]
        loose = rng.random((n, C)) < 0.02
        values[loose] = rng.random(int(loose.sum()), dtype=np.float32)
        assert values.min() >= 0 and values.max() <= 1
    else:
        raise KeyError(name)
    return [4097, 0, n - 4097 - 65, 65], values, truth


@pytest.mark.parametrize("name,C,bins", [("zeros", 5, 1000), ("ones", 5, 1000), ("negative_zero", 5, 1000), ("denormals", 5, 1000),
                                         ("trained", 5, 1000), ("trained", 16, 1000), ("trained", 64, 4096), ("hot", 5, 1000),
                                         ("hot", 2, 2), ("hot", 19, 1000), ("edges", 5, 2), ("edges", 5, 1000), ("edges", 5, 4096),
                                         ("edges", 3, 1000), ("edges", 64, 4096), ("zeros", 2, 2), ("ones", 64, 4096)])
def test_value_families_bit_for_bit(L, dev, name, C, bins):
    lengths, values, truth = _family(name, C, bins)
    got = _check(L, dev, lengths, C, bins, values, truth)
    if name in ("zeros", "negative_zero", "denormals"):
        assert (got[:, :, 1:] == 0).all()
    if name == "ones":
        assert (got[:, :, :-1] == 0).all()
    if name == "hot":
        assert got[2 % C, 1, bins // 2] == 70_000 and got[2 % C, 0].sum() == 0


FLAGS = {"nan": ("p", np.nan), "above_one": ("p", np.nextafter(np.float32(1), np.float32(2))), "negative": ("p", -1e-30),
         "truth_C": ("t", None), "truth_minus_one": ("t", -1)}


@pytest.mark.parametrize("what", sorted(FLAGS))
@pytest.mark.parametrize("C,bins", [(5, 1000), (19, 1000)])
def test_one_bad_value_sets_the_flag_and_is_left_out(L, dev, what, C, bins):
    lengths = [4097, 903]
    values, truth = _uniform(5000, C, 7)
    kind, v = FLAGS[what]
    if kind == "p":
        values[4500, C - 1] = v
    else:
        truth[4500] = C if v is None else v
    got = _check(L, dev, lengths, C, bins, values, truth, flag=1)
    assert got.sum() == 5000 * C - (1 if kind == "p" else C)


def test_side_stream_two_calls_and_a_larger_workspace(L, dev):
    C, bins, lengths = 5, 1000, _lengths(40)
    values, truth = _uniform(sum(lengths), C, 99)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        first = _check(L, dev, lengths, C, bins, values, truth)
    # the same arenas again: the entry zeroes the histogram itself and gives the same bytes; then a smaller problem in this workspace
    probs, row0, tbuf, off = _layout(lengths, C, values, truth)
    rc, a, _bad, arenas = _run(L, dev, probs, row0, lengths, tbuf, off, bins, extra_work=4096)
    rc2, b, _bad, _ = _run(L, dev, probs, row0, lengths, tbuf, off, bins, extra_work=4096, arenas=arenas)
    assert rc == 0 and rc2 == 0, last_error()
    assert a.tobytes() == b.tobytes() == first.tobytes()
    from deepgrp_amd.curves import reference_hist
    few = 3
    rc3, c, bad, _ = _run(L, dev, probs, row0[:few], lengths[:few], tbuf, off[:few], bins,
                          extra_work=int(L.dgrp_prob_hist_workspace_bytes(40, C, bins)) - int(L.dgrp_prob_hist_workspace_bytes(few, C, bins)) + 4096,
                          arenas=arenas)
    assert rc3 == 0 and bad == 0
    n = sum(lengths[:few])
    np.testing.assert_array_equal(c, reference_hist(values[:n], truth[:n], bins)[0])
    assert all(x.guards_intact() for x in arenas)


@pytest.mark.parametrize("C,shift", [(5, 0), (5, 1), (3, 2), (1, 3), (7, 1), (64, 3)])
def test_records_at_any_row_and_an_array_off_the_16_byte_grid(L, dev, C, shift):
    """Rows that are not padded (a record starts where 16-byte vectors do not) and an array that starts `shift` floats behind a
    16-byte boundary: the elements in front of the first and behind the last whole vector of every tile are counted once."""
    from deepgrp_amd.curves import reference_hist
    bins, lengths = 1000, [1, 4097, 2, 3, 4099, 0, 5, 8195]
    row0 = np.cumsum([3] + [n + k % 3 for k, n in enumerate(lengths[:-1])]).astype(np.int64)       # gaps of 0, 1 or 2 rows
    values, truth = _uniform(sum(lengths), C, 31 + C)
    probs = np.full((int(row0[-1]) + lengths[-1] + 2, C), PAD, np.float32)
    at = 0
    for r, n in enumerate(lengths):
        probs[row0[r]:row0[r] + n] = values[at:at + n]
        at += n
    off = (9 + np.r_[0, np.cumsum(lengths)[:-1]]).astype(np.int64)
    tbuf = np.concatenate([np.full(9, 77, np.int8), truth, np.full(3, 77, np.int8)])
    flat = torch.from_numpy(np.concatenate([np.full(shift, PAD, np.float32), probs.ravel()])).to(dev)
    assert flat.data_ptr() % 16 == 0
    d_truth = torch.from_numpy(tbuf).to(dev)
    ln = np.asarray(lengths, np.int64)
    wb = int(L.dgrp_prob_hist_workspace_bytes(len(ln), C, bins))
    hist, work = Arena(C * 2 * bins * 8), Arena(wb)
    d_bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    rc = L.dgrp_prob_hist_batch(flat.data_ptr() + 4 * shift, C, len(ln), i64ptr(row0), i64ptr(ln), d_truth.data_ptr(), i64ptr(off), bins,
                                hist.ptr, d_bad.data_ptr(), work.ptr, wb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    got = hist.body().cpu().numpy().view(np.int64).reshape(C, 2, bins)
    np.testing.assert_array_equal(got, reference_hist(values, truth, bins)[0])
    assert int(d_bad.item()) == 0 and hist.guards_intact() and work.guards_intact()


def test_nothing_to_count_gives_zeros_without_device_arrays(L, dev):
    C, bins = 5, 10
    hist = Arena(C * 2 * bins * 8)
    d_bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    assert L.dgrp_prob_hist_batch(None, C, 0, None, None, None, None, bins, hist.ptr, d_bad.data_ptr(), None, 0, s) == 0, last_error()
    torch.cuda.synchronize()
    assert not hist.body().any() and int(d_bad.item()) == 0 and hist.guards_intact()
    hist.body().fill_(0xA5)
    d_bad.fill_(7)
    z = np.zeros(3, np.int64)
    assert L.dgrp_prob_hist_batch(None, C, 3, i64ptr(z), i64ptr(z), None, i64ptr(z), bins, hist.ptr, d_bad.data_ptr(), None, 0, s) == 0, last_error()
    torch.cuda.synchronize()
    assert not hist.body().any() and int(d_bad.item()) == 0 and hist.guards_intact()


def test_a_short_workspace_is_refused_before_anything_is_written(L, dev):
    C, bins, lengths = 5, 1000, [100]
    values, truth = _uniform(100, C, 3)
    probs, row0, tbuf, off = _layout(lengths, C, values, truth)
    hist, work = Arena(C * 2 * bins * 8), Arena(int(L.dgrp_prob_hist_workspace_bytes(1, C, bins)))
    d_probs, d_truth = torch.from_numpy(probs).to(dev), torch.from_numpy(tbuf).to(dev)
    d_bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ln = np.asarray(lengths, np.int64)
    rc = L.dgrp_prob_hist_batch(d_probs.data_ptr(), C, 1, i64ptr(row0), i64ptr(ln), d_truth.data_ptr(), i64ptr(off), bins, hist.ptr,
                                d_bad.data_ptr(), work.ptr, work.n - 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == EINVAL and "workspace too small" in last_error()
    assert hist.untouched() and work.untouched() and int(d_bad.item()) == 7
