"""gru_split2_kernel launches min(tile pairs, CUs) workgroups and each walks the pairs blockIdx.x, blockIdx.x + gridDim.x, ...
(weights and input table loaded once per workgroup, one set-up pass per pair).  Which workgroup runs a window, and after which other
windows, must not show in a single bit: every case here compares a launch in which workgroups walk with launches in which none does
(slices of at most G * 32 windows, G = the device's CU count = the largest grid), as int32 views, and pins both to the float64
statement at the 1e-5 the forward tests use.  Model: 128 units, T = 200, s = 50, 5 classes (the stored synthetic weights)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, S, NCLS = 200, 50, 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def grid(dev):
    """G: the grid the launcher uses for a launch of at least that many tile pairs"""
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.fixture(scope="module")
def weights():
    from deepgrp_amd import synthetic
    return synthetic.trained_weights()


@pytest.fixture(scope="module")
def model(dev, weights):
    from deepgrp_amd.pipeline import DeviceModel
    w = weights
    dm = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=T)
    assert [dm.plan(mode, S).kernel for mode in (0, 1)] == ["split2"] * 2
    yield dm
    dm.close()


def _bases(nwin):
    """the shortest record dgrp_window_count cuts into nwin windows (it counts the window starts in front of n - T)"""
    return T + S * (nwin - 1) + 1


def _record(nwin, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(5, size=_bases(nwin), p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)


@pytest.fixture(scope="module")
def long_record(dev, grid, model):
    """2 G 32 + 16 + 7 windows: workgroup 0 walks three pairs, the others two; the last pair is a full tile and one of 7 windows.
    -> (class indices on the host, on the device, window count, mode-1 rows of the whole record in ONE launch, the same windows in
    slices no workgroup walks in).  Computed once; the tests do not write to it."""
    nwin = 2 * grid * 32 + 16 + 7
    idx = _record(nwin, 11)
    d = torch.from_numpy(idx).to(dev)
    walked = model.forward_windows(d, S, 0, nwin)
    sliced = torch.cat([model.forward_windows(d, S, w0, min(grid * 32, nwin - w0)) for w0 in range(0, nwin, grid * 32)])
    return idx, d, nwin, walked, sliced


def _bits(t):
    return t.contiguous().view(torch.int32)


def _max_merge(rows, n, B, step):
    """merged [n, C] of window rows [nwin, T, C]: window w lands at row (w, or w + nfull r - nfull B in the short last batch) * step,
    as the reference's batch loop places it; rows past n are dropped; max is exact"""
    nwin, dev = rows.shape[0], rows.device
    nfull, r = divmod(nwin, B)
    w = torch.arange(nwin, device=dev, dtype=torch.int64)
    row0 = torch.where(w < nfull * B, w, w + (nfull * r - nfull * B)) * step
    at = (row0[:, None] + torch.arange(T, device=dev, dtype=torch.int64)[None, :]).reshape(-1)
    keep = at < n
    want = torch.zeros((n, NCLS), dtype=torch.float32, device=dev)
    want.index_reduce_(0, at[keep], rows.reshape(-1, NCLS)[keep], "amax", include_self=True)
    return want


def test_walk_equals_no_walk_bitwise(long_record):
    _idx, _d, nwin, walked, sliced = long_record
    assert walked.shape == sliced.shape == (nwin, T, NCLS)
    assert torch.equal(_bits(walked), _bits(sliced))
    assert bool(torch.isfinite(walked).all()) and float((walked.sum(dim=2) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("batch", ["one", 256], ids=["no-shift", "partial-last-batch"])
def test_merged_output_is_the_max_merge_of_the_window_rows(dev, model, long_record, batch):
    """Mode 0 (image in LDS, flushed per pair, the next pair's set-up zeroing it again) = the max over the mode-1 rows, placed where the
    reference's batch loop puts them: `one` batch for the whole record (no shift), and batches of 256 (the short last batch of 23
    windows lands at nfull * 23 * s: placement active, rows of the last pairs far from their neighbours')."""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import ContigPipeline
    _idx, d, nwin, walked, _sliced = long_record
    B = nwin if batch == "one" else int(batch)
    pipe = ContigPipeline(model, S, B, 50, 50, True)
    assert model.plan(0, S, handle=pipe.handle).kernel == "split2"
    got = pipe.merged(d)
    n = d.numel()
    assert lib().dgrp_window_count(n, T, S) == nwin
    want = _max_merge(walked, n, B, S)
    assert (batch == "one") == (nwin % B == 0)
    bad = (_bits(got) != _bits(want)).any(dim=1).nonzero().reshape(-1)
    if bad.numel():
        print(f"{bad.numel()} of {n} rows differ: first {int(bad[0])}, last {int(bad[-1])}")
    assert bad.numel() == 0
    pipe.close()


def _batch_alone(pipe, d_base, offs, lens, which):
    """merged probabilities and segment rows of a batched launch against the same records run alone"""
    rows, d_probs, row0 = pipe.run_batch_probs(d_base, offs, lens, [0] * len(lens), list(range(len(lens))))
    for r in which:
        o, n = offs[r], lens[r]
        alone = pipe.merged(d_base[o:o + n].clone())
        assert torch.equal(_bits(d_probs[int(row0[r]):int(row0[r]) + n]), _bits(alone)), r
        want = pipe.run_idx(d_base[o:o + n].clone(), 0, contig=r)
        np.testing.assert_array_equal(rows[rows["contig"] == r], want)


def test_batched_records_straddling_pairs(dev, model):
    """Records of 1, 33 and 70 windows in one launch: 1 + 3 + 5 tiles, so pair 0 holds the whole first record and the head of the
    second (two tiles of one workgroup in different records) and pair 2 the tail of the second and the head of the third.  Merged
    probabilities and segment rows of each record as when it runs alone."""
    from deepgrp_amd.pipeline import ContigPipeline
    lens = [_bases(k) for k in (1, 33, 70)]
    offs, pos = [], 3                                            # records at odd byte offsets: unaligned ends of the staged spans
    for n in lens:
        offs.append(pos)
        pos += n + 5
    base = _record((pos + 64) // S + 4, 23)
    d_base = torch.from_numpy(base).to(dev)
    pipe = ContigPipeline(model, S, 256, 50, 50, True)
    assert pipe.batchable() and model.plan(0, S, handle=pipe.handle).kernel == "split2"
    _batch_alone(pipe, d_base, offs, lens, range(3))
    pipe.close()


def test_batched_records_walked(dev, grid, model):
    """More tile pairs of short records than workgroups: a walking workgroup looks its record up again for every pair (3 tiles per
    record, so pairs alternate between lying inside a record and straddling two).  First, last and a few records between."""
    from deepgrp_amd.pipeline import ContigPipeline
    nrec = (2 * grid * 2 + 2) // 3 + 5                           # > 2 G pairs of tiles
    n = _bases(33)
    offs = [7 + r * (n + 3) for r in range(nrec)]
    base = _record((offs[-1] + n) // S + 4, 29)
    d_base = torch.from_numpy(base).to(dev)
    pipe = ContigPipeline(model, S, 256, 50, 50, True)
    assert 3 * nrec > 2 * 2 * grid
    _batch_alone(pipe, d_base, offs, [n] * nrec, [0, 1, nrec // 2, nrec - 2, nrec - 1])
    pipe.close()


def _oracle_weights(orc, w):
    return orc.Weights(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, T)


def test_one_pair_with_a_one_window_tile(dev, orc, model, weights):
    """17 windows: one pair, its second tile holds one window (the record has no more than these 17 to hold against float64)."""
    idx = _record(17, 31)
    got = model.forward_windows(torch.from_numpy(idx).to(dev), S, 0, 17).cpu().numpy()
    want = orc.nn_forward(idx, _oracle_weights(orc, weights), S, 0, 17, np.float64)
    err = float(np.abs(got - want).max())
    print(f"17 windows: max |dp| = {err:.3e}")
    assert err < 1e-5


def test_walked_pairs_against_float64(orc, grid, weights, long_record):
    """32 windows of the long record -- 11 of its first pair, 11 of a middle pair (the second one its workgroup walks), 10 of the last
    (both tiles: the full one and the 7-window one) -- against the float64 statement."""
    idx, _d, nwin, walked, _sliced = long_record
    w = _oracle_weights(orc, weights)
    npairs = (nwin + 31) // 32
    mid = grid + grid // 2
    assert grid <= mid < 2 * grid <= npairs - 1
    for w0, k in ((3, 11), (32 * mid + 10, 11), (32 * (npairs - 1) + 13, 10)):
        want = orc.nn_forward(idx, w, S, w0, k, np.float64)
        err = float(np.abs(walked[w0:w0 + k].cpu().numpy() - want).max())
        print(f"windows {w0}..{w0 + k - 1}: max |dp| = {err:.3e}")
        assert err < 1e-5
    assert 32 * (npairs - 1) + 13 + 10 == nwin


@pytest.mark.parametrize("step", [207, 208])
def test_span_and_row_staging_of_the_sequences(dev, orc, model, weights, step):
    """The set-up stages a tile's 16 windows as ONE span of 15 s + T class indices where span + 15 bytes of alignment fit the
    [16][208] bytes of the carve -- up to s = 207 at T = 200 -- and window by window beyond.  40 windows (a full pair and a
    half-filled tile) on either side of that threshold: float64 at 1e-5, merged rows = the max-merge of the window rows."""
    from deepgrp_amd.pipeline import ContigPipeline
    assert (15 * step + T + 15 <= 16 * 208) == (step == 207)
    nwin = 40
    rng = np.random.default_rng(step)
    idx = rng.choice(5, size=T + step * (nwin - 1) + 1, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)
    d = torch.from_numpy(idx).to(dev)
    assert model.plan(1, step).kernel == "split2"
    got = model.forward_windows(d, step, 0, nwin)
    err = float(np.abs(got.cpu().numpy() - orc.nn_forward(idx, _oracle_weights(orc, weights), step, 0, nwin, np.float64)).max())
    print(f"step {step}, {nwin} windows: max |dp| = {err:.3e}")
    assert err < 1e-5
    pipe = ContigPipeline(model, step, 16, 50, 50, True)
    assert model.plan(0, step, handle=pipe.handle).kernel == "split2"
    assert torch.equal(_bits(pipe.merged(d)), _bits(_max_merge(got, d.numel(), 16, step)))
    pipe.close()


def test_attention_prepass_spill_bitwise(dev, grid):
    """Mode 2 (the recurrent pre-pass of an attention model: avg[t] spilled as float32 [windows, T, 128], the first bytes of the
    caller's workspace) on the three-pair record: walked = sliced, bit for bit, and so are the probabilities behind the second kernel."""
    from deepgrp_amd import synthetic
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import DeviceModel, stream_ptr
    w = synthetic.synthetic_weights(128, NCLS, attention=True, seed=9, gain=2.0)
    dm = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], w["scale"], vecsize=T)
    assert dm.attention and dm.plan(2, S).kernel == "split2"
    nwin = 2 * grid * 32 + 16 + 7
    d = torch.from_numpy(_record(nwin, 37)).to(dev)

    def run(w0, nw):
        wb = lib().dgrp_forward_workspace_bytes(dm.handle, nw)
        work = torch.zeros(wb, dtype=torch.uint8, device=dev)
        probs = torch.empty((nw, T, NCLS), dtype=torch.float32, device=dev)
        check(lib().dgrp_forward_windows(dm.handle, d.data_ptr(), d.numel(), S, w0, nw, probs.data_ptr(), work.data_ptr(), wb, stream_ptr()),
              "dgrp_forward_windows")
        return work[:nw * T * 128 * 4].view(torch.int32), probs

    avg, probs = run(0, nwin)
    assert int((avg != 0).sum()) > avg.numel() // 2
    for w0 in range(0, nwin, grid * 32):
        nw = min(grid * 32, nwin - w0)
        a, p = run(w0, nw)
        assert torch.equal(a, avg[w0 * T * 128:(w0 + nw) * T * 128]), w0
        assert torch.equal(_bits(p), _bits(probs[w0:w0 + nw])), w0
    dm.close()
