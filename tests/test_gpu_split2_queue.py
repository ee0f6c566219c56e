"""gru_split2_kernel hands tile pairs out from a queue: workgroup b starts with pair b, every later pair is gridDim.x + the old value of
a counter that lives in the call's workspace and is zeroed on the launch's stream.  Which workgroup runs a pair must not show in a
single bit, and launches that run side by side or back to back must not see one another's counter.  As in test_gpu_split2_walk.py
every case compares a launch in which workgroups take pairs from the queue with launches in which none does (slices of at most G * 32
windows, G = the device's CU count = the largest grid: one pair per workgroup, nothing queued), as int32 views.  Model: the stored
128-unit weights, T = 200, s = 50, 5 classes."""
import threading

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
    """the shortest record dgrp_window_count cuts into nwin windows"""
    return T + S * (nwin - 1) + 1


def _record(nwin, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(5, size=_bases(nwin), p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sliced(model, d, nwin, step):
    """the same windows in launches of at most `step` <= G * 32 windows: as many workgroups as pairs, the queue hands nothing out"""
    return torch.cat([model.forward_windows(d, S, w0, min(step, nwin - w0)) for w0 in range(0, nwin, step)])


def _max_merge(rows, n, B, step):
    """merged [n, C] of window rows [nwin, T, C] as the reference's batch loop places them (the short last batch of r windows starts at
    row nfull r step); max is exact"""
    nwin, dev = rows.shape[0], rows.device
    nfull, r = divmod(nwin, B)
    w = torch.arange(nwin, device=dev, dtype=torch.int64)
    row0 = torch.where(w < nfull * B, w, w + (nfull * r - nfull * B)) * step
    at = (row0[:, None] + torch.arange(T, device=dev, dtype=torch.int64)[None, :]).reshape(-1)
    keep = at < n
    want = torch.zeros((n, NCLS), dtype=torch.float32, device=dev)
    want.index_reduce_(0, at[keep], rows.reshape(-1, NCLS)[keep], "amax", include_self=True)
    return want


WINDOW_COUNTS = {
    "three-pairs": lambda g: 2 * g * 32 + 16 + 7,     # some workgroups take three pairs; the last pair is a full tile and one of 7 windows
    "one-queued": lambda g: g * 32 + 16,              # exactly one pair in the queue, and it has a single tile
    "none-queued": lambda g: g * 32,                  # a pair per workgroup: nothing to hand out
}


@pytest.fixture(scope="module")
def records(dev, grid, model):
    """per window count: (class indices on the host, on the device, window count, mode-1 rows of ONE launch, the same windows in slices
    in which no workgroup takes a second pair).  Computed once; the tests do not write to it."""
    out = {}
    for k, (name, count) in enumerate(WINDOW_COUNTS.items()):
        nwin = count(grid)
        idx = _record(nwin, 41 + k)
        d = torch.from_numpy(idx).to(dev)
        queued = model.forward_windows(d, S, 0, nwin)
        sliced = _sliced(model, d, nwin, grid * 32 if nwin > grid * 32 else grid * 16)
        out[name] = (idx, d, nwin, queued, sliced)
    return out


@pytest.mark.parametrize("count", list(WINDOW_COUNTS))
def test_window_rows_bitwise(records, count):
    _idx, _d, nwin, queued, sliced = records[count]
    assert queued.shape == sliced.shape == (nwin, T, NCLS)
    assert torch.equal(_bits(queued), _bits(sliced))
    assert bool(torch.isfinite(queued).all()) and float((queued.sum(dim=2) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("count,batch", [("three-pairs", "one"), ("three-pairs", 256), ("one-queued", "one"), ("one-queued", 256),
                                         ("none-queued", "one")],
                         ids=["three-pairs-no-shift", "three-pairs-partial-last-batch", "one-queued-no-shift", "one-queued-partial-last-batch",
                              "none-queued-no-shift"])
def test_merged_output_bitwise(model, records, count, batch):
    """Mode 0 (the image in LDS, flushed per pair) = the max over the rows of launches without a queued pair, placed where the
    reference's batch loop puts them: one batch for the whole record, and batches of 256 (the short last batch lands elsewhere)."""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import ContigPipeline
    _idx, d, nwin, _queued, sliced = records[count]
    B = nwin if batch == "one" else int(batch)
    assert (batch == "one") == (nwin % B == 0)
    pipe = ContigPipeline(model, S, B, 50, 50, True)
    assert model.plan(0, S, handle=pipe.handle).kernel == "split2"
    got = pipe.merged(d)
    n = d.numel()
    assert lib().dgrp_window_count(n, T, S) == nwin
    bad = (_bits(got) != _bits(_max_merge(sliced, n, B, S))).any(dim=1).nonzero().reshape(-1)
    if bad.numel():
        print(f"{bad.numel()} of {n} rows differ: first {int(bad[0])}, last {int(bad[-1])}")
    assert bad.numel() == 0
    pipe.close()


def test_attention_prepass_spill_bitwise(dev, grid):
    """Mode 2 (avg[t] spilled as float32 [windows, T, 128] into the first bytes of the caller's workspace, the queue word behind the
    spill) on the three-pair record: queued = sliced, bit for bit, and so are the probabilities behind the second kernel."""
    from deepgrp_amd import synthetic
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import DeviceModel, stream_ptr
    w = synthetic.synthetic_weights(128, NCLS, attention=True, seed=13, gain=2.0)
    dm = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], w["scale"], vecsize=T)
    assert dm.attention and dm.plan(2, S).kernel == "split2"
    nwin = 2 * grid * 32 + 16 + 7
    d = torch.from_numpy(_record(nwin, 47)).to(dev)

    def run(w0, nw):
        wb = lib().dgrp_forward_workspace_bytes(dm.handle, nw)
        work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=dev)             # (a counter that is not zeroed starts here)
        probs = torch.empty((nw, T, NCLS), dtype=torch.float32, device=dev)
        check(lib().dgrp_forward_windows(dm.handle, d.data_ptr(), d.numel(), S, w0, nw, probs.data_ptr(), work.data_ptr(), wb, stream_ptr()),
              "dgrp_forward_windows")
        return work[:nw * T * 128 * 4].view(torch.int32), probs

    avg, probs = run(0, nwin)
    for w0 in range(0, nwin, grid * 32):
        nw = min(grid * 32, nwin - w0)
        a, p = run(w0, nw)
        assert torch.equal(a, avg[w0 * T * 128:(w0 + nw) * T * 128]), w0
        assert torch.equal(_bits(p), _bits(probs[w0:w0 + nw])), w0
    dm.close()


def test_batched_records_straddling_queued_pairs(dev, grid, model):
    """More tile pairs of short records than workgroups (3 tiles per record: pairs alternate between lying inside a record and
    straddling two), so pairs past the first G come out of the queue and look their record up again.  Merged probabilities and
    segment rows of the first, the last and a few records between as when each runs alone."""
    from deepgrp_amd.pipeline import ContigPipeline
    nrec = (2 * grid * 2 + 2) // 3 + 5
    n = _bases(33)
    offs = [7 + r * (n + 3) for r in range(nrec)]                # odd byte offsets: unaligned ends of the staged spans
    base = _record((offs[-1] + n) // S + 4, 53)
    d_base = torch.from_numpy(base).to(dev)
    pipe = ContigPipeline(model, S, 256, 50, 50, True)
    assert pipe.batchable() and model.plan(0, S, handle=pipe.handle).kernel == "split2"
    assert 3 * nrec > 2 * 2 * grid
    rows, d_probs, row0 = pipe.run_batch_probs(d_base, offs, [n] * nrec, [0] * nrec, list(range(nrec)))
    for r in (0, 1, nrec // 2, 2 * nrec // 3, nrec - 2, nrec - 1):
        o = offs[r]
        alone = pipe.merged(d_base[o:o + n].clone())
        assert torch.equal(_bits(d_probs[int(row0[r]):int(row0[r]) + n]), _bits(alone)), r
        want = pipe.run_idx(d_base[o:o + n].clone(), 0, contig=r)
        np.testing.assert_array_equal(rows[rows["contig"] == r], want)
    pipe.close()


def test_counter_back_to_back_on_one_stream(model, records):
    """The same record three times on one stream with nothing between the calls (the allocator hands the calls the same workspace: a
    counter that is not zeroed again, or zeroed out of order, starts past the first pairs), rows and merged output."""
    from deepgrp_amd.pipeline import ContigPipeline
    _idx, d, nwin, queued, _sliced = records["three-pairs"]
    runs = [model.forward_windows(d, S, 0, nwin) for _ in range(3)]
    for k, got in enumerate(runs):
        assert torch.equal(_bits(got), _bits(queued)), k
    pipe = ContigPipeline(model, S, 256, 50, 50, True)
    merged = [pipe.merged(d) for _ in range(3)]
    want = _max_merge(queued, d.numel(), 256, S)
    for k, got in enumerate(merged):
        assert torch.equal(_bits(got), _bits(want)), k
    pipe.close()


def test_counter_on_two_streams_from_two_threads(dev, model, records):
    """Two host threads, a stream each, the same record at once: each call's counter lies in its own workspace."""
    _idx, d, nwin, queued, _sliced = records["three-pairs"]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    got, errs = [None, None], []
    start = threading.Barrier(2)

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                start.wait(timeout=30)
                got[k] = [model.forward_windows(d, S, 0, nwin) for _ in range(2)]
            streams[k].synchronize()
        except Exception as e:                                   # noqa: BLE001 (reported by the assertion below)
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    torch.cuda.synchronize()
    for k in range(2):
        for j, rows in enumerate(got[k]):
            assert torch.equal(_bits(rows), _bits(queued)), (k, j)


def _oracle_weights(orc, w):
    return orc.Weights(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, T)


def test_queued_pairs_against_float64(orc, grid, weights, records):
    """32 windows of pairs that came out of the queue -- 16 across the two tiles of a middle pair, 16 of the last pair (the end of its
    full tile and the 7-window one) -- against the float64 statement, at the 1e-5 of the forward tests."""
    idx, _d, nwin, queued, _sliced = records["three-pairs"]
    w = _oracle_weights(orc, weights)
    npairs = (nwin + 31) // 32
    mid = grid + grid // 2
    assert grid <= mid < npairs - 1 and npairs - 1 >= 2 * grid
    for w0, k in ((32 * mid + 8, 16), (32 * (npairs - 1) + 7, 16)):
        want = orc.nn_forward(idx, w, S, w0, k, np.float64)
        err = float(np.abs(queued[w0:w0 + k].cpu().numpy() - want).max())
        print(f"windows {w0}..{w0 + k - 1}: max |dp| = {err:.3e}")
        assert err < 1e-5
    assert 32 * (npairs - 1) + 7 + 16 == nwin
