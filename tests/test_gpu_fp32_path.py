"""The fp32 path (dgrp_model_flags bit 2) as a product path: GRU and LSTM models beyond the fused kernels' sizes -- 257-2048 units or
17-64 classes -- run every forward entry point on the plain-fp32 kernels of ref_kernels.hip (forward_ref in api.hip).  Held here to
5e-5 of the float64 statement across the whole envelope: both cells at every unit-slot count NSL of ref_rnn_kernel<CELL, NSL> and on
both sides of each NSL boundary, 17 and 64 classes, attention at 1025+ units and on long windows; a call cut into several passes of
ref_sub_windows windows (per-window output, merged output with the short last batch inside a later pass or on a pass edge, the
record entry points); and the command line with an fp32-path LSTM model."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 5e-5                                 # fp32 path vs float64 (the fused kernels' split-operand default: 1e-5)
B = 7                                      # user batch size of the merged runs of TABLE: a short last batch in every row

# (cell, units, T, attention, classes, step, windows, gain)
TABLE = [
    # NSL 1 (up to 256 units): on the fp32 path only for its classes
    ("GRU", 34, 342, True, 17, 50, 6, 1.0),           # the reference's default shape (defaults.toml) with 17 repeat classes
    ("GRU", 256, 40, False, 64, 7, 10, 1.5),
    ("LSTM", 24, 60, False, 17, 5, 12, 2.0),
    ("LSTM", 256, 30, False, 64, 5, 10, 1.5),
    # NSL 2: 257-512 units
    ("GRU", 257, 30, False, 5, 5, 12, 2.0),
    ("GRU", 512, 20, True, 17, 4, 8, 1.5),
    ("GRU", 300, 280, True, 20, 40, 4, 1.0),          # attention over T > 256 at more than 16 classes
    ("LSTM", 257, 30, False, 5, 5, 10, 1.0),
    ("LSTM", 512, 20, False, 17, 4, 8, 2.0),
    # NSL 4: 513-1024 units
    ("GRU", 513, 16, False, 3, 3, 8, 1.0),
    ("GRU", 1024, 12, False, 64, 3, 6, 2.0),
    ("LSTM", 513, 16, False, 2, 3, 8, 1.5),
    ("LSTM", 1024, 12, False, 33, 3, 6, 1.0),
    # NSL 8: 1025-2048 units, the full 64 KiB of h_{t-1} in LDS at 2048
    ("GRU", 1025, 12, True, 20, 3, 6, 1.5),
    ("GRU", 2048, 10, True, 5, 2, 5, 1.0),
    ("GRU", 2048, 12, False, 64, 3, 5, 2.0),
    ("LSTM", 1025, 12, False, 5, 3, 6, 2.0),
    ("LSTM", 2048, 12, False, 64, 2, 5, 1.5),
]


def _id(row):
    cell, u, T, att, c, s, nw, gain = row
    return f"{cell}{u}{'att' if att else ''}-T{T}-C{c}-s{s}-nw{nw}-g{gain}"


def nsl(u):
    """The unit-slot count of ref_rnn_kernel<CELL, NSL> a model of `u` units launches (dgrp_forward_windows_reference)."""
    n = (u + 255) // 256
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8


def _weights(orc, cell, u, T, att, c, seed, gain):
    """Random model with random biases of both layers (every term of the cell is exercised)."""
    rng = np.random.default_rng(seed)
    if cell == "LSTM":
        w = orc.LSTMWeights.random(u, c, T, seed=seed, gain=gain)
        w.bias[:] += rng.normal(0, 0.2, size=w.bias.shape).astype(np.float32)      # on top of unit_forget_bias's +1
    else:
        w = orc.Weights.random(u, c, T, att, seed=seed, gain=gain)
        w.bias[:] = rng.normal(0, 0.2, size=w.bias.shape).astype(np.float32)
    w.ff_bias[:] = rng.normal(0, 0.2, size=w.ff_bias.shape).astype(np.float32)
    return w


def _model(w, cell, T):
    from deepgrp_amd.pipeline import DeviceModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # the fp32 path's warning (test_gpu_classes.py)
        if cell == "LSTM":
            return DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
        return DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)


def _forward(orc, cell):
    return orc.lstm_forward if cell == "LSTM" else orc.nn_forward


def _check_fp32_plan(dm, att, s):
    assert dm.fp32_only and dm.kernel_flags & 4
    for mode in (0, 1, 2) if att else (0, 1):
        assert dm.plan(mode, s).kernel == "fp32", mode


def _idx(rng, n):
    return rng.choice(5, size=n, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


@pytest.mark.parametrize("row", TABLE, ids=[_id(r) for r in TABLE])
def test_window_probabilities_vs_float64(dev, orc, row):
    """Per-window probabilities within 5e-5 of float64, rows summing to 1; the max error of the CPU fp32 statement of the same
    windows printed beside the device's.  Pipelines at level 0 (--fast) and level 1 run the one fp32 kernel set: the same
    probabilities and merged output bit for bit, and the merged output is the reference's merge of those probabilities."""
    from deepgrp_amd.pipeline import ContigPipeline
    cell, u, T, att, c, s, nw, gain = row
    w = _weights(orc, cell, u, T, att, c, seed=u + c, gain=gain)
    dm = _model(w, cell, T)
    _check_fp32_plan(dm, att, s)
    rng = np.random.default_rng(u * 131 + T + c)
    N = T + nw * s
    assert orc.window_count(N, T, s) == nw
    idx = _idx(rng, N)
    d_idx = torch.from_numpy(idx).to(dev)

    forward = _forward(orc, cell)
    want = forward(idx, w, s, 0, nw, np.float64)
    cpu32 = forward(idx, w, s, 0, nw, np.float32)
    probs = dm.forward_windows(d_idx, s, 0, nw).cpu().numpy()
    assert probs.shape == (nw, T, c)
    err, cpu_err = float(np.abs(probs - want).max()), float(np.abs(cpu32 - want).max())
    print(f"{_id(row)} NSL {nsl(u)}: device {err:.2e}, CPU fp32 {cpu_err:.2e}")
    assert err < TOL, (err, cpu_err)
    np.testing.assert_allclose(probs.sum(axis=2), 1.0, atol=1e-5)

    same = orc.merge_all(probs, N, s, B)
    merged = {}
    for fast in (False, True):
        pipe = ContigPipeline(dm, s, B, fast=fast)
        p = dm.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy()
        np.testing.assert_array_equal(p.view(np.uint32), probs.view(np.uint32), err_msg=f"fast={fast}")
        merged[fast] = pipe.merged(d_idx).cpu().numpy()
        pipe.close()
    np.testing.assert_array_equal(merged[True].view(np.uint32), merged[False].view(np.uint32))
    np.testing.assert_array_equal(merged[False].view(np.uint32), same.view(np.uint32))
    dm.close()


def test_table_covers_the_fp32_envelope(dev, orc):
    """No launches: every model of TABLE is created on the fp32 path and plans the fp32 kernels; TABLE reaches every (cell, NSL) pair,
    both sides of every NSL boundary and 2048 units for both cells, 17 and 64 classes for both cells, GRU attention beyond 1024 units,
    attention over T > 256 at more than 16 classes, and the reference's default shape with 17+ classes.  Rows beyond 1024 units
    stay small, so that the float64 statement does not dominate the file's time."""
    pairs, units, classes = set(), {}, {}
    for cell, u, T, att, c, s, nw, gain in TABLE:
        w = _weights(orc, cell, u, 4, att, c, seed=1, gain=1.0)
        dm = _model(w, cell, T)
        _check_fp32_plan(dm, att, s)
        dm.close()
        pairs.add((cell, nsl(u)))
        units.setdefault(cell, set()).add(u)
        classes.setdefault(cell, set()).add(c)
        assert 1.0 <= gain <= 2.0
        if u > 1024:
            assert T <= 16 and nw <= 8, _id((cell, u, T, att, c, s, nw, gain))
    assert pairs == {(cell, n) for cell in ("GRU", "LSTM") for n in (1, 2, 4, 8)}, sorted(pairs)
    for cell in ("GRU", "LSTM"):
        assert {256, 257, 512, 513, 1024, 1025, 2048} <= units[cell], (cell, sorted(units[cell]))
        assert {17, 64} <= classes[cell], (cell, sorted(classes[cell]))
    assert [nsl(u) for u in (256, 257, 512, 513, 1024, 1025, 2048)] == [1, 2, 2, 4, 4, 8, 8]
    assert any(cell == "GRU" and att and u > 1024 for cell, u, T, att, c, s, nw, g in TABLE)
    assert any(att and T > 256 and c > 16 for cell, u, T, att, c, s, nw, g in TABLE)
    assert any(cell == "GRU" and 32 <= u <= 36 and T == 342 and att and c >= 17 for cell, u, T, att, c, s, nw, g in TABLE)


def _pass_edges(P, nwin):
    return list(range(P, nwin, P))


def test_several_passes_inside_one_call(dev, orc):
    """One call over more windows than one pass of the fp32 kernels (ref_sub_windows, read from dgrp_forward_window_chunk) --
    at least three passes and a short last one:
      * dgrp_forward_windows: float64 at both windows on each side of every pass edge, the first and the last window;
      * dgrp_forward_merge in ONE call with the short last batch of B starting strictly inside a later pass, and on a pass edge:
        bit for bit the reference's merge of the same handle's probabilities;
      * dgrp_forward_merge_record (ContigPipeline.merged) and dgrp_predict_record (run_idx) on the same record, MSS and softmax
        labels: merged output bit for bit, rows = the oracle's post-processing of the device's probabilities."""
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import ContigPipeline, stream_ptr, upload_sequence
    L = lib()
    u, T, att, C, s = 300, 400, True, 20, 50
    w = _weights(orc, "GRU", u, T, att, C, seed=21, gain=1.5)
    # an input-driven state and a head led by the per-position half: the argmax moves along the record, so many labels occur
    w.kernel *= 8.0
    w.recurrent *= 0.5
    w.ff_kernel[:u] *= 0.3
    w.ff_kernel[u:] *= 2.0
    w.ff_bias[:] = 0.0
    dm = _model(w, "GRU", T)
    _check_fp32_plan(dm, att, s)
    P = int(L.dgrp_forward_window_chunk(dm.handle))
    assert 256 <= P <= 1024 and P % 16 == 0, P                      # a pass of a few hundred windows
    nwin = 3 * P + P // 5 + 1                                       # three whole passes and a short fourth
    rng = np.random.default_rng(5)
    seq = "A" + "".join(rng.choice(list("ACGTN"), size=T + nwin * s - 2, p=[.245, .245, .245, .245, .02])) + "C"
    st, d_idx = upload_sequence(seq.encode())
    N = d_idx.numel()
    assert st == 0 and N == len(seq) and orc.window_count(N, T, s) == nwin
    idx = d_idx.cpu().numpy()

    probs = dm.forward_windows(d_idx, s, 0, nwin).cpu().numpy()
    edges = _pass_edges(P, nwin)
    assert len(edges) >= 3
    sample = sorted({0, nwin - 1} | {e + d for e in edges for d in (-2, -1, 0, 1)})
    errs = []
    for a in sample:
        want = orc.nn_forward(idx, w, s, a, 1, np.float64)[0]
        errs.append(float(np.abs(probs[a] - want).max()))
    print(f"passes of {P} windows, {nwin} windows: max |dp| {max(errs):.2e} on windows {sample}")
    assert max(errs) < TOL, dict(zip(sample, errs))
    np.testing.assert_allclose(probs.sum(axis=2), 1.0, atol=1e-5)

    # batch sizes: the short last batch (placement.nfullB) inside a later pass, and on a pass edge
    b_in = next(b for b in range(97, P) if nwin % b and (nwin // b * b) % P and nwin // b * b > P)
    b_edge = P // 2
    assert nwin % b_edge and (nwin // b_edge * b_edge) % P == 0 and nwin // b_edge * b_edge > P
    wb = L.dgrp_forward_workspace_bytes(dm.handle, nwin)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    for Bb in (b_in, b_edge):
        same = orc.merge_all(probs, N, s, Bb)
        out = torch.zeros((N, C), dtype=torch.float32, device=dev)
        check(L.dgrp_forward_merge(dm.handle, d_idx.data_ptr(), N, s, Bb, 0, nwin, out.data_ptr(), work.data_ptr(), wb, stream_ptr()),
              "dgrp_forward_merge")
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), same.view(np.uint32), err_msg=f"dgrp_forward_merge B={Bb}")
        for use_mss in (True, False):
            pipe = ContigPipeline(dm, s, Bb, 5, 6, use_mss)
            assert not pipe.batchable()
            merged = pipe.merged(d_idx).cpu().numpy()
            np.testing.assert_array_equal(merged.view(np.uint32), same.view(np.uint32), err_msg=f"record B={Bb}")
            rows = pipe.run_idx(d_idx, st, contig=4)
            pipe.close()
            want = orc.predict_contig(seq, lambda _i: (lambda a, b: probs[a:a + b]), T, C, s, Bb, 5, 6, use_mss)
            got = np.stack([rows["start"], rows["end"], rows["label"]], 1).reshape(-1, 3)
            np.testing.assert_array_equal(got, want, err_msg=f"rows B={Bb} use_mss={use_mss}")
            assert len(set(got[:, 2].tolist())) > 5, (Bb, use_mss, np.unique(got[:, 2]))
    dm.close()


def test_cli_predict_with_fp32_path_lstm_model(orc, tmp_path):
    """`deepgrp predict` with an LSTM model of 264 units and 18 classes (the fp32 path; not batchable, so record by record) on a
    FASTA of edge-length records -- 1, T-1, T, T+1 bases, an empty record, lower case with inner N, one record longer than a pass
    of the fp32 kernels -- and an all-N record last, which raises the reference's ValueError after the rows before it are written:
    the TSV is the oracle's post-processing of the device's window probabilities, and --fast writes the same bytes."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd._lib import lib
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.pipeline import ContigPipeline
    from test_gpu_api import _expected_tsv
    T, u, C, s = 24, 264, 18, 3
    w = _weights(orc, "LSTM", u, T, False, C, seed=3, gain=1.5)
    w.kernel *= 6.0                                                 # an input-driven state: thousands of rows, several labels
    w.recurrent *= 0.5
    model_file = str(tmp_path / "lstm_fp32.hdf5")
    dgmodel.save_keras_hdf5(model_file, w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model = dgmodel.load_model(model_file)
    assert model.rnn == "LSTM" and model.fp32_only and not ContigPipeline(model, s, 7, 3, 5).batchable()
    P = int(lib().dgrp_forward_window_chunk(model.handle))
    rng = np.random.default_rng(17)
    acgt = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    long_n = T + (P + P // 3) * s
    recs = {"one": acgt(1), "Tm1": acgt(T - 1), "T": acgt(T), "Tp1": acgt(T + 1), "empty": "",
            "mixed x": "".join(rng.choice(list("acgtn"), size=3000, p=[.24, .24, .24, .24, .04])).strip("n"),
            "long": "NN" + acgt(long_n) + "N"}
    assert orc.window_count(long_n, T, s) > P
    text = lambda d: "".join(f">{h}\n" + "".join(sq[i:i + 60] + "\n" for i in range(0, len(sq), 60)) for h, sq in d.items())
    head = tmp_path / "head.fa"
    head.write_text(text(recs))
    fasta = tmp_path / "in.fa"
    fasta.write_text(text(dict(recs, allN="N" * 50)))
    flags = ["-b", "7", "-s", str(s), "-x", "5", "-l", "3"]
    outs = []
    for extra in ([], ["--fast"]):
        out = tmp_path / f"out{len(extra)}.tsv"
        with warnings.catch_warnings(), pytest.raises(ValueError, match="negative dimensions"):
            warnings.simplefilter("ignore", RuntimeWarning)
            main(flags + ["predict", model_file, str(fasta), "--output", str(out)] + extra)
        outs.append(out.read_bytes())
    want = _expected_tsv(orc, str(head), model_file, None, s, 7, 3, 5, True).replace(str(head), str(fasta))
    assert outs[0] == want.encode()
    assert outs[1] == outs[0]
    assert want.count("\tlong\t") > 1000 and want.count("\tmixed x\t") > 100
    model.close()
