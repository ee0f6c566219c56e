"""Saturated gates and a counting cell state on the forward kernels that test_gpu_blend.py leaves out -- gru_stream64_kernel,
gru_fused_kernel at 5 and 8 waves, rnn_split_stream_kernel with either cell, lstm_fused_kernel at 1-4 waves and the fp32 path
(ref_rnn_kernel<CELL, NSL>) -- against the float64 statement.

The random weights of the other modules keep every pre-activation within a few units of 0 and the LSTM cell state below 5.  Every
row of saturation_family.TABLE runs here with two weight sets:

  GRU   above      blend_family.above: z and candidate biases of either sign up to 90 and 45, recurrent columns times 6
        base       the plain gain-1.5 weights
  LSTM  saturated  saturation_family.saturated: every gate at either end in some unit, and counter units whose cell state is
                   +-t -- past |c| = 44.4 the 2^(2 log2e c) inside h = o * tanh(c) is inf in float32 at one end and 0 at the other
        base       the plain gain-1.5 weights

A miss on the second set is a bug at that shape, a miss on the first alone one in the gate or cell arithmetic.
test_saturation_family_host.py shows on the CPU that float32 and float64 agree to 3.2e-7 on all of these inputs and that the named
units move the output by 4.6e-3 and more: a miss here is the kernel's.  The bounds are the project's contracts: 1e-5 with split
operands, 1e-3 with fp16 operands (test_forward_windows_vs_oracle), 5e-5 on the fp32 path (test_gpu_fp32_path.py).

Measured on an MI355X (this module: 44 tests in 4.9 s, float64 statements included; no case above 0.6 s), largest |dp| over the
rows of a family, window probabilities and merged output alike:
                                                  structured weights   plain weights   contract
  stream64  gru_stream64_kernel, GRU, level 1     2.0e-7               8.9e-8          1e-5
  fused     gru_fused_kernel<5|8>, GRU, level 0   7.5e-5               2.9e-5          1e-3
  stream    rnn_split_stream_kernel, GRU, level 1 1.3e-7               7.6e-8          1e-5
  stream    rnn_split_stream_kernel, LSTM         1.1e-7               8.9e-8          1e-5 (160 units at level 0: the same figures)
  lstm      lstm_fused_kernel<1..4>, level 0      1.1e-4               5.5e-5          1e-3
  fp32      ref_rnn_kernel<GRU, 2|4>              2.4e-7               6.4e-8          5e-5
  fp32      ref_rnn_kernel<LSTM, 2|4>             2.8e-7               8.9e-8          5e-5
No kernel missed its contract on either weight set.
"""
import warnings

import numpy as np
import pytest

import saturation_family as sf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 7                                      # user batch size of the merged runs: a short last batch in every row
CASES = [(row, kind) for row in sf.TABLE for kind in sf.KINDS[row[1]]]
CASE_IDS = [f"{sf.row_id(row)}-{kind}" for row, kind in CASES]


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _modes(row):
    return (2,) if row[4] else (1, 0)


def _tol(row):
    """The project's contracts: 5e-5 on the fp32 path (TOL of test_gpu_fp32_path.py), else 1e-5 with split operands and 1e-3
    with fp16 operands (test_forward_windows_vs_oracle).  The LSTM beyond 128 units has the split-operand kernel only, at either
    level: it is held to the bound of the level it was asked for."""
    fam, level = row[0], row[7]
    return 5e-5 if fam == "fp32" else 1e-5 if level == 1 else 1e-3


def _device_model(w, row):
    from deepgrp_amd.pipeline import DeviceModel
    fam, cell, u, T = row[:4]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # the fp32 path's warning (test_gpu_classes.py)
        if cell == "LSTM":
            dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
        else:
            dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
    assert dm.fp32_only == (fam == "fp32") and bool(dm.kernel_flags & 4) == (fam == "fp32")
    if cell == "GRU":
        assert not dm.kernel_flags & 1, "beyond 128 units the two-reciprocal blend is the only one"
    return dm


def _check_plan(dm, row, handle):
    for mode in _modes(row):
        plan = dm.plan(mode, row[5], handle=handle)
        assert plan.kernel == row[0], f"mode {mode}: {plan} ran instead of {row[0]}"


@pytest.mark.parametrize("row,kind", CASES, ids=CASE_IDS)
def test_saturated_vs_float64(dev, orc, row, kind):
    """Window probabilities within the row's contract of float64, finite, rows summing to 1, also at the row's small window counts;
    the merged output with a short last batch bit for bit the reference's merge of the same handle's probabilities and within the
    same bound of the float64 merge (mode 0; with attention the second kernel's merge)."""
    from deepgrp_amd.pipeline import ContigPipeline
    fam, cell, u, T, att, s, nw, level, small = row
    w, idx, want = sf.case(orc, cell, kind, u, T, att, s, nw)
    dm = _device_model(w, row)
    tol = _tol(row)
    N = idx.size
    assert orc.window_count(N, T, s) == nw
    d_idx = torch.from_numpy(idx.copy()).to(dev)                   # (the cached array is read-only)
    ref = orc.merge_all(want.astype(np.float32), N, s, B)

    pipe = ContigPipeline(dm, s, B, fast=level == 0)
    _check_plan(dm, row, pipe.handle)
    probs = dm.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy()
    assert probs.shape == (nw, T, sf.C)
    finite = bool(np.isfinite(probs).all())
    err = float(np.abs(probs - want).max()) if finite else float("nan")
    print(f"{sf.row_id(row)} {kind}: max |dp| = {err:.2e}")
    assert finite
    assert err < tol
    np.testing.assert_allclose(probs.sum(axis=2), 1.0, atol=1e-5)
    for k in small:
        few = dm.forward_windows(d_idx, s, 0, k, handle=pipe.handle).cpu().numpy()
        assert np.isfinite(few).all() and np.abs(few - want[:k]).max() < tol, k
        np.testing.assert_allclose(few.sum(axis=2), 1.0, atol=1e-5)
    merged = pipe.merged(d_idx).cpu().numpy()
    np.testing.assert_array_equal(merged.view(np.uint32), orc.merge_all(probs, N, s, B).view(np.uint32))
    merr = float(np.abs(merged - ref).max())
    print(f"{sf.row_id(row)} {kind}: merged max |dp| = {merr:.2e}")
    assert np.isfinite(merged).all() and merr < tol
    pipe.close()
    dm.close()
