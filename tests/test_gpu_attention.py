"""The softmax over time of attention_wave_kernel<UP, CM, AT>, attention_row_kernel<AT, EPL, TT> and ref_head_kernel on attention
scales that make it do work, against the float64 statement.

The glorot scale of the other modules' weights (every |scale[k]| < 0.6) leaves the attention logits within 0.1 to 0.3 of each other:
the softmax over t is all but a mean, the running maximum hardly moves from tile to tile (alpha ~ 1) and most shapes run a single
tile.  Every row of attention_family.TABLE -- one per attention code path -- runs here with five weight sets:

  base      the plain gain-1.5 weights: a miss here is a bug at that shape
  uniform   scale 0: a[t] = 1 / T exactly; a padded step that is counted, or one counted 2^SH times, moves the mean
  peaked    scale * 100: nearly one-hot, the peak mid-window and elsewhere in every window
  rising    e[t] strictly increasing: the peak on the last step, every tile raises the running maximum, alpha = 0 on the steep rows
  falling   e[t] strictly decreasing: the peak on step 0, alpha = 1 and the later tiles' weights underflow to 0

A miss on a structured kind alone is a bug in the softmax over time.  test_attention_family_host.py shows on the CPU that these inputs
are well conditioned (the kernels' float32 formulation, or fp16 operands, within a quarter of the contract of float64) and that an
online softmax that does not rescale its context or its sum, counts padded steps or pools by a mean misses the contract tenfold and
more.  The bounds are the project's contracts: 1e-5 with split operands, 1e-3 with fp16 operands (test_forward_windows_vs_oracle),
5e-5 on the fp32 path (test_gpu_fp32_path.py).  Each case asserts the pre-pass kernel and the row length of its avg[t] spill,
which select the attention kernel's template.

Measured on an MI355X (this module: 77 tests in 3.7 s, float64 statements included; no case above 0.2 s), max |dp| of the window
probabilities (the merged output: the same figures or smaller):
  kernel  units / T / C           plain     uniform   peaked    rising    falling   contract
  wave    16 / 65 / 5             8.3e-8    1.1e-7    2.1e-7    3.6e-7    2.8e-7    1e-5
  wave    24 / 64 / 5             1.2e-7    1.1e-7    3.5e-7    3.0e-7    1.2e-7    1e-5
  wave    48 / 150 / 5            1.0e-7    9.0e-8    2.0e-7    1.1e-6    2.3e-7    1e-5
  wave    64 / 130 / 16           3.8e-8    4.0e-8    1.2e-7    3.3e-7    4.5e-8    1e-5
  wave    64 / 128 / 5            9.3e-8    1.0e-7    1.7e-7    9.0e-7    1.1e-7    1e-5
  wave    40 / 520 / 5            9.5e-8    9.9e-8    1.7e-7    9.0e-7    3.0e-7    1e-5
  wave    32 / 130 / 5, fp16      6.1e-5    6.0e-5    1.3e-4    2.0e-4    5.2e-5    1e-3
  wave    64 / 65 / 16, fp16      1.0e-5    1.0e-5    3.5e-5    1.9e-4    1.3e-5    1e-3
  row     96 / 50 / 5             8.2e-8    1.1e-7    3.8e-7    1.2e-6    1.3e-7    1e-5
  row     112 / 41 / 16           4.1e-8    3.6e-8    9.5e-8    4.1e-7    4.6e-8    1e-5
  row     128 / 42 / 5, fp16      1.5e-5    1.5e-5    6.1e-5    1.6e-4    2.7e-5    1e-3
  row     192 / 40 / 5            6.2e-8    5.0e-8    1.3e-7    8.6e-7    7.2e-8    1e-5
  row     256 / 33 / 5            5.9e-8    5.9e-8    1.4e-7    9.4e-8    6.6e-8    1e-5
  row     160 / 45 / 5, fp16      1.7e-5    1.7e-5    4.5e-5    1.9e-4    2.3e-5    1e-3
  fp32    300 / 30 / 5            5.1e-8    5.9e-8    5.8e-8    3.4e-7    5.4e-8    5e-5
No kernel missed its contract on any weight set: the structured kinds cost the level-1 kernels a factor of up to 14 over the plain
weights (`rising`, where the logits are sums of terms of 2400 in float32), still an eighth of the contract.  With the rescaling of the
context taken out of attention_row_kernel and that of the sum out of attention_wave_kernel, 35 of these cases fail; at 16 / 65 and
64 / 65, where the second tile holds one step, only `rising` does.
"""
import warnings

import numpy as np
import pytest

import attention_family as af

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 7                                      # user batch size of the merged runs: a short last batch in every row
KINDS = ("base",) + af.KINDS
CASES = [(row, kind) for row in af.TABLE for kind in KINDS]
CASE_IDS = [f"{af.row_id(row)}-{kind}" for row, kind in CASES]


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _device_model(w, row):
    from deepgrp_amd.pipeline import DeviceModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # the fp32 path's warning (test_gpu_classes.py)
        dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=w.T)
    fp32 = row[0][0] == af.FP32
    assert dm.fp32_only == fp32 and bool(dm.kernel_flags & 4) == fp32
    return dm


def _check_plan(dm, row, handle):
    """The pre-pass kernel and the row length of its spill: with the level and the class count they select the attention kernel
    (dgrp_attention_launch_recs: attention_wave_kernel<avg_up, 8 | 16, float | _Float16> up to 64, attention_row_kernel beyond)."""
    (template, pre, up, tile), u, T, C, s = row[:5]
    plan = dm.plan(2, s, handle=handle)
    assert plan.kernel == pre, f"{plan} ran instead of {pre}"
    assert plan.avg_up == up, f"{plan}: spill rows of {plan.avg_up}, not {up}"
    assert (plan.avg_up <= 64) == (template == af.WAVE) or template == af.FP32


@pytest.mark.parametrize("row,kind", CASES, ids=CASE_IDS)
def test_attention_vs_float64(dev, orc, row, kind):
    """Window probabilities within the row's contract of float64, finite, rows summing to 1, also at the row's small window counts;
    the merged output with a short last batch bit for bit the reference's merge of the same handle's probabilities and within the
    same bound of the float64 merge (the attention kernel's LDS image and its atomic-max flush)."""
    from deepgrp_amd.pipeline import ContigPipeline
    variant, u, T, C, s, nw, level, small = row[:8]
    w, idx, want = af.row_case(orc, row, kind)
    dm = _device_model(w, row)
    tol = af.contract(row)
    N = idx.size
    assert orc.window_count(N, T, s) == nw
    d_idx = torch.from_numpy(idx.copy()).to(dev)                   # (the cached array is read-only)
    ref = orc.merge_all(want.astype(np.float32), N, s, B)

    pipe = ContigPipeline(dm, s, B, fast=level == 0)
    _check_plan(dm, row, pipe.handle)
    probs = dm.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy()
    assert probs.shape == (nw, T, C)
    finite = bool(np.isfinite(probs).all())
    err = float(np.abs(probs - want).max()) if finite else float("nan")
    print(f"{af.row_id(row)} {kind}: max |dp| = {err:.2e}")
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
    print(f"{af.row_id(row)} {kind}: merged max |dp| = {merr:.2e}")
    assert np.isfinite(merged).all() and merr < tol
    pipe.close()
    dm.close()


BATCH_ROWS = [r for r in af.TABLE if (r[1], r[2]) in ((48, 150), (96, 50))]


@pytest.mark.parametrize("row", BATCH_ROWS, ids=[af.row_id(r) for r in BATCH_ROWS])
def test_predict_batch_with_the_peak_on_the_last_step(dev, orc, row):
    """dgrp_predict_batch (att_window_row over a record table) gives the rows of dgrp_predict_record record by record, bit for bit,
    with `rising` weights -- every window's context is its last step's -- on one row of either attention kernel."""
    from deepgrp_amd.pipeline import ContigPipeline
    (template, pre, up, tile), u, T, C, s = row[:5]
    w = af.row_case(orc, row, "rising")[0]
    dm = _device_model(w, row)
    rng = np.random.default_rng(u + T)
    lens = [1, T - 1, T, T + 1, 64, T + s, T + 16 * s, 3 * T + 7, 2000] + [int(x) for x in rng.integers(1, 3000, 12)]
    offs, pos = [], 0
    for n in lens:
        pos += int(rng.integers(0, 37)); offs.append(pos); pos += n
    base = rng.choice(5, size=pos + 5, p=[.24, .25, .25, .24, .02]).astype(np.uint8)
    d_base = torch.from_numpy(base).to(dev)
    pipe = ContigPipeline(dm, s, B, 4, 6)
    assert pipe.batchable()
    _check_plan(dm, row, pipe.handle)
    sp = [int(x) for x in rng.integers(0, 1000, len(lens))]
    got = pipe.run_batch(d_base, offs, lens, sp, list(range(len(lens))))
    want = np.concatenate([pipe.run_idx(d_base[o:o + n].clone(), p0, contig=i) for i, (o, n, p0) in enumerate(zip(offs, lens, sp))])
    np.testing.assert_array_equal(got, want)
    print(f"{af.row_id(row)} rising: {len(want)} segment rows of {len(lens)} records, labels {np.unique(want['label']).tolist()}")
    assert len(want) > len(lens)
    pipe.close()
    dm.close()
