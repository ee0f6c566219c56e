"""Every recurrent kernel and both attention kernels at 2-16 classes (the fused kernels' logit tile is 16 wide; the reference's class
count is len(repeats_to_search) + 1, the user's choice), against the float64 statement -- and which kernel ran.

The class count reaches each kernel through its own lane masks and strides and through the merged launch's LDS image, whose length
is budget / (4 C) rows: C decides whether the rows 16 windows span fit the image (full), fit only in part (partial: the other windows
merge into HBM with atomics of their own) or not at all (none).  Every row of TABLE names the kernel family and the image regime its
launch must take (DeviceModel.plan, i.e. dgrp_model_plan): a shape that drifts to another kernel or regime fails here instead of
silently testing something else."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 7                                      # user batch size of the merged runs: a short last batch in every row

# (family, image, cell, units, T, attention, C, step, windows, level, one_tile)
#   family  the recurrent kernel (mode 0 and 1 without attention, the pre-pass, mode 2, with attention)
#   image   the merged launch's LDS image: full / partial / none -- of the recurrent kernel without attention, of the attention kernel
#           with it; "-" on the fp32 path
#   level   1 split operands (the default), 0 fp16 operands (`--fast`)
TABLE = [
    # gru_wave_kernel: NU16 = 1..4 unit groups; with attention UP 16 / 48 / 64 rows of fp32 spill into attention_wave_kernel CM 8 | 16
    ("wave", "full", "GRU", 16, 60, False, 2, 4, 40, 1, False),
    ("wave", "partial", "GRU", 32, 200, False, 16, 50, 36, 1, False),     # the benchmark's window and step
    ("wave", "none", "GRU", 48, 600, False, 16, 50, 20, 1, False),
    ("wave", "full", "GRU", 64, 90, False, 3, 10, 33, 1, False),
    ("wave", "full", "GRU", 16, 40, True, 8, 5, 30, 1, False),
    ("wave", "full", "GRU", 16, 50, True, 16, 5, 30, 1, False),
    ("wave", "full", "GRU", 48, 60, True, 8, 5, 25, 1, False),
    ("wave", "full", "GRU", 48, 80, True, 9, 6, 25, 1, False),
    ("wave", "full", "GRU", 64, 100, True, 3, 10, 20, 1, False),
    ("wave", "partial", "GRU", 64, 200, True, 16, 100, 20, 1, False),
    # gru_split_kernel: 65-96 units; the 17-32-unit attention pre-pass (UP 32 fp32 spill); DGRP_SPLIT_ONE_TILE at 1, 2 and 4 waves
    ("split", "full", "GRU", 80, 100, False, 2, 10, 30, 1, False),
    ("split", "partial", "GRU", 80, 300, False, 16, 20, 20, 1, False),
    ("split", "full", "GRU", 32, 60, True, 2, 5, 25, 1, False),
    ("split", "full", "GRU", 24, 60, True, 16, 4, 25, 1, False),
    ("split", "partial", "GRU", 40, 100, False, 16, 10, 30, 1, True),
    ("split", "full", "GRU", 128, 100, False, 2, 10, 30, 1, True),
    ("split", "full", "GRU", 24, 60, False, 9, 5, 30, 1, True),
    # attention_row_kernel (65-256 units): its image on (3s + T rows) and off ((3s + T) 4 C > 48 KiB), 2 and 4 units per lane
    ("split", "full", "GRU", 96, 100, True, 9, 10, 20, 1, False),
    ("split", "none", "GRU", 96, 800, True, 16, 10, 8, 1, False),
    # gru_split2_kernel: 97-128 units
    ("split2", "full", "GRU", 128, 60, False, 2, 4, 40, 1, False),
    ("split2", "partial", "GRU", 128, 200, False, 16, 50, 36, 1, False),
    ("split2", "none", "GRU", 100, 500, False, 16, 20, 20, 1, False),
    ("split2", "full", "GRU", 112, 100, True, 16, 10, 20, 1, False),
    ("split2", "full", "GRU", 128, 100, True, 2, 10, 16, 1, False),
    # gru_stream64_kernel: 129-256 units, odd (5) and even (6, 8) counts of 32-unit slices
    ("stream64", "full", "GRU", 160, 100, False, 2, 20, 24, 1, False),
    ("stream64", "partial", "GRU", 256, 200, False, 16, 50, 20, 1, False),
    ("stream64", "full", "GRU", 192, 100, True, 16, 20, 20, 1, False),
    ("stream64", "none", "GRU", 192, 1400, True, 9, 10, 5, 1, False),
    # rnn_split_stream_kernel: a GRU window beyond gru_stream64_kernel's carve, the LSTM at level 1, and beyond 128 units at level 0
    ("stream", "none", "GRU", 256, 3200, False, 3, 50, 3, 1, False),
    ("stream", "partial", "LSTM", 48, 100, False, 16, 10, 30, 1, False),
    ("stream", "full", "LSTM", 160, 80, False, 2, 10, 24, 0, False),
    # lstm_fused_kernel: up to 128 units, level 0
    ("lstm", "full", "LSTM", 64, 60, False, 2, 5, 30, 0, False),
    ("lstm", "partial", "LSTM", 128, 200, False, 16, 50, 20, 0, False),
    # gru_fused_kernel: level 0, 1 / 4 / 5 / 8 waves; with attention UP 32 / 64 rows of fp16 spill into attention_wave_kernel
    ("fused", "none", "GRU", 32, 1000, False, 2, 50, 6, 0, False),
    ("fused", "partial", "GRU", 128, 200, False, 16, 50, 20, 0, False),
    ("fused", "none", "GRU", 128, 900, False, 16, 10, 8, 0, False),
    ("fused", "full", "GRU", 160, 200, False, 9, 50, 20, 0, False),
    ("fused", "full", "GRU", 256, 200, False, 16, 50, 20, 0, False),
    ("fused", "full", "GRU", 256, 60, False, 2, 5, 24, 0, False),
    ("fused", "full", "GRU", 32, 60, True, 8, 5, 25, 0, False),
    ("fused", "partial", "GRU", 32, 100, True, 16, 60, 20, 0, False),
    ("fused", "full", "GRU", 64, 60, True, 2, 5, 25, 0, False),
    ("fused", "none", "GRU", 64, 700, True, 16, 10, 12, 0, False),
    # the plain-fp32 kernels: more than 16 classes or more than 256 units
    ("fp32", "-", "GRU", 40, 60, False, 17, 5, 20, 1, False),
    ("fp32", "-", "GRU", 300, 30, False, 3, 4, 12, 1, False),
]


def _id(row):
    fam, img, cell, u, T, att, c, s, nw, level, one = row
    return f"{fam}-{img}-{cell}{u}{'att' if att else ''}-T{T}-C{c}-s{s}-L{level}{'-onetile' if one else ''}"


def _regime(ospan, T, s, want):
    """full / partial / none of a merged launch's LDS image of `ospan` rows, `want` = the rows its windows span."""
    if ospan == 0:
        return "none"
    assert T <= ospan <= want, (ospan, T, want)
    return "full" if ospan == want else "partial"


def attention_kernel(row, avg_up):
    """The second kernel of an attention model (dgrp_attention_launch_recs) and its merged image regime: attention_wave_kernel<UP, CM,
    spill type> up to 64 units, attention_row_kernel beyond -- stated here from the launcher's arithmetic, which is not exported."""
    fam, img, cell, u, T, att, c, s, nw, level, one = row
    esz = 4 if level == 1 else 2
    if avg_up <= 64:
        stat = 4 * avg_up * 2 * 4 + 4 * 64 * (avg_up + 16 // esz) * esz
        budget = 78 * 1024 if stat <= 40 * 1024 and esz == 2 else 156 * 1024
        want = 15 * s + T
        ospan = min(want, (budget - stat) // (c * 4))
        ospan = ospan if ospan >= T else 0
        return ("wave", avg_up, 8 if c <= 8 else 16, "f32" if esz == 4 else "f16"), _regime(ospan, T, s, want)
    span = 3 * s + T
    return ("row", 2 if u <= 128 else 4, "f32" if esz == 4 else "f16"), "full" if span * c * 4 <= 48 * 1024 else "none"


def _make(orc, row, seed=11, gain=1.5):
    from deepgrp_amd.pipeline import DeviceModel
    fam, img, cell, u, T, att, c, s, nw, level, one = row
    if cell == "LSTM":
        w = orc.LSTMWeights.random(u, c, T, seed=seed, gain=gain)
        dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
    else:
        w = orc.Weights.random(u, c, T, att, seed=seed, gain=gain)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)              # the fp32 path's warning: tested on its own below
            dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
    return w, dm


def _modes(row):
    return (2,) if row[5] else (1, 0)


def _check_plan(dm, row, handle):
    """The row's kernel family for every mode its launches take, and its image regime; returns the attention kernel (or None)."""
    fam, img, cell, u, T, att, c, s, nw, level, one = row
    for mode in _modes(row):
        plan = dm.plan(mode, s, handle=handle)
        assert plan.kernel == fam, f"mode {mode}: {plan} ran instead of {fam}"
        if mode == 0 and fam != "fp32":
            assert _regime(plan.ospan, T, s, 15 * s + T) == img, f"merged image {plan} is not {img}"
    if att and fam != "fp32":
        plan = dm.plan(2, s, handle=handle)
        kind, regime = attention_kernel(row, plan.avg_up)
        assert regime == img, f"attention kernel {kind}: image {regime}, not {img}"
        return kind
    return None


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


@pytest.mark.parametrize("row", TABLE, ids=[_id(r) for r in TABLE])
def test_kernel_at_class_count(dev, orc, row, monkeypatch):
    """Per-window probabilities within 1e-5 (level 1) / 1e-3 (level 0) of float64, rows summing to 1; the merged output bit for bit
    the reference's merge of the same handle's probabilities (whole record in one call and in launches of 48 windows) and within the
    same bound of the float64 merge; at 2 and 16 classes the segment rows of the MSS and softmax paths."""
    from deepgrp_amd.pipeline import ContigPipeline
    fam, img, cell, u, T, att, c, s, nw, level, one = row
    if one:
        monkeypatch.setenv("DGRP_SPLIT_ONE_TILE", "1")
    w, dm = _make(orc, row)
    assert dm.fp32_only == (fam == "fp32")
    pipe = ContigPipeline(dm, s, B, 5, 6, fast=level == 0)
    _check_plan(dm, row, pipe.handle)
    rng = np.random.default_rng(u * 100 + T + c)
    N = T + nw * s
    idx = rng.choice(5, size=N, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)
    d_idx = torch.from_numpy(idx).to(dev)
    assert orc.window_count(N, T, s) == nw

    forward = orc.lstm_forward if cell == "LSTM" else orc.nn_forward
    want = forward(idx, w, s, 0, nw, np.float64)
    tol = 1e-3 if level == 0 else 5e-5 if fam == "fp32" else 1e-5
    probs = dm.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy()
    assert probs.shape == (nw, T, c)
    err = float(np.abs(probs - want).max())
    print(f"{_id(row)}: max |dp| = {err:.2e}")
    assert err < tol
    np.testing.assert_allclose(probs.sum(axis=2), 1.0, atol=1e-5)

    same = orc.merge_all(probs, N, s, B)
    ref = orc.merge_all(want.astype(np.float32), N, s, B)
    for chunk in (1 << 20, 48):
        p = ContigPipeline(dm, s, B, fast=level == 0, chunk_windows=chunk)
        merged = p.merged(d_idx).cpu().numpy()
        p.close()
        np.testing.assert_array_equal(merged.view(np.uint32), same.view(np.uint32), err_msg=f"chunk {chunk}")
        assert np.abs(merged - ref).max() < tol

    if c in (2, 16):
        for use_mss in (True, False):
            pp = ContigPipeline(dm, s, B, 5, 6, use_mss, fast=level == 0)
            rows = pp.run_idx(d_idx, 13, contig=2)
            pp.close()
            labels = orc.labels_from_merged(same, 5, 6, use_mss)
            np.testing.assert_array_equal(np.stack([rows["start"], rows["end"], rows["label"]], 1).reshape(-1, 3),
                                          orc.segments(labels, 13), err_msg=f"use_mss={use_mss}")
    pipe.close()
    dm.close()


# what TABLE must reach: (family, mode, image regime) of the recurrent launches and the attention kernels by kind
REQUIRED_PLANS = {
    ("wave", 1, "-"), ("wave", 2, "-"), ("wave", 0, "full"), ("wave", 0, "partial"), ("wave", 0, "none"),
    ("split", 1, "-"), ("split", 2, "-"), ("split", 0, "full"), ("split", 0, "partial"),
    ("split2", 1, "-"), ("split2", 2, "-"), ("split2", 0, "full"), ("split2", 0, "partial"), ("split2", 0, "none"),
    ("stream64", 1, "-"), ("stream64", 2, "-"), ("stream64", 0, "full"), ("stream64", 0, "partial"),
    ("stream", 1, "-"), ("stream", 0, "full"), ("stream", 0, "partial"), ("stream", 0, "none"),
    ("lstm", 1, "-"), ("lstm", 0, "full"), ("lstm", 0, "partial"),
    ("fused", 1, "-"), ("fused", 2, "-"), ("fused", 0, "full"), ("fused", 0, "partial"), ("fused", 0, "none"),
    ("fp32", 1, "-"), ("fp32", 0, "-"),
}
REQUIRED_ATTENTION = {
    (("wave", up, cm, "f32"), img) for up, cm, img in
    ((16, 8, "full"), (16, 16, "full"), (32, 8, "full"), (32, 16, "full"), (48, 8, "full"), (48, 16, "full"), (64, 8, "full"),
     (64, 16, "partial"))} | {
    (("wave", up, cm, "f16"), img) for up, cm, img in ((32, 8, "full"), (32, 16, "partial"), (64, 8, "full"), (64, 16, "none"))} | {
    (("row", 2, "f32"), "full"), (("row", 2, "f32"), "none"), (("row", 4, "f32"), "full"), (("row", 4, "f32"), "none")}
REQUIRED_SPLIT_WAVES = {1, 2, 3, 4}                 # gru_split_kernel<NW>
REQUIRED_FUSED_WAVES = {1, 4, 5, 8}


def test_table_covers_every_kernel_regime_and_class_count(dev, orc, monkeypatch):
    """No launches: every model of TABLE is built and its plans queried.  The (family, mode, image regime) pairs and the attention
    kernels reached must be exactly the required sets; the class counts every family runs at include 2 and 16."""
    plans, attn, classes = set(), set(), {}
    split_waves, fused_waves = set(), set()
    for row in TABLE:
        fam, img, cell, u, T, att, c, s, nw, level, one = row
        monkeypatch.setenv("DGRP_SPLIT_ONE_TILE", "1") if one else monkeypatch.delenv("DGRP_SPLIT_ONE_TILE", raising=False)
        _, dm = _make(orc, row)
        dm.set_precision(level)
        kind = _check_plan(dm, row, None)
        for mode in _modes(row):
            plans.add((fam, mode, img if mode == 0 else "-"))
        if kind:
            attn.add((kind, img))
        if fam == "split":
            split_waves.add((u + 31) // 32)
        if fam == "fused":
            fused_waves.add((u + 31) // 32)
        classes.setdefault(fam, set()).add(c)
        dm.close()
    monkeypatch.delenv("DGRP_SPLIT_ONE_TILE", raising=False)
    assert plans == REQUIRED_PLANS, (sorted(plans - REQUIRED_PLANS), sorted(REQUIRED_PLANS - plans))
    assert attn == REQUIRED_ATTENTION, (sorted(attn - REQUIRED_ATTENTION), sorted(REQUIRED_ATTENTION - attn))
    assert split_waves == REQUIRED_SPLIT_WAVES and REQUIRED_FUSED_WAVES <= fused_waves
    for fam, cs in classes.items():
        if fam != "fp32":
            assert {2, 16} <= cs, (fam, cs)
    every = set().union(*classes.values())
    assert {2, 3, 8, 9, 16, 17} <= every
    print(f"covered: {len(plans)} (family, mode, image) pairs, {len(attn)} attention kernels")


def test_case_comments_name_the_kernel_that_runs(dev, orc):
    """The rows that the case lists of test_gpu_parity.py assign to gru_wave_kernel or gru_stream64_kernel run those kernels
    (level 1): the comments are checks, not hopes.  Window probabilities take mode 1 (mode 2 with attention), merged runs mode 0."""
    import test_gpu_parity as par
    from deepgrp_amd.pipeline import DeviceModel

    def kernel(u, T, att, mode, s):
        w = orc.Weights.random(u, 5, T, att, seed=7)
        dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
        assert dm.kernel_flags & 2
        k = dm.plan(2 if att else mode, s).kernel
        dm.close()
        return k

    fwd = par.FORWARD_CASES
    a = fwd.index((192, 50, True, 1.0, 10, 21))
    for u, T, att, gain, s, nw in fwd[a:a + 4]:
        assert kernel(u, T, att, 1, s) == "stream64", (u, T, att)
    b = fwd.index((34, 200, True, 1.0, 50, 23))
    for u, T, att, gain, s, nw in fwd[b:b + 12]:
        assert u <= 64 and kernel(u, T, att, 1, s) == "wave", (u, T, att)
    mc = par.MERGE_CASES
    a = mc.index((2100, 120, 20, 6, 192, False))
    for N, T, s, B_, u, att in mc[a:a + 4]:
        assert kernel(u, T, att, 0, s) == "stream64", (N, T, u)
    b = mc.index((2000, 200, 50, 7, 36, False))
    for N, T, s, B_, u, att in mc[b:b + 6]:
        assert kernel(u, T, att, 0, s) == "wave", (N, T, u)


def test_plan_query_errors_and_fp32_path_boundary(dev, orc):
    """dgrp_model_plan refuses mode 2 on a model without attention; 16 classes run the fused kernels, 17 the fp32 path (flags bit 2)
    with the package's warning."""
    from deepgrp_amd._lib import DgrpError
    from deepgrp_amd.pipeline import DeviceModel
    w = orc.Weights.random(40, 16, 50, False, seed=3)
    dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=50)
    assert not dm.fp32_only and not (dm.kernel_flags & 4) and dm.plan(1, 5).kernel == "wave"
    with pytest.raises(DgrpError, match="without attention"):
        dm.plan(2, 5)
    for mode, step in ((3, 5), (-1, 5), (0, 0)):
        with pytest.raises(DgrpError, match="dgrp_model_plan"):
            dm.plan(mode, step)
    dm.close()
    w = orc.Weights.random(40, 17, 50, True, seed=3)
    with pytest.warns(RuntimeWarning, match="17 classes"):
        dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=50)
    assert dm.fp32_only and dm.kernel_flags & 4
    assert [dm.plan(m, 5).kernel for m in (0, 1, 2)] == ["fp32"] * 3
    dm.close()


# ------------------------------------------------------------------------------------------------------- batched path
@pytest.mark.parametrize("cell,u,T,att,c,s,Bb,fam,mode", [("GRU", 36, 60, True, 16, 7, 9, "wave", 2),
                                                          ("GRU", 128, 60, False, 2, 13, 256, "split2", 0),
                                                          ("GRU", 192, 50, False, 9, 10, 16, "stream64", 0),
                                                          ("LSTM", 48, 40, False, 16, 7, 9, "stream", 0)])
def test_predict_batch_at_class_count(dev, orc, cell, u, T, att, c, s, Bb, fam, mode):
    """dgrp_predict_batch (one recurrent launch over a record table) gives the rows of dgrp_predict_record record by record, bit for
    bit, at 2, 9 and 16 classes."""
    from deepgrp_amd.pipeline import ContigPipeline, DeviceModel
    if cell == "LSTM":
        w = orc.LSTMWeights.random(u, c, T, seed=u, gain=2.0)
        m = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
    else:
        w = orc.Weights.random(u, c, T, att, seed=u, gain=3.0)
        m = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
    assert m.plan(mode, s).kernel == fam
    rng = np.random.default_rng(u + c)
    lens = [1, T - 1, T, T + 1, 64, T + s, T + 16 * s, 3 * T + 7, 2000] + [int(x) for x in rng.integers(1, 4000, 20)]
    offs, pos = [], 0
    for n in lens:
        pos += int(rng.integers(0, 37)); offs.append(pos); pos += n
    base = rng.choice(5, size=pos + 5, p=[.24, .25, .25, .24, .02]).astype(np.uint8)
    d_base = torch.from_numpy(base).to(dev)
    pipe = ContigPipeline(m, s, Bb, 4, 6)
    assert pipe.batchable()
    sp = [int(x) for x in rng.integers(0, 1000, len(lens))]
    got = pipe.run_batch(d_base, offs, lens, sp, list(range(len(lens))))
    want = np.concatenate([pipe.run_idx(d_base[o:o + n].clone(), p0, contig=i) for i, (o, n, p0) in enumerate(zip(offs, lens, sp))])
    np.testing.assert_array_equal(got, want)
    labels = np.unique(want["label"])
    assert len(want) > len(lens) and (len(labels) > 1 or c == 2)
    pipe.close()
    m.close()


# ------------------------------------------------------------------------------------------------------- command line
@pytest.mark.parametrize("c", [2, 16])
def test_cli_predict_at_class_count(orc, tmp_path, c):
    """`python -m deepgrp_amd predict` with a 2- and a 16-class model file: the TSV of the reference pipeline run by the oracle on the
    same probabilities."""
    from deepgrp_amd.model import save_keras_hdf5
    from test_gpu_api import _expected_tsv
    T, u = 40, 36
    w = orc.Weights.random(u, c, T, True, seed=c, gain=3.0)
    model_file = str(tmp_path / f"model_c{c}.hdf5")
    save_keras_hdf5(model_file, w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
    rng = np.random.default_rng(c)
    recs = {"chr1": "NNN" + "".join(rng.choice(list("ACGT"), size=3000)), "short": "".join(rng.choice(list("ACGT"), size=T - 1)),
            "chr2 x": "".join(rng.choice(list("acgtn"), size=1200, p=[.23, .23, .23, .23, .08])).strip("n")}
    fasta = tmp_path / "in.fa"
    fasta.write_text("".join(f">{h}\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n" for h, s in recs.items()))
    out = tmp_path / "out.tsv"
    r = subprocess.run([sys.executable, "-m", "deepgrp_amd", "-b", "7", "-s", "4", "-x", "5", "-l", "3", "predict", model_file, str(fasta),
                        "--output", str(out)], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = _expected_tsv(orc, str(fasta), model_file, None, 4, 7, 3, 5, True)
    assert out.read_bytes() == want.encode()
    assert want.count("\n") > 3


# ------------------------------------------------------------------------------------------------------- confusion matrix
@pytest.mark.parametrize("ncls", [2, 16, 17])
def test_confusion_matrix_at_class_count(dev, ncls):
    """dgrp_confusion_matrix against np.histogram2d on either side of the kernel's LDS pitch change (16 -> 64 columns past 16 classes)."""
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import stream_ptr
    rng = np.random.default_rng(ncls)
    n = 300_007
    t = rng.integers(0, ncls, n)
    p = np.where(rng.random(n) < 0.6, t, rng.integers(0, ncls, n))
    d_t, d_p = torch.from_numpy(t.astype(np.int8)).to(dev), torch.from_numpy(p.astype(np.int8)).to(dev)
    cnf = torch.full((ncls, ncls), -1, dtype=torch.int64, device=dev)
    bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    check(lib().dgrp_confusion_matrix(d_t.data_ptr(), d_p.data_ptr(), n, ncls, cnf.data_ptr(), bad.data_ptr(), stream_ptr()))
    want, _, _ = np.histogram2d(t, p, bins=ncls, range=[[0, ncls], [0, ncls]])
    np.testing.assert_array_equal(cnf.cpu().numpy(), want.astype(np.int64))
    assert int(bad.item()) == 0
