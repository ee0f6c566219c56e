"""Both GRU blends of every kernel that has two -- gru_wave_kernel, gru_split_kernel, gru_split2_kernel, gru_fused_kernel, each
in its three modes -- against the float64 statement.

The constructor (dgrp_model_create) gives a model of up to 128 units the one-reciprocal blend (dgrp_model_flags bit 0) when its
bound on (1 + 2^az)(1 + 2^ag) is at most 2^120, and the two-reciprocal instantiation of every kernel otherwise.  The random weights
of the other modules never cross the bound, so they only ever run one of each pair.  Every row of blend_family.TABLE runs here with
three weight sets:

  above   structured weights beyond the bound (blend_family.above): the two-reciprocal kernels on the inputs they exist for, gates
          saturated at both ends
  forced  the plain gain-1.5 weights under DGRP_GRU_SAFE=1: the two-reciprocal kernels on ordinary gates, and beside them the same
          weights without the variable (the one-reciprocal kernels); the difference of the two is printed
  near    structured weights just inside the bound (blend_family.near): the one-reciprocal kernels with the product at 2^100 and
          above at every step, the margin the constant 120 claims

test_blend_family_host.py shows on the CPU that float32 and float64 agree to 3.2e-7 on these inputs: a miss here is the kernel's.

Measured on an MI355X (this module: 69 tests in 4.1 s, no case above 0.3 s), largest figure over the rows:
                                          split operands (contract 1e-5)   fp16 operands (contract 1e-3)
  above,  two-reciprocal - float64        1.7e-7                           9.7e-5
  forced, two-reciprocal - float64        8.6e-8                           5.7e-5
  forced, one-reciprocal - float64        1.5e-7                           5.7e-5
  near,   one-reciprocal - float64        2.6e-7                           6.2e-5
  forced, two-reciprocal - one-reciprocal 1.5e-7                           2.7e-5      (printed, not asserted)
  above, gru_split2_kernel - gru_split_kernel<4> (100 and 128 units): 1.2e-7 (asserted: 2e-6)
"""
import numpy as np
import pytest

import blend_family as bf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 7                                      # user batch size of the merged runs: a short last batch in every row
KINDS = ("above", "forced", "near")
IDS = [bf.row_id(r) for r in bf.TABLE]


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _modes(row):
    return (2,) if row[3] else (1, 0)


def _tol(level):
    """The project's contract (test_forward_windows_vs_oracle): 1e-5 with split operands, 1e-3 with fp16 operands."""
    return 1e-5 if level == 1 else 1e-3


def _device_model(w):
    from deepgrp_amd.pipeline import DeviceModel
    dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=w.T)
    assert not dm.fp32_only and dm.kernel_flags & 2
    return dm


def _models(w, kind, monkeypatch):
    """The model under test of `kind`, its blend asserted, and for "forced" the same weights with the blend the constructor picks."""
    natural = _device_model(w)
    if kind == "above":
        assert not natural.kernel_flags & 1, f"bound {bf.blend_bound(w):.1f}: the constructor took the one-reciprocal blend"
        return natural, None
    assert natural.kernel_flags & 1, f"bound {bf.blend_bound(w):.1f}: the constructor refused the one-reciprocal blend"
    if kind == "near":
        return natural, None
    monkeypatch.setenv("DGRP_GRU_SAFE", "1")
    forced = _device_model(w)
    monkeypatch.delenv("DGRP_GRU_SAFE")
    assert not forced.kernel_flags & 1
    return forced, natural


def _set_tiles(monkeypatch, one):
    monkeypatch.setenv("DGRP_SPLIT_ONE_TILE", "1") if one else monkeypatch.delenv("DGRP_SPLIT_ONE_TILE", raising=False)


def _check_plan(dm, row, handle):
    for mode in _modes(row):
        plan = dm.plan(mode, row[4], handle=handle)
        assert plan.kernel == row[0], f"mode {mode}: {plan} ran instead of {row[0]}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", bf.TABLE, ids=IDS)
def test_blend_vs_float64(dev, orc, row, kind, monkeypatch):
    """Window probabilities within the contract of float64 (1e-5 split operands, 1e-3 fp16 operands), finite, rows summing to 1,
    also at the row's small window counts; the merged output with a short last batch bit for bit the reference's merge of the same
    handle's probabilities and within the same bound of the float64 merge (mode 0; with attention the second kernel's merge)."""
    from deepgrp_amd.pipeline import ContigPipeline
    fam, u, T, att, s, nw, level, one, small = row
    _set_tiles(monkeypatch, one)
    w, idx, want = bf.case(orc, "base" if kind == "forced" else kind, u, T, att, s, nw)
    dm, other = _models(w, kind, monkeypatch)
    tol = _tol(level)
    N = idx.size
    assert orc.window_count(N, T, s) == nw
    d_idx = torch.from_numpy(idx.copy()).to(dev)                   # (the cached array is read-only)
    ref = orc.merge_all(want.astype(np.float32), N, s, B)

    results = []
    for m in (dm, other) if other is not None else (dm,):
        pipe = ContigPipeline(m, s, B, fast=level == 0)
        _check_plan(m, row, pipe.handle)
        probs = m.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy()
        assert probs.shape == (nw, T, bf.C) and np.isfinite(probs).all()
        err = float(np.abs(probs - want).max())
        print(f"{bf.row_id(row)} {kind} onercp={m.kernel_flags & 1}: max |dp| = {err:.2e}")
        assert err < tol
        np.testing.assert_allclose(probs.sum(axis=2), 1.0, atol=1e-5)
        for k in small:
            few = m.forward_windows(d_idx, s, 0, k, handle=pipe.handle).cpu().numpy()
            assert np.isfinite(few).all() and np.abs(few - want[:k]).max() < tol, k
            np.testing.assert_allclose(few.sum(axis=2), 1.0, atol=1e-5)
        merged = pipe.merged(d_idx).cpu().numpy()
        np.testing.assert_array_equal(merged.view(np.uint32), orc.merge_all(probs, N, s, B).view(np.uint32))
        assert np.isfinite(merged).all() and np.abs(merged - ref).max() < tol
        pipe.close()
        results.append(probs)
    if other is not None:
        # measured, not asserted: both are held to float64 above, which bounds their difference by twice the contract
        print(f"{bf.row_id(row)} two-reciprocal - one-reciprocal: max |dp| = {float(np.abs(results[0] - results[1]).max()):.2e}")
        other.close()
    dm.close()


@pytest.mark.parametrize("row", [r for r in bf.TABLE if r[0] == "split2" and not r[3]], ids=lambda r: bf.row_id(r))
def test_two_reciprocal_split_kernels_agree_across_tiles(dev, orc, row, monkeypatch):
    """gru_split2_kernel and gru_split_kernel<4> (DGRP_SPLIT_ONE_TILE) run the same two-reciprocal gate chain on `above` weights at
    100 and 128 units: within 2e-6 of each other, the figure test_two_tile_and_one_tile_split_kernels_agree holds the
    one-reciprocal chain to -- a record must not change its calls with the way it was batched -- window probabilities and merged
    output alike."""
    from deepgrp_amd.pipeline import ContigPipeline
    fam, u, T, att, s, nw, level, one, small = row
    _set_tiles(monkeypatch, False)
    w, idx, want = bf.case(orc, "above", u, T, att, s, nw)
    dm, _ = _models(w, "above", monkeypatch)
    d_idx = torch.from_numpy(idx.copy()).to(dev)                   # (the cached array is read-only)
    pipe = ContigPipeline(dm, s, B)
    got = {}
    for tiles in (2, 1):
        _set_tiles(monkeypatch, tiles == 1)
        assert [dm.plan(mode, s, handle=pipe.handle).kernel for mode in (1, 0)] == ["split2" if tiles == 2 else "split"] * 2
        got[tiles] = (dm.forward_windows(d_idx, s, 0, nw, handle=pipe.handle).cpu().numpy(), pipe.merged(d_idx).cpu().numpy())
    _set_tiles(monkeypatch, False)
    dp, dmrg = (float(np.abs(got[2][i] - got[1][i]).max()) for i in (0, 1))
    print(f"u={u} above: two tiles - one tile: windows {dp:.2e}, merged {dmrg:.2e}")
    assert dp < 2e-6 and dmrg < 2e-6
    assert max(float(np.abs(got[t][0] - want).max()) for t in (2, 1)) < 1e-5
    assert np.array_equal(got[2][1] == 0, got[1][1] == 0)
    pipe.close()
    dm.close()


FAMILIES = ("wave", "split", "split2", "fused")


def test_table_reaches_every_family_mode_and_blend(dev, orc, monkeypatch):
    """No launches: every model of the table is built and its plans queried.  The (family, mode, one-reciprocal) triples reached
    are exactly the four families in three modes with either blend; with the two-reciprocal blend gru_split_kernel runs at 1-4
    waves and gru_wave_kernel at 1-4 unit groups, in every mode the family has at that size."""
    reached, split_waves, wave_groups = set(), set(), set()
    for row in bf.TABLE:
        fam, u, T, att, s, nw, level, one, small = row
        _set_tiles(monkeypatch, one)
        for kind in KINDS:
            w = {"above": lambda: bf.above(orc, u, bf.C, T, att, bf.SEED)[0], "near": lambda: bf.near(orc, u, bf.C, T, att, bf.SEED)[0],
                 "forced": lambda: bf.base(orc, u, bf.C, T, att, bf.SEED)}[kind]()
            dm, other = _models(w, kind, monkeypatch)
            for m in (dm, other) if other is not None else (dm,):
                m.set_precision(level)
                _check_plan(m, row, None)
                onercp = m.kernel_flags & 1
                for mode in _modes(row):
                    reached.add((fam, mode, onercp))
                    if fam == "split" and not onercp:
                        split_waves.add(((u + 31) // 32, mode))
                    if fam == "wave" and not onercp:
                        wave_groups.add(((u + 15) // 16, mode))
                m.close()
    _set_tiles(monkeypatch, False)
    want = {(fam, mode, blend) for fam in FAMILIES for mode in (0, 1, 2) for blend in (0, 1)}
    assert reached == want, (sorted(reached - want), sorted(want - reached))
    assert {nw_ for nw_, mode in split_waves} == {1, 2, 3, 4}
    assert {(nw_, mode) for nw_ in (1, 2, 3, 4) for mode in (0, 1)} <= split_waves and {(1, 2), (3, 2)} <= split_waves
    assert {nu for nu, mode in wave_groups} == {1, 2, 3, 4}
    # (two unit groups with attention run gru_split_kernel<1>, the 17-32-unit pre-pass)
    assert {(nu, mode) for nu in (1, 2, 3, 4) for mode in (0, 1)} | {(1, 2), (3, 2), (4, 2)} == wave_groups
    print(f"covered: {len(reached)} (family, mode, blend) triples")
