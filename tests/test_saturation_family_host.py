"""The inputs of test_gpu_saturation.py are what it takes them for.  No kernel is measured here: every shape of
saturation_family.TABLE is so well conditioned that a float32 evaluation of the plain statement stays within a tenth of the
level-1 contract of the float64 one, the named units of the LSTM family pin the gate or the cell state they are named for, those
units carry weight in the output (a kernel that got them wrong would move the probabilities by more than any contract), and nothing
but the named columns differs from the random weights.  A shape that misses a condition wants another seed or other magnitudes, not
another figure."""
import numpy as np
import pytest

import blend_family as bf
import saturation_family as sf

SHAPES = sorted({(cell, u, att, T, s, nw) for fam, cell, u, T, att, s, nw, level, small in sf.TABLE})
IDS = [f"{cell}{u}{'att' if att else ''}-T{T}" for cell, u, att, T, s, nw in SHAPES]
LSTM_SHAPES = [sh for sh in SHAPES if sh[0] == "LSTM"]
LSTM_IDS = [i for i, sh in zip(IDS, SHAPES) if sh[0] == "LSTM"]
# every weight set the GPU module runs: the structured one and the random weights it is built on
CASES = [(sh, kind) for sh in SHAPES for kind in sf.KINDS[sh[0]]]
CASE_IDS = [f"{i}-{kind}" for i, sh in zip(IDS, SHAPES) for kind in sf.KINDS[sh[0]]]


@pytest.mark.parametrize("shape,kind", CASES, ids=CASE_IDS)
def test_families_are_well_conditioned(orc, shape, kind):
    """float32 against float64, both the plain statement on the CPU: within 1e-6, a tenth of the level-1 contract, the figure of
    test_blend_family_host.py (measured: GRU above at most 3.2e-7, LSTM saturated at most 2.0e-7, the random weights at most
    1.1e-7); finite, and no class probability collapses to 0 or 1 (measured: 4.6e-2 .. 0.54)."""
    cell, u, att, T, s, nw = shape
    w, idx, want = sf.case(orc, cell, kind, u, T, att, s, nw)
    forward = orc.lstm_forward if cell == "LSTM" else orc.nn_forward
    got = forward(idx, w, s, 0, nw, np.float32)
    err = float(np.abs(got - want).max())
    print(f"{cell} {kind} u={u} T={T} att={att}: float32 - float64 = {err:.2e}, probabilities {want.min():.2e} .. {want.max():.3f}")
    assert np.isfinite(want).all() and np.isfinite(got).all() and want.shape == (nw, T, sf.C)
    assert err < 1e-6
    assert want.max() < 0.99 and want.min() > 1e-3


@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=LSTM_IDS)
def test_lstm_groups_pin_what_they_are_named_for(orc, shape):
    """On the float64 numpy statement of the cell (forward direction, every window): counter units end at c = +-T to 1e-6, both
    signs, and where T >= 60 a unit of each sign passes |c| = 45, beyond which 2^(2 log2e c) is inf in float32 on one side and
    flushed to 0 on the other; input_shut units keep c = 0, forget_shut units |c| <= 1, output units h = tanh(c) or 0; every unit
    outside the groups keeps |c| < 5: what the random weights alone never leave."""
    cell, u, att, T, s, nw = shape
    w, named = sf.saturated(orc, u, sf.C, T, sf.SEED)
    assert w.T == T and set(named) == set(sf.LSTM_GROUPS)
    idx = bf.sequence(u, T, s, nw)
    cs, hs, th = sf.lstm_states(w, idx, s, nw)                       # [T, nw, u]
    assert np.isfinite(cs).all() and np.isfinite(hs).all()

    cnt = named["counter"]
    last = cs[-1][:, cnt]
    assert np.abs(np.abs(last) - T).max() < 1e-6
    signs = np.sign(last)
    assert (signs == signs[0]).all() and {-1.0, 1.0} == set(signs[0])
    assert np.abs(cs[:, :, cnt] - signs[0] * (np.arange(T) + 1)[:, None, None]).max() < 1e-6       # c = +-t at every step
    if T >= 60:
        assert last.max() > 45 and last.min() < -45
    assert np.abs(cs[:, :, named["input_shut"]]).max() < 1e-8 and np.abs(hs[:, :, named["input_shut"]]).max() < 1e-8
    assert np.abs(cs[:, :, named["forget_shut"]]).max() <= 1.0
    out = named["output"]
    o_bias = w.bias[3 * u + out]
    assert (o_bias > 15).any() and (o_bias < -15).any()
    assert np.abs(hs[:, :, out[o_bias > 0]] - th[:, :, out[o_bias > 0]]).max() < 1e-8
    assert np.abs(hs[:, :, out[o_bias < 0]]).max() < 1e-8
    cand = w.bias[2 * u + named["candidate"]]
    assert cand.max() > 9 and cand.min() < -9 and np.abs(cand).max() > 44
    rest = np.ones(u, bool)
    rest[np.concatenate(list(named.values()))] = False
    assert np.abs(cs[:, :, rest]).max() < 5.0
    assert np.abs(cs[:, :, named["candidate"]]).max() < 5.0 and np.abs(cs[:, :, named["cols"]]).max() < 5.0

    # the random weights alone: no unit at all leaves |c| < 5
    cs0 = sf.lstm_states(sf.lstm_base(orc, u, sf.C, T, sf.SEED), idx, s, nw)[0]
    print(f"LSTM u={u} T={T}: max |c| {np.abs(cs).max():.1f} saturated, {np.abs(cs0).max():.2f} on the random weights")
    assert np.abs(cs0).max() < 5.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_named_units_carry_weight_in_the_output(orc, shape):
    """With the Dense rows of one group zeroed (with attention both halves) the float64 probabilities move by at least 3e-3, three
    times the loosest contract (measured: 4.6e-3 .. 2.7e-1): a kernel that got those units wrong cannot hide behind the head.
    input_shut is left out: its correct contribution is 0, which is asserted instead."""
    cell, u, att, T, s, nw = shape
    kind = sf.KINDS[cell][0]
    w, idx, want = sf.case(orc, cell, kind, u, T, att, s, nw)
    named = sf.weights(orc, cell, kind, u, T, att)[1]
    assert set(named) == set(sf.LSTM_GROUPS if cell == "LSTM" else sf.GRU_GROUPS)
    for group, units in named.items():
        ffk = w.ff_kernel.copy()
        ffk[units] = 0
        if att:
            ffk[u + units] = 0
        if cell == "LSTM":
            got = orc.lstm_forward(idx, orc.LSTMWeights(w.kernel, w.recurrent, w.bias, ffk, w.ff_bias, T), s, 0, nw, np.float64)
        else:
            got = orc.nn_forward(idx, orc.Weights(w.kernel, w.recurrent, w.bias, ffk, w.ff_bias, w.scale, T), s, 0, nw, np.float64)
        moved = float(np.abs(got - want).max())
        print(f"{cell} u={u} T={T} att={att}: Dense rows of {group} zeroed: {moved:.2e}")
        if group == "input_shut":
            assert moved < 1e-8
        else:
            assert moved >= 3e-3, group


@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=LSTM_IDS)
def test_nothing_but_the_named_columns_differs_from_the_base(orc, shape):
    cell, u, att, T, s, nw = shape
    b = sf.lstm_base(orc, u, sf.C, T, sf.SEED)
    w, named = sf.saturated(orc, u, sf.C, T, sf.SEED)
    n = max(2, round(u / 24))
    assert [len(named[g]) for g in sf.LSTM_GROUPS] == [n] * 5 + [max(1, n // 2)]
    every = np.concatenate(list(named.values()))
    assert len(set(every)) == len(every) and every.min() >= 0 and every.max() < u
    I, F, G, O = 0, u, 2 * u, 3 * u
    touched_bias = np.concatenate([I + named["counter"], F + named["counter"], G + named["counter"], I + named["input_shut"],
                                   F + named["forget_shut"], O + named["output"], G + named["candidate"]])
    touched_rec = np.concatenate([I + named["cols"], G + named["cols"]])
    keep_b, keep_r = np.ones(4 * u, bool), np.ones(4 * u, bool)
    keep_b[touched_bias], keep_r[touched_rec] = False, False
    np.testing.assert_array_equal(w.bias[keep_b], b.bias[keep_b])
    assert (np.abs(w.bias[~keep_b].astype(np.float64) - b.bias[~keep_b]) > 9).all()
    np.testing.assert_array_equal(w.recurrent[:, keep_r], b.recurrent[:, keep_r])
    np.testing.assert_allclose(w.recurrent[:, touched_rec], 6 * b.recurrent[:, touched_rec], rtol=1e-6)
    for name in ("kernel", "ff_kernel", "ff_bias"):
        np.testing.assert_array_equal(getattr(w, name), getattr(b, name))
    # the GRU rows: blend_family.above and blend_family.base themselves (test_blend_family_host.py states what they are)
    assert sf.SEED == bf.SEED == 11 and sf.C == bf.C == 5


def test_gru_rows_differ_from_the_base_in_the_named_columns_only(orc):
    for cell, u, att, T, s, nw in SHAPES:
        if cell != "GRU" or T > 100:                                # (the long window: the same 256-unit weights but for T)
            continue
        b = bf.base(orc, u, bf.C, T, att, bf.SEED)
        w, named = bf.above(orc, u, bf.C, T, att, bf.SEED)
        assert bf.blend_bound(w) >= 130.0
        touched = np.concatenate(list(named.values()))
        assert len(set(touched)) == len(touched)
        keep = np.ones(3 * u, bool)
        keep[np.concatenate([touched, 2 * u + touched])] = False
        np.testing.assert_array_equal(w.recurrent[:, keep], b.recurrent[:, keep])
        np.testing.assert_array_equal(w.bias[:, keep], b.bias[:, keep])
        np.testing.assert_array_equal(w.kernel, b.kernel)
        np.testing.assert_array_equal(w.ff_kernel, b.ff_kernel)


def waves(u):
    """Waves of 32 units a fused kernel of `u` units runs (lstm_fused_kernel<NW>, gru_fused_kernel<NW>)."""
    return (u + 31) // 32


def test_table_reaches_every_family_and_cell():
    """No launch and no model: the rows name every family for both weight sets (each row runs with both), both cells on the streamed
    kernel and on the fp32 path, lstm_fused_kernel at 1, 2, 3 and 4 waves, gru_fused_kernel at 5 and 8, gru_stream64_kernel with and
    without attention, a window of 60 steps and more in every LSTM family, and the kernel sizes the families stand for."""
    fams = {}
    for row in sf.TABLE:
        fam, cell, u, T, att, s, nw, level, small = row
        fams.setdefault((fam, cell), []).append(row)
        assert len(sf.KINDS[cell]) == 2
        assert not (cell == "LSTM" and att)
        assert nw % 8 and nw % 16, sf.row_id(row)
        assert (level == 0) == (fam in ("fused", "lstm") or row == ("stream", "LSTM", 160, 80, False, 6, 37, 0, ())), sf.row_id(row)
    assert set(fams) == {("stream64", "GRU"), ("fused", "GRU"), ("stream", "GRU"), ("stream", "LSTM"), ("lstm", "LSTM"),
                         ("fp32", "GRU"), ("fp32", "LSTM")}
    assert {waves(r[2]) for r in fams["lstm", "LSTM"]} == {1, 2, 3, 4}
    assert {waves(r[2]) for r in fams["fused", "GRU"]} == {5, 8}
    assert {r[4] for r in fams["stream64", "GRU"]} == {False, True}
    assert all(128 < r[2] <= 256 for fam in ("stream64", "fused") for r in fams[fam, "GRU"])
    assert all(r[2] > 256 for cell in ("GRU", "LSTM") for r in fams["fp32", cell])
    assert any(r[4] for r in fams["fp32", "GRU"])
    stream_lstm = fams["stream", "LSTM"]
    assert any(r[2] <= 128 and r[7] == 1 for r in stream_lstm) and any(r[2] > 128 and r[7] == 1 for r in stream_lstm)
    assert any(r[2] > 128 and r[7] == 0 for r in stream_lstm)
    for fam in ("stream", "lstm", "fp32"):
        assert max(r[3] for r in fams[fam, "LSTM"]) >= 60, fam
    assert sum(1 for r in sf.TABLE if r[8]) >= 3 and all(r[8] in ((), (1, 9)) for r in sf.TABLE)
    assert len({sf.row_id(r) for r in sf.TABLE}) == len(sf.TABLE)
