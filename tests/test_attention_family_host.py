"""The weights of attention_family.py are what test_gpu_attention.py takes them for, shown on the CPU before any kernel is involved:
their logits have the structure each kind is named after, they are so well conditioned that the kernels' own float32 formulation
(level 1, fp32 path) or fp16 operands (level 0) stay within a quarter of the row's contract of float64 -- the kernel keeps three
quarters for what the emulations do not model -- and a tile-wise online softmax with a deliberate defect, or a plain mean over t,
misses the same contract tenfold and more.  Every amplitude of attention_family.TABLE is chosen here, from the references alone.

Measured (float64 numpy and the C statement; this module: 93 tests in 11 s):
  structure     largest rise of the running maximum per tile under `rising` (the smallest over the windows): 201 at 48/150, 205 at
                64/130, 210 at 64/128 (wave kernel), 110 at 96/50, 128 at 112/41, 133 at 192/40, 150 at 256/33 (row kernel), all at
                A = 1200 -- past 87.4 alpha is 0 or denormal; 65 at 40/520 (A = 600), 15 to 61 on the level-0 rows
                under `falling` (A = 1200) every logit behind the first tile lies 162 (128/42, tile of 4) to 696 (64/65) below the peak
                mean largest weight under `peaked`, G = 100: 0.47 (40/520) to 0.89 (24/64) up to 128 units, 0.46 to 0.66 up to 256,
                0.15 at 300; the peak anywhere from step 0 to T - 1
  level 1       float32 formulation, the largest of 8 draws of +-2 ulp on every reciprocal, against float64 (bound 2.5e-6): at most
                2.0e-6 (64/128 rising A = 1200), 1.7e-6 at 40/520 rising A = 600 (A = 1200: 3.1e-6, hence 600), 1.2e-6 peaked;
                on the fp32 path 2.9e-7 (bound 1.25e-5)
  level 0       fp16 operands against float64 (bound 2.5e-4): uniform at most 4.9e-5, peaked G = 100 9.5e-5, falling A = 1200
                6.1e-5; rising 1.9e-4 at 32/130 A = 80 (A = 150: 4.1e-4), 1.1e-4 at 64/65 A = 600, 1.5e-4 at 128/42 A = 300
                (A = 600: 3.1e-4), 2.3e-4 at 160/45 A = 600
  sensitivity   in units of the row's contract, the kind of the row that shows most: context not rescaled 64 (64/65, level 0) to
                43000 (96/50), sum not rescaled 27 to 9900, padded steps counted 10.5 (64/65, level 0, uniform) to 5500, mean
                pooling 27 to 15000
Three choices that these tests forced: `falling` takes A from (600, 1200) at level 0 as well, not from the level-0 ladder of `rising` --
its conditioning does not depend on A, and 600 leaves the tile of 4 steps at 128/42 only 81 below the peak, short of 103.3 -- and
`rising` below A = 150 silences the other units (attention_family.QUIET_BELOW), or 32/130 would not be monotone at the A = 80 that
fp16 operands allow it; and at T = 520 the ramp units' z bias is 6.5 (rising) and 6.0 (falling) in place of 5, with which z^T =
0.03 and the logits are not monotone (attention_family.ramp_bias).
"""
import functools

import numpy as np
import pytest

import attention_family as af

ROWS = list(range(len(af.TABLE)))
IDS = [af.row_id(r) for r in af.TABLE]
TILED = [i for i in ROWS if af.TABLE[i][0][0] != af.FP32]
UNDERFLOW = 126 * np.log(2.0)                   # a rise of the maximum beyond which alpha = 2^(< -126) is 0 or denormal: 87.4
ROUNDING_SEEDS = tuple(range(8))                # draws of the +-2 ulp on the reciprocals: the largest error of them counts
GONE = 149 * np.log(2.0)                        # a logit this far below the maximum has weight < 2^-149, 0 in float32: 103.3


def _amplitudes(row, kind, rung=None):
    G, A_rise, A_fall = row[8:]
    chosen = {"peaked": (G, 0), "rising": (0, A_rise), "falling": (0, A_fall)}.get(kind, (0, 0))
    if rung is None:
        return chosen
    return (rung, 0) if kind == "peaked" else (0, rung)


@functools.lru_cache(maxsize=None)
def _reference(orc, i, kind, rung=None):
    """(weights, class indices, float64 probabilities of the C statement, float64 avg and logits of the numpy one) of row i."""
    variant, u, T, C, s, nw = af.TABLE[i][:6]
    w, idx, want = af.case(orc, kind, u, C, T, s, nw, *_amplitudes(af.TABLE[i], kind, rung))
    avg = af.states(w, idx, s, nw)
    e = af.logits(w, avg)
    avg.setflags(write=False), e.setflags(write=False)
    return w, idx, want, avg, e


def _weights_over_t(e):
    a = np.exp(e - e.max(axis=1, keepdims=True))
    return a / a.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("i", ROWS, ids=IDS)
def test_kinds_have_the_structure_they_are_named_after(orc, i):
    """uniform: every weight 1 / T.  rising / falling: e[t] strictly monotone in every window, the ramp units' states strictly
    increasing; rising raises the running maximum on every tile; under falling every step behind the first tile has weight below
    2^-149.  peaked: mean largest weight at least 0.4 up to 128 units."""
    row = af.TABLE[i]
    (template, pre, up, tile), u, T = row[0], row[1], row[2]
    w, idx, want, avg, e = _reference(orc, i, "uniform")
    assert (w.scale == 0).all() and np.abs(_weights_over_t(e) - 1.0 / T).max() == 0.0

    w, idx, want, avg, e = _reference(orc, i, "peaked")
    amax = float(_weights_over_t(e).max(axis=1).mean())
    peaks = _weights_over_t(e).argmax(axis=1)
    print(f"{af.row_id(row)} peaked G={row[8]}: mean largest weight {amax:.2f}, peaks at {peaks.min()}..{peaks.max()}")
    assert amax >= 0.4 or u > 128

    for kind, sign in (("rising", 1.0), ("falling", -1.0)):
        w, idx, want, avg, e = _reference(orc, i, kind)
        units = af.ramp_units(u)
        assert (np.diff(avg[:, :, units], axis=1) > 0).all(), "the ramp units' states rise"
        assert (sign * np.diff(e, axis=1) > 0).all(), f"{kind}: e[t] is not strictly monotone in every window"
        assert (_weights_over_t(e).argmax(axis=1) == (T - 1 if kind == "rising" else 0)).all()
        rise = np.diff(af.tile_maxima(e, tile), axis=1)
        if kind == "rising":
            assert (rise > 0).all(), "a tile that does not raise the running maximum"
            if rise.size:
                print(f"{af.row_id(row)} rising A={row[9]}: rise per tile {rise.min():.2f} .. {rise.max():.1f}, "
                      f"largest of a window at least {rise.max(axis=1).min():.1f}")
        else:
            assert (rise == 0).all()
            if T > tile:
                below = float((e[:, :1] - e[:, tile:]).min())
                print(f"{af.row_id(row)} falling A={row[10]}: later tiles at least {below:.1f} below the peak")
                assert below > GONE


@pytest.mark.parametrize("template", [af.WAVE, af.ROW])
def test_each_kernel_has_a_rising_row_whose_alpha_underflows(orc, template):
    """At level 1 each kernel template has a rising row in which every window has a tile that raises the maximum by more than
    87.4: alpha = 2^(< -126), zero or denormal."""
    best = 0.0
    for i in TILED:
        row = af.TABLE[i]
        if row[0][0] == template and row[6] == 1 and row[2] > row[0][3]:
            e = _reference(orc, i, "rising")[4]
            best = max(best, float(np.diff(af.tile_maxima(e, row[0][3]), axis=1).max(axis=1).min()))
    print(f"{template}: largest rise per tile {best:.1f}")
    assert best > UNDERFLOW


# ---------------------------------------------------------------------------------------------------------- conditioning
def _float32_error(orc, i, kind, rung=None):
    """The kernels' float32 formulation of the logits on float32 states, everything behind the logits in float64, against float64."""
    w, idx, want, avg, e = _reference(orc, i, kind, rung)
    variant, u, T, C, s, nw = af.TABLE[i][:6]
    a32 = af.states(w, idx, s, nw, np.float32)
    a64 = a32.astype(np.float64)
    return max(float(np.abs(af.head(w, a64, af.softmax_pool(af.logits_float32(w, a32, np.random.default_rng(seed)), a64)) - want).max())
               for seed in ROUNDING_SEEDS)


def _fp16_error(orc, i, kind, rung=None):
    """fp16 operands: the recurrent kernel, the h fed to it and avg rounded to fp16, everything else in float64, against float64."""
    w, idx, want, avg, e = _reference(orc, i, kind, rung)
    variant, u, T, C, s, nw = af.TABLE[i][:6]
    a16 = af.states(w, idx, s, nw, fp16_operands=True)
    return float(np.abs(af.head(w, a16, af.softmax_pool(af.logits(w, a16), a16)) - want).max())


@pytest.mark.parametrize("kind", af.KINDS)
@pytest.mark.parametrize("i", ROWS, ids=IDS)
def test_amplitudes_are_well_conditioned(orc, i, kind):
    """Within a quarter of the row's contract of float64 under the emulation of the row's level, for the amplitude the table holds
    (the larger rungs of its ladder are printed beside it: the table takes the largest that fits with every draw of the rounding).
    A condition on the inputs, not a measurement of any kernel: a row that misses it wants another amplitude, not another figure."""
    row = af.TABLE[i]
    error = _float32_error if row[6] == 1 else _fp16_error
    bound = af.contract(row) / 4
    ladder = {"peaked": af.ladders(row)[0], "rising": af.ladders(row)[1], "falling": af.ladders(row)[2]}.get(kind, (None,))
    chosen = {"peaked": row[8], "rising": row[9], "falling": row[10]}.get(kind)
    assert chosen in ladder
    errs = {rung: error(orc, i, kind, rung) for rung in ladder if rung is None or rung >= chosen}
    print(f"{af.row_id(row)} {kind}: " + ", ".join(f"{rung}: {err:.1e}" for rung, err in errs.items()) + f" (bound {bound:.2e})")
    assert errs[chosen] < bound


# ----------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("i", ROWS, ids=IDS)
def test_defects_of_the_online_softmax_show_tenfold(orc, i):
    """The statement pieced together in numpy is the C statement, and the intact tile-wise online softmax is the statement, to
    1e-12.  Each defect of it -- context not rescaled by alpha, run_l not rescaled by alpha (rows of more than one tile), padded
    steps counted (rows whose T is no multiple of the tile) -- and mean pooling move the output of at least one kind by ten times
    the row's contract.  A row that misses the factor wants another amplitude or shape, not another factor."""
    row = af.TABLE[i]
    (template, pre, up, tile), u, T = row[0], row[1], row[2]
    defects = ["mean"] + (["ctx", "sum"] if T > tile else []) + (["pad"] if T % tile else [])
    moved = {d: {} for d in defects}
    for kind in af.KINDS:
        w, idx, want, avg, e = _reference(orc, i, kind)
        assert np.abs(af.head(w, avg, af.softmax_pool(e, avg)) - want).max() < 1e-12
        assert np.abs(af.head(w, avg, af.online_pool(e, avg, tile)) - want).max() < 1e-12
        for d in defects:
            ctx = af.mean_pool(e, avg) if d == "mean" else af.online_pool(e, avg, tile, d)
            moved[d][kind] = float(np.abs(af.head(w, avg, ctx) - want).max()) / af.contract(row)
    for d in defects:
        kind = max(moved[d], key=moved[d].get)
        print(f"{af.row_id(row)} {d}: {kind} moves by {moved[d][kind]:.1f} contracts")
        assert moved[d][kind] >= 10.0, moved[d]
    assert moved["mean"]["uniform"] < 1e-6 and all(moved["mean"][k] >= 10.0 for k in ("peaked", "rising", "falling"))


def test_table_rows_reach_what_they_are_listed_for():
    """The tile arithmetic the comments of the table claim: valid steps in the last tile, whole tiles, window counts ragged against
    16 and 4."""
    last = {(r[1], r[2]): r[2] % r[0][3] for r in af.TABLE}
    assert last[(16, 65)] == 1 and last[(24, 64)] == 0 and last[(48, 150)] == 22 and last[(64, 130)] == 2 and last[(64, 128)] == 0
    assert last[(40, 520)] == 8 and last[(32, 130)] == 2 and last[(64, 65)] == 1
    assert last[(96, 50)] == 2 and last[(112, 41)] == 1 and last[(128, 42)] == 2 and last[(192, 40)] == 0 and last[(256, 33)] == 1
    assert last[(160, 45)] == 5
    for r in af.TABLE:
        assert r[5] == 9 or (33 <= r[5] <= 37 and r[5] % 16 and r[5] % 4), r
        assert all(k <= r[5] for k in r[7])
    for template in (af.WAVE, af.ROW):
        assert any(r[7] == (1, 5) for r in af.TABLE if r[0][0] == template)
