"""Weights on either side of the constructor's one-reciprocal bound, well conditioned.  Shared by test_blend_family_host.py (the
bound and the conditioning, CPU) and test_gpu_blend.py (every GRU kernel of up to 128 units, both blends, against float64).

dgrp_model_create (api.hip) bounds both pre-activations of every unit by the weights' absolute column sums and biases; a model whose
bound is at most 120 (and that has at most 128 units) takes the one-reciprocal blend, every other the two-reciprocal one.  Scaling
`gain` crosses the bound too, but a large orthogonal recurrent matrix makes the cell chaotic: float32 and float64 evaluations of the
same weights then disagree by more than any kernel could be held to.  The families below change a few units of the gain-1.5 weights
instead -- biases and single recurrent columns -- so that the gates of those units saturate, which damps the dynamics:

  above   bound >= 130 (two-reciprocal blend): about units / 8 units, a third each with a z-gate bias of +-20 .. 90, a candidate
          bias of +-10 .. 45 and with the z and h recurrent columns times 6; both signs, so that z, r * (...) and the tanh saturate
          towards either end
  near    bound in [100, 119] (one-reciprocal blend at the edge of its proof): units whose z input bias of -50 .. -55 and candidate
          input bias of +11 .. +13 drive (1 + 2^az)(1 + 2^ag) to 2^100 and beyond at every step -- the overflow margin the constant
          120 claims -- and as many units with the other three sign combinations.  The recurrent sums of the bound are worst cases
          that no state reaches; what must be large is the part that is always there, the biases.  The z and h recurrent columns of
          these units are scaled down to leave the biases that room under 119.
"""
import functools

import numpy as np

LOG2E = 1.4426950408889634
LIMIT = 120.0                                  # api.hip: worst <= 120.0
GAIN = 1.5                                     # the base of both families (and the `forced` weights of test_gpu_blend.py)


def blend_bound(w):
    """The constructor's bound (api.hip, dgrp_model_create): per unit 1 + log2e * sz + 2 log2e * sg, the maximum over the units.
    sz, sg: largest |input kernel entry| of the z / h column, the biases (z: the two summed in double, then the absolute value;
    h: float32 absolute values of each), the absolute recurrent column sum (float32 absolute values, summed in double)."""
    u = w.u
    k, r, b = w.kernel, w.recurrent, w.bias
    assert k.dtype == r.dtype == b.dtype == np.float32
    a64 = lambda x: np.abs(x).astype(np.float64)                               # fabsf, then widened
    kz, kg = a64(k[:, :u]).max(axis=0), a64(k[:, 2 * u:]).max(axis=0)
    sz = kz + np.abs(b[0, :u].astype(np.float64) + b[1, :u].astype(np.float64)) + a64(r[:, :u]).sum(axis=0)
    sg = kg + a64(b[0, 2 * u:]) + a64(b[1, 2 * u:]) + a64(r[:, 2 * u:]).sum(axis=0)
    return float((1.0 + LOG2E * sz + 2 * LOG2E * sg).max())


def bias_drive(w):
    """Per unit log2e |b_z| + 2 log2e |b_h|: the part of the bound that every step really reaches."""
    u, b = w.u, w.bias.astype(np.float64)
    return LOG2E * np.abs(b[0, :u] + b[1, :u]) + 2 * LOG2E * (np.abs(b[0, 2 * u:]) + np.abs(b[1, 2 * u:]))


def base(orc, u, C, T, attention, seed):
    return orc.Weights.random(u, C, T, attention, seed=seed, gain=GAIN)


def _rebuild(orc, w, kernel, rec, bias):
    return orc.Weights(kernel, rec, bias, w.ff_kernel, w.ff_bias, w.scale, w.T)


def _units(u, n, seed):
    """`n` distinct units spread over every 16- and 32-unit group of the model, in a fixed pseudo-random order."""
    return np.random.default_rng(1000 * seed + u).permutation(u)[:n]


def above(orc, u, C, T, attention, seed):
    """Weights beyond the bound (see the module docstring); returns (weights, {"zbias" | "hbias" | "cols": units})."""
    w = base(orc, u, C, T, attention, seed)
    kernel, rec, bias = w.kernel.astype(np.float64), w.recurrent.astype(np.float64), w.bias.astype(np.float64)
    nb = max(2, round(u / 24))                                  # per bias group: both signs
    nc = max(1, round(u / 24))
    pick = _units(u, 2 * nb + nc, seed)
    zb, hb, cols = pick[:nb], pick[nb:2 * nb], pick[2 * nb:]
    sign = lambda i: 1.0 if i % 2 == 0 else -1.0
    for i, (j, mag) in enumerate(zip(zb, np.linspace(90.0, 20.0, nb))):          # the largest first: 90 alone is 130 of bound
        bias[i % 2, j] += sign(i // 2 + i) * mag                                 # input and recurrent bias alike: the kernels sum them
    for i, (j, mag) in enumerate(zip(hb, np.linspace(45.0, 10.0, nb))):
        bias[i % 2, 2 * u + j] += sign(i // 2 + i) * mag                         # b_in_h outside, b_rec_h inside r * (...)
    for j in cols:
        rec[:, j] *= 6.0
        rec[:, 2 * u + j] *= 6.0
    return _rebuild(orc, w, kernel, rec, bias), {"zbias": zb, "hbias": hb, "cols": cols}


# near: what a driven unit's bound is made of -- 1, the biases, and REC_ROOM for its input kernel and recurrent columns
REC_ROOM = 5.0
NEAR_TOP = 117.5                                # the largest unit bound: inside [100, 119] with room for float32 rounding of the biases


def near(orc, u, C, T, attention, seed):
    """Weights just inside the bound (see the module docstring); returns (weights, {"drive" | "other": units})."""
    w = base(orc, u, C, T, attention, seed)
    kernel, rec, bias = w.kernel.astype(np.float64), w.recurrent.astype(np.float64), w.bias.astype(np.float64)
    nd = max(2, round(u / 32))
    pick = _units(u, 2 * nd + 1, seed + 1)
    drive, other = pick[:nd], pick[nd:]
    k32 = np.abs(w.kernel).astype(np.float64)
    for i, j in enumerate(np.concatenate([drive, other])):
        # the unit's recurrent part of the bound, scaled into what REC_ROOM leaves beside the input kernel
        kpart = LOG2E * k32[:, j].max() + 2 * LOG2E * k32[:, 2 * u + j].max()
        rpart = LOG2E * np.abs(rec[:, j]).sum() + 2 * LOG2E * np.abs(rec[:, 2 * u + j]).sum()
        f = min(1.0, (REC_ROOM - kpart) / rpart)
        assert f > 0
        rec[:, j] *= f
        rec[:, 2 * u + j] *= f
        if i < nd:
            bh = np.linspace(11.0, 13.0, nd)[i]                                  # candidate input bias
            sz, sh = -1.0, 1.0
        else:
            bh = 11.0 + (i - nd) % 3
            sz, sh = ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))[(i - nd) % 3]
        top = NEAR_TOP - 1.5 * (i % 4)                                           # unit bounds 113 .. 117.5
        room = top - 1.0 - REC_ROOM - 2 * LOG2E * (bh + abs(bias[1, 2 * u + j]))
        bz = room / LOG2E                                                        # -50 .. -55 with the candidate biases above
        bias[0, j] = sz * bz - bias[1, j]                                        # the two z biases sum to sz * bz
        bias[0, 2 * u + j] = sh * bh
    return _rebuild(orc, w, kernel, rec, bias), {"drive": drive, "other": other}


def sequence(u, T, s, nw):
    """Class indices of `nw` windows of T at step s (and no more: dgrp_window_count of it is nw), a few N among them."""
    rng = np.random.default_rng(u * 100 + T)
    return rng.choice(5, size=T + nw * s, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)


SEED = 11
C = 5


@functools.lru_cache(maxsize=None)
def case(orc, kind, u, T, attention, s, nw):
    """(weights, class indices, float64 probabilities [nw, T, C]) of one shape and family, computed once per process and
    read-only.  kind: "above", "near" or "base" (the plain gain-1.5 weights)."""
    w = {"above": lambda: above(orc, u, C, T, attention, SEED)[0], "near": lambda: near(orc, u, C, T, attention, SEED)[0],
         "base": lambda: base(orc, u, C, T, attention, SEED)}[kind]()
    idx = sequence(u, T, s, nw)
    want = orc.nn_forward(idx, w, s, 0, nw, np.float64)
    for a in (idx, want, w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias):
        a.setflags(write=False)
    return w, idx, want


# ------------------------------------------------------------------------------------------------------------- shapes
# (family, units, T, attention, step, windows, level, one_tile, small) -- the smallest shapes that reach every (kernel family,
# mode, blend): 5 classes, 33-40 windows (ragged against the 16- and 8-window tiles: the last tile is partly filled), and on one
# row per family `small` window counts (one window; one full 8-window tile and one window of the next).
#   level     1 split operands (the default), 0 fp16 operands
#   one_tile  DGRP_SPLIT_ONE_TILE=1: gru_split_kernel in place of gru_wave_kernel / gru_split2_kernel
# Without attention a row runs mode 1 (window probabilities) and mode 0 (merged); with attention mode 2 and the attention kernel.
TABLE = [
    # gru_wave_kernel<NU>: 1..4 groups of 16 units
    ("wave", 16, 40, False, 5, 33, 1, False, (1, 9)),
    ("wave", 32, 50, False, 7, 37, 1, False, ()),
    ("wave", 48, 60, False, 10, 35, 1, False, ()),
    ("wave", 64, 45, False, 6, 40, 1, False, ()),
    ("wave", 16, 50, True, 5, 34, 1, False, ()),
    ("wave", 36, 60, True, 8, 33, 1, False, ()),
    ("wave", 64, 40, True, 5, 39, 1, False, ()),
    # gru_split_kernel<NW>: 65-96 units (3 waves; with attention attention_row_kernel behind it), the 17-32-unit attention pre-pass
    # (1 wave), and 1, 2 and 4 waves in place of the other two kernels
    ("split", 80, 50, False, 7, 36, 1, False, (1, 9)),
    ("split", 96, 40, True, 5, 33, 1, False, ()),
    ("split", 24, 60, True, 9, 38, 1, False, ()),
    ("split", 24, 45, False, 5, 35, 1, True, ()),
    ("split", 40, 50, False, 8, 37, 1, True, ()),
    ("split", 128, 40, False, 6, 34, 1, True, ()),
    # gru_split2_kernel: 97-128 units
    ("split2", 100, 55, False, 7, 37, 1, False, (1, 9)),
    ("split2", 128, 40, False, 5, 40, 1, False, ()),
    ("split2", 112, 50, True, 10, 33, 1, False, ()),
    # gru_fused_kernel<NW>: fp16 operands, 1..4 waves
    ("fused", 32, 40, False, 5, 36, 0, False, (1, 9)),
    ("fused", 64, 60, False, 10, 33, 0, False, ()),
    ("fused", 96, 50, False, 6, 39, 0, False, ()),
    ("fused", 128, 45, False, 8, 35, 0, False, ()),
    ("fused", 32, 55, True, 7, 34, 0, False, ()),
    ("fused", 64, 40, True, 5, 38, 0, False, ()),
]


def row_id(row):
    fam, u, T, att, s, nw, level, one, small = row
    return f"{fam}-u{u}{'att' if att else ''}-T{T}-s{s}-w{nw}-L{level}{'-onetile' if one else ''}"
