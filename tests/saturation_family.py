"""Saturated gates for the forward kernels that blend_family.py leaves out: gru_stream64_kernel, gru_fused_kernel at 5-8 waves,
rnn_split_stream_kernel with either cell, lstm_fused_kernel and the fp32 path (ref_rnn_kernel<CELL, NSL>).  Shared by
test_saturation_family_host.py (what the inputs are, CPU) and test_gpu_saturation.py (the kernels against float64).

GRU rows take blend_family.above unchanged (z and candidate biases of either sign up to 90 and 45, recurrent columns times 6) and,
beside it, blend_family.base.  LSTM rows take `saturated` below and the plain gain-1.5 weights it is built on.  The LSTM cell state
is unbounded, |c| <= t, and every LSTM kernel evaluates h = o * tanh(c) as 1 - 2 / (1 + 2^(2 log2e c)); random weights keep |c|
below 5, far from where that exponential leaves float32 range (|c| > 44.4) or flushes to 0.  `saturated` changes a few units of the
random weights -- biases and single recurrent columns, as blend_family.above does -- so that each gate of the cell sits at either
end in some unit and the cell state of some units counts the steps:

  counter      b_i += 30, b_f += 60 .. 30, b_c += +-(45 .. 15): i = f = 1 and tanh(z_c) = +-1, so c = +-t; in a window of 60 and
               more steps the exponential of tanh(c) overflows in the units of one sign and vanishes in those of the other
  input_shut   b_i -= 90 .. 20: c and h stay 0
  forget_shut  b_f -= 90 .. 20: a cell without memory, c = i tanh(z_c)
  output       b_o += +-(90 .. 20): h = tanh(c), or h = 0
  candidate    b_c += +-(45 .. 10): tanh(z_c) at either end under ordinary gates
  cols         recurrent columns j (input gate) and 2u + j (candidate) times 6: a large recurrent drive

(gate columns i|f|c|o; signs alternate inside a group and the magnitudes fall linearly.)  The counter's smallest biases are what
`c = +-T to 1e-6` takes at T = 200: the cell loses T (1 - tanh z_c) + T^2 / 2 (1 - f) over a window, and the random part of either
pre-activation stays below 2, so z_c >= 13 and z_f >= 28 leave 2e-9 and 1e-8.
"""
import functools

import numpy as np

import blend_family as bf

SEED = bf.SEED
C = bf.C
GAIN = bf.GAIN
LSTM_GROUPS = ("counter", "input_shut", "forget_shut", "output", "candidate", "cols")
GRU_GROUPS = ("zbias", "hbias", "cols")


def lstm_base(orc, u, C, T, seed):
    return orc.LSTMWeights.random(u, C, T, seed=seed, gain=GAIN)


def saturated(orc, u, C, T, seed):
    """LSTM weights with every gate at either end in some unit (see the module docstring); returns (weights, {group: units})."""
    w = lstm_base(orc, u, C, T, seed)
    rec, bias = w.recurrent.astype(np.float64), w.bias.astype(np.float64)
    n = max(2, round(u / 24))
    nc = max(1, n // 2)
    pick = np.random.default_rng(1000 * seed + u).permutation(u)
    assert 5 * n + nc <= u
    named = {g: pick[k * n:(k + 1) * n] for k, g in enumerate(LSTM_GROUPS[:5])}
    named["cols"] = pick[5 * n:5 * n + nc]
    sign = lambda i: 1.0 if i % 2 == 0 else -1.0
    I, F, G, O = 0, u, 2 * u, 3 * u
    fall = lambda hi, lo: np.linspace(hi, lo, n)
    for i, j in enumerate(named["counter"]):
        bias[I + j] += 30.0
        bias[F + j] += fall(60.0, 30.0)[i]
        bias[G + j] += sign(i) * fall(45.0, 15.0)[i]
    for i, j in enumerate(named["input_shut"]):
        bias[I + j] -= fall(90.0, 20.0)[i]
    for i, j in enumerate(named["forget_shut"]):
        bias[F + j] -= fall(90.0, 20.0)[i]
    for i, j in enumerate(named["output"]):
        bias[O + j] += sign(i) * fall(90.0, 20.0)[i]
    for i, j in enumerate(named["candidate"]):
        bias[G + j] += sign(i) * fall(45.0, 10.0)[i]
    for j in named["cols"]:
        rec[:, I + j] *= 6.0
        rec[:, G + j] *= 6.0
    return orc.LSTMWeights(w.kernel, rec, bias, w.ff_kernel, w.ff_bias, w.T), named


def lstm_states(w, idx, s, nw):
    """The cell on plain float64 numpy, forward direction: (c, h, tanh(c)) as [T, nw, u]."""
    u, T = w.u, w.T
    W, U, b = w.kernel.astype(np.float64), w.recurrent.astype(np.float64), w.bias.astype(np.float64)
    win = idx[(np.arange(nw) * s)[:, None] + np.arange(T)[None, :]]
    sig = lambda x: 1 / (1 + np.exp(-x))
    h, c = np.zeros((nw, u)), np.zeros((nw, u))
    cs, hs = [], []
    with np.errstate(over="ignore"):                               # exp(90) and beyond: 1 / (1 + inf) = 0 is the statement
        for t in range(T):
            g = np.eye(5)[win[:, t]] @ W + h @ U + b
            c = sig(g[:, u:2 * u]) * c + sig(g[:, :u]) * np.tanh(g[:, 2 * u:3 * u])
            h = sig(g[:, 3 * u:]) * np.tanh(c)
            cs.append(c), hs.append(h)
    cs, hs = np.stack(cs), np.stack(hs)
    return cs, hs, np.tanh(cs)


def weights(orc, cell, kind, u, T, attention):
    """(weights, {group: units}) of one kind: GRU "above" | "base", LSTM "saturated" | "base"."""
    if cell == "GRU":
        return bf.above(orc, u, C, T, attention, SEED) if kind == "above" else (bf.base(orc, u, C, T, attention, SEED), {})
    assert not attention
    return saturated(orc, u, C, T, SEED) if kind == "saturated" else (lstm_base(orc, u, C, T, SEED), {})


KINDS = {"GRU": ("above", "base"), "LSTM": ("saturated", "base")}


@functools.lru_cache(maxsize=None)
def case(orc, cell, kind, u, T, attention, s, nw):
    """(weights, class indices, float64 probabilities [nw, T, C]) of one shape and kind, computed once per process and read-only,
    like blend_family.case (which serves the GRU rows)."""
    assert kind in KINDS[cell]
    if cell == "GRU":
        return bf.case(orc, kind, u, T, attention, s, nw)
    w = weights(orc, cell, kind, u, T, attention)[0]
    idx = bf.sequence(u, T, s, nw)
    want = orc.lstm_forward(idx, w, s, 0, nw, np.float64)
    for a in (idx, want, w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias):
        a.setflags(write=False)
    return w, idx, want


# ------------------------------------------------------------------------------------------------------------- shapes
# (family, cell, units, T, attention, step, windows, level, small): 5 classes, window counts ragged against the 16- and 8-window
# tiles, `small` window counts (one window; one full 8-window tile and one window of the next) on one row per family.  level: 1
# split operands (the default), 0 fp16 operands; the fp32 path runs the same kernels at either.  Every LSTM family has a row of 60
# steps and more: only there does |c| pass 45.
TABLE = [
    # gru_stream64_kernel: 129-256 units in waves of 64 (3 and 4 waves); with attention attention_row_kernel behind it
    ("stream64", "GRU", 160, 50, False, 7, 36, 1, (1, 9)),
    ("stream64", "GRU", 256, 45, False, 8, 35, 1, ()),
    ("stream64", "GRU", 192, 40, True, 5, 33, 1, ()),
    ("stream64", "GRU", 256, 40, True, 6, 34, 1, ()),
    # gru_fused_kernel<5> and <8>
    ("fused", "GRU", 160, 50, False, 7, 36, 0, ()),
    ("fused", "GRU", 256, 45, False, 8, 35, 0, ()),
    # rnn_split_stream_kernel: a GRU window too long for gru_stream64_kernel's carve (test_gpu_classes.py), every level-1 LSTM up
    # to 256 units, the level-0 LSTM beyond 128
    ("stream", "GRU", 256, 3200, False, 50, 3, 1, ()),
    ("stream", "LSTM", 48, 60, False, 5, 33, 1, (1, 9)),
    ("stream", "LSTM", 128, 200, False, 10, 34, 1, ()),
    ("stream", "LSTM", 160, 80, False, 6, 37, 1, ()),
    ("stream", "LSTM", 256, 60, False, 5, 33, 1, ()),
    ("stream", "LSTM", 160, 80, False, 6, 37, 0, ()),
    # lstm_fused_kernel<1..4>; from 3 waves on the weight fragments are re-read
    ("lstm", "LSTM", 32, 60, False, 5, 33, 0, ()),
    ("lstm", "LSTM", 64, 60, False, 7, 35, 0, ()),
    ("lstm", "LSTM", 96, 60, False, 6, 34, 0, ()),
    ("lstm", "LSTM", 128, 200, False, 10, 34, 0, (1, 9)),
    # ref_rnn_kernel<CELL, NSL>: NSL 2 and 4
    ("fp32", "GRU", 300, 30, False, 4, 17, 1, ()),
    ("fp32", "GRU", 520, 16, False, 3, 9, 1, ()),
    ("fp32", "GRU", 300, 30, True, 4, 17, 1, ()),
    ("fp32", "LSTM", 257, 64, False, 4, 9, 1, ()),
    ("fp32", "LSTM", 300, 30, False, 4, 17, 1, ()),
    ("fp32", "LSTM", 513, 16, False, 3, 9, 1, ()),
]


def row_id(row):
    fam, cell, u, T, att, s, nw, level, small = row
    return f"{fam}-{cell}{u}{'att' if att else ''}-T{T}-s{s}-w{nw}-L{level}"
