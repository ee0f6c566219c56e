"""Attention scales that make the softmax over time do work.  Shared by test_attention_family_host.py (what the inputs are and what
they can show, CPU) and test_gpu_attention.py (attention_wave_kernel, attention_row_kernel and ref_head_kernel against float64).

orc.Weights.random draws the attention scale glorot-uniform over (u, 1): every |scale[k]| is below 0.6, the logits
e[t] = sum_k scale[k] tanh(q[k] + avg[t, k]) differ by 0.1 to 0.3 across a window, and the softmax over t is so flat that replacing it
by a plain mean moves the output by 1e-3 and less.  Whatever the online softmax of the two kernels does wrong -- the running maximum,
the rescaling by alpha = 2^(log2e (run_m - new_m)), the -inf logits behind the window's end, the row kernel's count-once mask -- is
attenuated a thousandfold before an assertion sees it.  The kinds below start from the gain-1.5 weights of blend_family.base:

  uniform   scale = 0: a[t] = 1 / T exactly and the context is the mean of avg; a padded step that is counted, or a step counted
            2^SH times, moves the mean directly
  peaked    scale * G: the softmax is nearly one-hot, the peak wherever the window's states put it
  rising    two ramp units (input z bias + zb, input candidate bias + 10: z ~ const, hh ~ 1, so the state in both directions is
            1 - z^t, strictly increasing) whose scale is +A: e[t] strictly increasing, the peak at T - 1, every tile raises the
            running maximum and alpha < 1 throughout, 0 where the rise per tile passes 87.4 (= 126 ln 2)
  falling   the same units with scale -A: the peak at t = 0, alpha = 1 and the weights of the later tiles underflow to 0

The ramp units are saturated, so their state does not feel operand precision: the kinds stay well conditioned at large A.  The
amplitudes of every row (G, A of rising, A of falling) are chosen by test_attention_family_host.py from the references alone --
never from a GPU result.  Below A = QUIET_BELOW the other units' scale is set to 0 in rising and falling: their 0.1 to 0.3 of logit
noise across a window would break the strict order that a larger A enforces.
"""
import functools

import numpy as np

import blend_family as bf

SEED = bf.SEED
KINDS = ("uniform", "peaked", "rising", "falling")
C2 = 2.8853900817779268                         # 2 log2 e: tanh(x) = 1 - 2 / (1 + 2^(C2 x))
COMP = np.array([3, 2, 1, 0, 4])                # the complement of a class index


QUIET_BELOW = 150                               # rising / falling below this A: the scale of every unit but the ramp units is 0


def ramp_bias(T, kind):
    """The ramp units' z bias: z = sigmoid(zb) ~ 0.993 / 0.989 / 0.953, so that 1 - z^t is still rising at the window's end.  At
    T = 520 it no longer is with zb = 5 (z^T = 0.03: the logits stop being monotone); there `rising` takes 6.5, which keeps the
    ramp alive on the last steps, where its peak is, and `falling` 6.0, which keeps the first step clear of the second in float32
    (the gap between their logits is A (1 - z) against a rounding error of the logits that grows with A as well)."""
    if T > 256:
        return 6.5 if kind == "rising" else 6.0
    return 5.0 if T >= 100 else 4.5 if T > 50 else 3.0


def ramp_units(u):
    return bf._units(u, 2, SEED)


def weights(orc, kind, u, C, T, G, A):
    """orc.Weights of one kind ("base": the plain gain-1.5 weights)."""
    w = bf.base(orc, u, C, T, True, SEED)
    if kind == "base":
        return w
    if kind == "uniform":
        return orc.Weights(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, np.zeros(u, np.float32), T)
    if kind == "peaked":
        return orc.Weights(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale.astype(np.float64) * G, T)
    assert kind in ("rising", "falling")
    units = ramp_units(u)
    bias, scale = w.bias.astype(np.float64), w.scale.astype(np.float64)
    bias[0, units] += ramp_bias(T, kind)
    bias[0, 2 * u + units] += 10.0
    if A < QUIET_BELOW:
        scale[:] = 0.0
    scale[units] = A if kind == "rising" else -A
    return orc.Weights(w.kernel, w.recurrent, bias, w.ff_kernel, w.ff_bias, scale, T)


@functools.lru_cache(maxsize=None)
def case(orc, kind, u, C, T, s, nw, G, A):
    """(weights, class indices, float64 probabilities [nw, T, C]) of one shape and kind, computed once per process and read-only,
    like blend_family.case."""
    w = weights(orc, kind, u, C, T, G, A)
    idx = bf.sequence(u, T, s, nw)
    want = orc.nn_forward(idx, w, s, 0, nw, np.float64)
    for a in (idx, want, w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale):
        a.setflags(write=False)
    return w, idx, want


def row_case(orc, row, kind):
    variant, u, T, C, s, nw, level, small, G, A_rise, A_fall = row
    return case(orc, kind, u, C, T, s, nw, G if kind == "peaked" else 0, {"rising": A_rise, "falling": A_fall}.get(kind, 0))


# ------------------------------------------------------------------------------------------- the statement, piece by piece
def states(w, idx, s, nw, dtype=np.float64, fp16_operands=False):
    """avg[nw, T, u] = (forward + reverse-complement GRU states) / 2 on plain numpy in `dtype`.  fp16_operands: the recurrent kernel
    and the h fed to it rounded to fp16 (the state itself stays in `dtype`) and avg rounded to fp16 -- the operands of the level-0
    kernels and their spill."""
    T, u = w.T, w.u
    f16 = lambda x: x.astype(np.float16).astype(dtype)
    W, U = w.kernel.astype(dtype), w.recurrent.astype(dtype)
    bi, br = w.bias.astype(dtype)
    if fp16_operands:
        U = f16(U)
    win = idx[(np.arange(nw) * s)[:, None] + np.arange(T)[None, :]].astype(np.int64)
    onehot = np.eye(5, dtype=dtype)[win]
    one = dtype(1)

    def gru(x):
        h, outs = np.zeros((nw, u), dtype), []
        for t in range(T):
            xm, hm = x[:, t, :] @ W + bi, (f16(h) if fp16_operands else h) @ U + br
            z = one / (one + np.exp(-(xm[:, :u] + hm[:, :u])))
            r = one / (one + np.exp(-(xm[:, u:2 * u] + hm[:, u:2 * u])))
            h = z * h + (one - z) * np.tanh(xm[:, 2 * u:] + r * hm[:, 2 * u:])
            outs.append(h)
        return np.stack(outs, axis=1)

    avg = (gru(onehot) + gru(onehot[:, ::-1, :][:, :, COMP])) / dtype(2)
    return f16(avg) if fp16_operands else avg


def logits(w, avg):
    """e[nw, T] = sum_k scale[k] tanh(q[k] + avg[t, k]), q = avg[T - 1], in float64."""
    avg = avg.astype(np.float64)
    return (w.scale.astype(np.float64) * np.tanh(avg[:, -1:, :] + avg)).sum(-1)


def logits_float32(w, avg, rng):
    """e as the kernels form it, in float32: r = 1 / (1 + 2^(C2 (q + a))), every r off by a random -2 .. 2 ulp (v_exp_f32 and
    v_rcp_f32 are 1 ulp each), e = sum(scale) - 2 sum_k scale[k] r[k] summed unit by unit."""
    f = np.float32
    avg, sc, c = avg.astype(f), w.scale.astype(f), f(C2)
    r = (f(1) / (f(1) + np.exp2(c * avg + c * avg[:, -1:, :]))).astype(f)
    r = (r * (f(1) + rng.integers(-2, 3, r.shape).astype(f) * f(2.0 ** -23))).astype(f)
    acc, ssum = np.zeros(avg.shape[:2], f), f(0)
    for k in range(avg.shape[2]):
        acc = (acc + (f(-2) * sc[k]) * r[:, :, k]).astype(f)
        ssum = f(ssum + sc[k])
    return (ssum + acc).astype(np.float64)


def softmax_pool(e, avg):
    """The statement: ctx[nw, u] = sum_t softmax_t(e)[t] avg[t]."""
    a = np.exp(e - e.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    return (a[:, :, None] * avg).sum(axis=1)


def mean_pool(e, avg):
    return avg.mean(axis=1)


def online_pool(e, avg, tile, defect=None):
    """The kernels' softmax over t: tiles of `tile` steps, the steps behind the window's end at -inf with weight 0, running maximum
    and sum, context and sum rescaled by alpha per tile.  defect: "ctx" the context is not rescaled, "sum" run_l is not rescaled,
    "pad" the padded steps count, with the last row and its logit (what the kernels load for them)."""
    nw, T, u = avg.shape
    run_m, run_l, ctx = np.full(nw, -np.inf), np.zeros(nw), np.zeros((nw, u))
    for t0 in range(0, T, tile):
        t = np.minimum(t0 + np.arange(tile), T - 1)
        valid = (t0 + np.arange(tile) < T) | (defect == "pad")
        et = np.where(valid[None, :], e[:, t], -np.inf)
        new_m = np.maximum(run_m, et.max(axis=1))
        alpha = np.exp2(bf.LOG2E * (run_m - new_m))
        pt = np.where(valid[None, :], np.exp2(bf.LOG2E * (et - new_m[:, None])), 0.0)
        run_l = run_l * (1.0 if defect == "sum" else alpha) + pt.sum(axis=1)
        ctx = ctx * (1.0 if defect == "ctx" else alpha[:, None]) + (pt[:, :, None] * avg[:, t, :]).sum(axis=1)
        run_m = new_m
    return ctx / run_l[:, None]


def head(w, avg, ctx):
    """Class probabilities [nw, T, C] of concat(ctx, avg[t]) . ff_kernel + ff_bias, in float64."""
    T = avg.shape[1]
    feat = np.concatenate([np.repeat(ctx[:, None, :], T, axis=1), avg.astype(np.float64)], axis=2)
    lg = feat @ w.ff_kernel.astype(np.float64) + w.ff_bias.astype(np.float64)
    p = np.exp(lg - lg.max(axis=2, keepdims=True))
    return p / p.sum(axis=2, keepdims=True)


def tile_maxima(e, tile):
    """[nw, tiles]: the running maximum after each tile, the padded steps of the last tile at -inf."""
    nw, T = e.shape
    pad = np.full((nw, -T % tile), -np.inf)
    return np.maximum.accumulate(np.concatenate([e, pad], axis=1).reshape(nw, -1, tile).max(axis=2), axis=1)


# ------------------------------------------------------------------------------------------------------------- shapes
# (variant, units, T, classes, step, windows, level, small, G, A of rising, A of falling): one row per attention code path, 33-37
# windows (ragged against the wave kernel's 16 windows per workgroup and the row kernel's 4; the T = 520 row: 9), `small` window
# counts on one row per kernel template (one window: waves without a window; 5: one window in the row kernel's second workgroup).
#   variant  (kernel template, pre-pass kernel of DeviceModel.plan, row length of the avg[t] spill, tile in steps)
#   level    1 split operands and fp32 spill (contract 1e-5), 0 fp16 operands and spill (1e-3); the fp32 path: 5e-5
#   G, A, A  the largest rung of the row's ladders (below) that test_attention_family_host.py admits
WAVE, ROW, FP32 = "wave", "row", "fp32"
TABLE = [
    # attention_wave_kernel<UP, CM, AT>: tiles of 64 steps
    ((WAVE, "wave", 16, 64), 16, 65, 5, 5, 33, 1, (1, 5), 100, 1200, 1200),     # <16,8,float>: the second tile holds one valid step
    ((WAVE, "split", 32, 64), 24, 64, 5, 7, 35, 1, (), 100, 1200, 1200),        # <32,8,float>: one whole tile; gru_split_kernel<1> pre-pass
    ((WAVE, "wave", 48, 64), 48, 150, 5, 10, 37, 1, (1, 5), 100, 1200, 1200),   # <48,8,float>: DEPTH 2, PIPE; second pass d = 0 only
    ((WAVE, "wave", 64, 64), 64, 130, 16, 8, 34, 1, (), 100, 1200, 1200),       # <64,16,float>: 2 valid steps in the last tile
    ((WAVE, "wave", 64, 64), 64, 128, 5, 6, 35, 1, (), 100, 1200, 1200),        # <64,8,float>: two whole tiles, the AHEAD prefetch bound
    ((WAVE, "wave", 48, 64), 40, 520, 5, 50, 9, 1, (), 100, 600, 1200),         # <48,8,float>: T > 512, logit halves not hoisted
    ((WAVE, "fused", 32, 64), 32, 130, 5, 9, 33, 0, (), 100, 80, 1200),         # <32,8,_Float16>: fp16 spill, three tiles
    ((WAVE, "fused", 64, 64), 64, 65, 16, 5, 35, 0, (1, 5), 100, 600, 1200),    # <64,16,_Float16>: one step in tile 2
    # attention_row_kernel<AT, EPL, TT>: tiles of TT steps
    ((ROW, "split", 96, 8), 96, 50, 5, 5, 33, 1, (1, 5), 100, 1200, 1200),      # <float,2,8>: 2 valid steps in the last tile
    ((ROW, "split2", 128, 8), 112, 41, 16, 7, 35, 1, (), 100, 1200, 1200),      # <float,2,8>: one valid step in the last tile
    ((ROW, "fused", 128, 4), 128, 42, 5, 6, 34, 0, (1, 5), 100, 300, 1200),     # <_Float16,2,4>
    ((ROW, "stream64", 192, 8), 192, 40, 5, 5, 33, 1, (1, 5), 100, 1200, 1200), # <float,4,8>: T a multiple of the tile
    ((ROW, "stream64", 256, 8), 256, 33, 5, 6, 37, 1, (), 100, 1200, 1200),     # <float,4,8>: one valid step in the last tile
    ((ROW, "fused", 160, 8), 160, 45, 5, 8, 37, 0, (), 100, 600, 1200),         # <_Float16,4,8>
    # ref_head_kernel: a plain two-pass softmax, the control (no tiles: one of T steps)
    ((FP32, "fp32", 0, 30), 300, 30, 5, 4, 33, 1, (), 100, 1200, 1200),
]


def ladders(row):
    """(G, A of rising, A of falling) rungs a row chooses from.  At level 1 the float32 formulation of the logits carries A = 1200
    on every row but T = 520, where the ramp is slow and `rising` spreads its weight over many steps.  With fp16 operands `rising`
    grows ill conditioned with A -- the fp16 rounding of avg moves the logits in proportion to A -- and takes a modest A, while
    `falling`, whose conditioning does not depend on A, carries the underflow case at either level."""
    return ((100,), (600, 1200), (600, 1200)) if row[6] == 1 else ((30, 100), (40, 80, 150, 300, 600), (600, 1200))


def contract(row):
    """The project's contracts (test_gpu_saturation._tol): 5e-5 on the fp32 path, 1e-5 with split operands, 1e-3 with fp16 operands."""
    return 5e-5 if row[0][0] == FP32 else 1e-5 if row[6] == 1 else 1e-3


def row_id(row):
    (template, pre, up, tile), u, T, C, s, nw, level = row[:7]
    return f"{template}-u{u}-T{T}-C{C}-s{s}-w{nw}-L{level}"
