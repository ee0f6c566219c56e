"""The reference's post-processing as numpy evaluates it, and the inputs where a restatement of it goes wrong.  Shared by
test_oracle_post_numerics.py (the oracle, CPU) and test_gpu_post_numerics.py (the HIP kernels).

The expressions below are deepgrp/prediction.py:51-57 (the score transform of apply_mss) and :62-65 (softmax), followed by
the argmax of deepgrp/__main__.py:83, written out as the reference writes them: numpy's float32 log and exp, its pairwise row
sum and its first-maximum argmax are what the oracle and the kernels are held to, bit for bit."""
import contextlib
import io

import numpy as np

F32_ONE = 0x3F800000                       # bit pattern of 1.0f: +0.0 .. 1.0 are the patterns 0 .. F32_ONE


def np_scores(probs):
    """apply_mss's score transform (prediction.py:51-57): scores float64 [N], classes int64 [N]."""
    results_classes = probs.argmax(axis=1)
    mins = probs.max(axis=1) + 1e-6
    mins[mins > 0.99] = 0.99
    t_scores = np.log(mins / (1 - mins))
    scores = np.where(results_classes > 0, t_scores, -10 * t_scores).astype(float)
    return scores, results_classes


def np_t_scores(row_max):
    """The class-independent part of np_scores from the row maxima (float32 [N]): t_scores, float32."""
    mins = row_max + 1e-6
    mins[mins > 0.99] = 0.99
    return np.log(mins / (1 - mins))


def np_softmax(array):
    """prediction.py:62-65, then __main__.py:83: softmax values float32 [N, C] and labels int64 [N]."""
    e_x = np.exp(array - np.max(array))
    sm = e_x / e_x.sum(axis=1, keepdims=True)
    return sm, sm.argmax(axis=1)


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def hexbits(x):
    """float32 or float64 values as their bit patterns, for failure messages."""
    x = np.asarray(x)
    return [f"0x{int(v):0{x.itemsize * 2}x}" for v in x.view(np.uint32 if x.itemsize == 4 else np.uint64)]


def simd_line():
    """numpy's SIMD extensions as np.show_runtime() prints them: numpy's float32 log and exp are per-ISA routines, so a
    mismatch found on a host whose numpy dispatches differently may be the host's, not the code under test."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        np.show_runtime()
    text = " ".join(buf.getvalue().split())
    i = text.find("'simd_extensions'")
    j = text.find("}", i)
    return f"numpy {np.__version__}: " + (text[i:j + 1] if i >= 0 and j > i else text[:400])


def mismatch_report(what, inputs, got, want, bad, k=6):
    """First `k` rows where `bad` holds: the inputs (rows or values) and both results as hex bit patterns."""
    idx = np.flatnonzero(bad)[:k]
    lines = [f"{what}: {int(np.count_nonzero(bad))} of {bad.size} differ ({simd_line()})"]
    for i in idx:
        lines.append(f"  row {i}: input {hexbits(np.atleast_1d(inputs[i]))} got {hexbits(np.atleast_1d(got[i]))} "
                     f"numpy {hexbits(np.atleast_1d(want[i]))}")
    return "\n".join(lines)


# --------------------------------------------------------------------------------------------------- inputs: softmax
def softmax_cases(C, n_random, seed, n_small=4096):
    """float32 [N, C] arrays at C classes, by name:
      random     probabilities in [0, 1) (what the merged network output holds), `n_random` rows
      logits     N(0, 4) values: row maxima and exponentials spread over many binades
      near_tie   the row maximum v at column j and nextafter(v, +inf) at a later column k (C >= 2)
      exact_tie  the row maximum at two or three columns: the first one must win (C >= 2)
      underflow  a peak in [-20, 0] per row, the other columns 87-200 below it: their exponentials are subnormal or zero;
                 the global maximum 0 sits in row 0"""
    rng = np.random.default_rng(seed * 1000 + C)
    out = {"random": rng.random((n_random, C), dtype=np.float32),
           "logits": (rng.standard_normal((n_small, C)) * 4).astype(np.float32)}
    rows = np.arange(n_small)
    if C >= 2:
        a = (rng.random((n_small, C), dtype=np.float32) * 0.9).astype(np.float32)
        j = rng.integers(0, C - 1, n_small)
        k = j + 1 + (rng.integers(0, 1 << 30, n_small) % (C - 1 - j))
        v = (0.9 + 0.1 * rng.random(n_small)).astype(np.float32)
        a[rows, j] = v
        a[rows, k] = np.nextafter(v, np.float32(np.inf))
        out["near_tie"] = a
        b = (rng.random((n_small, C), dtype=np.float32) * 0.9).astype(np.float32)
        b[rows, j] = v
        b[rows, k] = v
        three = rng.random(n_small) < 0.3
        b[rows[three], rng.integers(0, C, n_small)[three]] = v[three]
        out["exact_tie"] = b
    peak = -(rng.random(n_small) * 20).astype(np.float32)
    u = (peak[:, None] - (87 + 113 * rng.random((n_small, C)))).astype(np.float32)
    u[rows, rng.integers(0, C, n_small)] = peak
    u[0, 0] = 0.0
    out["underflow"] = u
    return out


# --------------------------------------------------------------------------------------------------- inputs: scores
def score_rows(row_max, C, phase=0):
    """float32 [N, C] rows whose maxima are `row_max` (float32 [N], >= 0), the rest 0.  Row i holds its maximum at column
    (i // 3 + phase) % C and, for C >= 2, by i % 3: nothing else (0), the same value at another column (1: an exact tie,
    the other column before or after), or nextafter(maximum, 0) at another column (2: a near tie, before or after)."""
    n = row_max.size
    i = np.arange(n, dtype=np.int64)
    col = (i // 3 + phase) % C
    a = np.zeros((n, C), np.float32)
    if C >= 2:
        kind = i % 3
        other = (col + 1 + (i // (3 * C)) % (C - 1)) % C
        tie = kind == 1
        a[i[tie], other[tie]] = row_max[tie]
        near = kind == 2
        a[i[near], other[near]] = np.nextafter(row_max[near], np.float32(0))
    a[i, col] = row_max
    return a


def score_sweep_bits(stride=16, dense=1 << 16):
    """Bit patterns of row maxima in [+0.0, 1.0]: every `stride`-th, plus every pattern in the neighbourhoods where the
    score formula turns: the 0.99 clamp (maxima near 0.99 - 1e-6), the sign change of the log (near 0.5), the maxima that
    1e-6 swamps (the lowest patterns, the patterns around 1e-6) and the patterns just below 2^-10.  (Some patterns come
    twice: harmless, and cheaper than sorting them out.)"""
    def around(x):
        b = int(np.float32(x).view(np.uint32))
        return np.arange(max(b - dense, 0), min(b + dense, F32_ONE) + 1, dtype=np.uint32)
    parts = [np.arange(0, F32_ONE + 1, stride, dtype=np.uint32), np.array([F32_ONE], np.uint32),
             around(np.float32(0.99) - np.float32(1e-6)), around(np.float32(0.5) - np.float32(1e-6)), around(0.5),
             np.arange(0, dense, dtype=np.uint32), around(1e-6),
             np.arange(int(np.float32(2.0 ** -10).view(np.uint32)) - 4 * dense, int(np.float32(2.0 ** -10).view(np.uint32)),
                       dtype=np.uint32)]
    return np.concatenate(parts)
