"""Checker of the training kernels: the model of deepgrp/model.py:293-336 restated in plain torch ops on the CPU (Keras weight
layout, explicit dropout masks, Keras' CategoricalCrossentropy), differentiated by autograd, in float64 or float32; and the two
optimizer formulas as numpy statements in either precision.  tests/test_train_host.py pins the forward pass to
oracle.nn_forward_numpy."""
import numpy as np
import torch

COMP = [3, 2, 1, 0, 4]
NAMES = ("kernel", "recurrent_kernel", "bias", "scale", "ff_kernel", "ff_bias")


def forward(w, idx, starts, T, masks, dtype=torch.float64):
    """Class probabilities [B, T, C] (torch) of the windows idx[start : start + T]; w: dict of torch tensors of `dtype`."""
    u = w["recurrent_kernel"].shape[0]
    starts = np.asarray(starts, np.int64)
    win = np.minimum(np.asarray(idx)[starts[:, None] + np.arange(T)[None, :]].astype(np.int64), 4)
    x = torch.eye(5, dtype=dtype)[torch.from_numpy(win)]
    rc = x.flip(1)[:, :, COMP]
    if masks is not None:
        m = torch.as_tensor(np.asarray(masks), dtype=dtype)
        x, rc = x * m[:, 0, None, :], rc * m[:, 1, None, :]
    bi, br = w["bias"][0], w["bias"][1]

    def gru(seq):
        h = torch.zeros(seq.shape[0], u, dtype=dtype)
        outs = []
        for t in range(T):
            xm = seq[:, t, :] @ w["kernel"] + bi
            hm = h @ w["recurrent_kernel"] + br
            z = torch.sigmoid(xm[:, :u] + hm[:, :u])
            r = torch.sigmoid(xm[:, u:2 * u] + hm[:, u:2 * u])
            hh = torch.tanh(xm[:, 2 * u:] + r * hm[:, 2 * u:])
            h = z * h + (1 - z) * hh
            outs.append(h)
        return torch.stack(outs, 1), h

    fwd, hf = gru(x)
    rev, hr = gru(rc)
    avg = (fwd + rev) / 2
    if w.get("scale") is not None:
        q = ((hf + hr) / 2)[:, None, :]
        e = (w["scale"] * torch.tanh(q + avg)).sum(-1)
        a = torch.softmax(e, 1)
        ctx = (a[:, :, None] * avg).sum(1)
        feat = torch.cat([ctx[:, None, :].expand(-1, T, -1), avg], 2)
    else:
        feat = avg
    return torch.softmax(feat @ w["ff_kernel"] + w["ff_bias"], 2)


def crossentropy(probs, y):
    """Keras' CategoricalCrossentropy on probabilities: divided by their sum, clipped to [1e-7, 1 - 1e-7], mean over B T."""
    p = probs / probs.sum(-1, keepdim=True)
    p = p.clamp(1e-7, 1 - 1e-7)
    return -(y * torch.log(p)).sum(-1).mean()


def tensors(weights, dtype, requires_grad=False):
    return {k: torch.tensor(np.asarray(weights[k], np.float64), dtype=dtype, requires_grad=requires_grad)
            for k in NAMES if weights.get(k) is not None}


def loss_and_grads(weights, idx, truth, starts, T, masks, dtype=torch.float64):
    """(loss float, {name: gradient ndarray float64}, probabilities ndarray) of one batch; truth int8 [C, N] multi-hot."""
    w = tensors(weights, dtype, True)
    probs = forward(w, idx, starts, T, masks, dtype)
    starts = np.asarray(starts, np.int64)
    y = np.asarray(truth)[:, starts[:, None] + np.arange(T)[None, :]].transpose(1, 2, 0)
    loss = crossentropy(probs, torch.tensor(y, dtype=dtype))
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy().astype(np.float64) for k, v in w.items()}, probs.detach().numpy()


def flat(tensors_by_name):
    return np.concatenate([np.asarray(tensors_by_name[k]).reshape(-1) for k in NAMES if tensors_by_name.get(k) is not None])


def rmsprop_step(w, g, ms, mom, lr, rho, momentum, epsilon, dtype=np.float64):
    """TensorFlow's RMSprop: ms = rho ms + (1 - rho) g^2; mom = momentum mom + lr g / sqrt(ms + epsilon); w -= mom.
    Arrays of `dtype`; the scalars are rounded to it once.  Returns (w, ms, mom)."""
    f = dtype
    g = g.astype(f)
    ms = f(rho) * ms + (f(1.0 - rho) * g) * g
    mom = f(momentum) * mom + (f(lr) * g) / np.sqrt(ms + f(epsilon))
    return w - mom, ms, mom


def adam_step(w, g, m, v, lr, b1, b2, epsilon, step, dtype=np.float64):
    """TensorFlow's Adam: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + epsilon).
    Returns (w, m, v)."""
    f = dtype
    g = g.astype(f)
    lr_t = lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    m = f(b1) * m + f(1.0 - b1) * g
    v = f(b2) * v + (f(1.0 - b2) * g) * g
    return w - (f(lr_t) * m) / (np.sqrt(v) + f(epsilon)), m, v


def rel_err(got, want):
    """max |got - want| / max |want| (0 / 0 = 0)."""
    want = np.asarray(want, np.float64)
    d = float(np.abs(np.asarray(got, np.float64) - want).max())
    s = float(np.abs(want).max())
    return d / s if s > 0 else d


def bound(e32):
    """At most 4 x the float32 figure (the summation order differs, the precision may not), with a floor of 1e-6."""
    return max(4.0 * e32, 1e-6)


def make_case(units, T, batch, classes, attention, seed):
    """A small record with N bases and multi-hot truth, start positions that repeat, dropout masks with zeros."""
    from deepgrp_amd import synthetic
    rng = np.random.default_rng(seed)
    n = 4 * T + 37
    idx = rng.integers(0, 4, n).astype(np.uint8)
    idx[rng.random(n) < 0.08] = 4
    starts = rng.integers(0, n - T, batch).astype(np.int64)
    if batch > 2:
        starts[1] = n - T - 1                                           # the last start fetch_batch can draw
    if batch > 1:
        starts[-1] = starts[0]                                          # a repeated start
    first = int(starts[0])
    idx[first + T // 2] = 4                                             # an N inside a window
    truth = np.zeros((classes, n), np.int8)
    for c in range(1, classes):
        a = int(rng.integers(0, n - T // 2 - 1))
        truth[c, a:a + int(rng.integers(2, T + 3))] = 1                # runs may overlap
    truth[1, first + 1:first + 4] = 1
    truth[0, truth[1:].sum(0) == 0] = 1
    truth[2 if classes > 2 else 0, first + 1:first + 3] = 1            # two ones on a base inside a window
    masks = ((rng.random((batch, 2, 5)) >= 0.3) / 0.7).astype(np.float32)
    masks[0, 0, 1] = 0.0
    w = synthetic.synthetic_weights(units, classes, attention, seed=seed + 1)
    return dict(idx=idx, truth=truth, starts=starts, masks=masks, weights=w, T=T)
