"""The stream and thread contract of include/deepgrp_hip.h, entry point by entry point.

  * "all work is enqueued asynchronously on [`stream`] unless a function says it synchronises": every device entry point runs behind
    a LATE PRODUCER (stream_harness.py) -- poison inputs on the device, a delay on a non-blocking side stream, then the copies that
    put the real inputs in place, then the call on that stream.  A launch or copy on the null stream or an unforked lane reads the
    poison, an unjoined lane leaves the sentinel in the clone taken behind the call, a host table read after the call returned is read
    after it was zeroed.  Asynchronous entry points must return while the delay still runs; synchronising ones are called while it
    still runs and (where the synchronisation is their last act) must return with the stream drained.
  * "workspaces are caller-provided scratch whose contents are unspecified": the workspace arrives filled with 0xA5, 0x00 and 0xFF;
    the outputs are the same bit for bit (for entry points without a workspace the fill is the sentinel of the output buffers).
  * "functions are re-entrant; a dgrp_model may be shared by threads that use different streams and workspaces": four host threads
    with a stream, a view (levels 0 and 1 alternating), a workspace and records of their own give the rows of the same calls made one
    after the other; dgrp_last_error and the kernel timer are per thread.

Every result is compared with the statement the entry point's own test module uses (oracle, numpy, zlib, the brute-force helpers of
test_gpu_mask / test_gpu_evaluate, tracks.reference_text) at the same exactness, and bit for bit with the same call on the idle
default stream.  A positive control (dgrp_encode on the null stream while its producer is delayed) shows per module run that the
trap works on the stream pair in use.

Wall time on one MI355X, both measured in one run (pytest's own figure): this module 10.2 s for its 111 cases,
tests/test_gpu_batch.py 4.5 s for its 23."""
import ctypes as C
import threading
import warnings
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import FILLS, SEG, Harness, c_i64, dev_of, i64ptr, last_error, segs      # noqa: E402

EINVAL = -1


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def H(L):
    from deepgrp_amd.pipeline import require_gpu
    h = Harness(require_gpu())
    h.choose_side(L)
    return h


def _fid(fill):
    return f"fill{fill:02X}"


fills = pytest.mark.parametrize("fill", FILLS, ids=[_fid(f) for f in FILLS])


def _idx(rng, n):
    return rng.choice(5, size=n, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---------------------------------------------------------------------------------------------------------- the control
def test_positive_control(H):
    """dgrp_encode with the null stream while its producer sits behind the delay on the side stream reads the poison (all 'N': class
    4 everywhere): the trap works, without touching the library, on the stream pair every test of this module uses."""
    print("positive control per pool stream:", H.control)
    assert H.side is not None, f"the control tripped on none of {len(H.pool)} side streams (hardware queues shared with the null stream?): {H.control}"
    hit = H.control[H.pool.index(H.side)]
    assert hit["producer_still_delayed"] and hit["read_poison"] and not hit["read_real"]


# ---------------------------------------------------------------------------------------------------------- async: A2 / A3 / A6
@fills
def test_async_encode_onehot(H, L, orc, fill):
    n = 5003
    rng = np.random.default_rng(1)
    real = rng.choice(np.frombuffer(b"ACGTNacgtnRY*", np.uint8), size=n)
    poison = np.full(n, ord("N"), np.uint8)
    want = orc.encode_idx(real.tobytes())
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_encode(b["seq"].data_ptr(), n, b["idx"].data_ptr(), s), None),
                     {"seq": (real, poison)}, {"idx": np.full(n, fill, np.uint8)}, fill=fill)
    np.testing.assert_array_equal(late["idx"], want)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_onehot(b["seq"].data_ptr(), n, b["oh"].data_ptr(), s), None),
                     {"seq": (real, poison)}, {"oh": np.full((5, n), fill, np.uint8).view(np.int8)}, fill=fill)
    oh = np.zeros((5, n), np.int8)
    oh[want, np.arange(n)] = 1
    np.testing.assert_array_equal(late["oh"], oh)


@fills
def test_async_windows_onehot(H, L, orc, fill):
    T, s, w0, nw = 30, 4, 3, 40
    n = (w0 + nw - 1) * s + T + 5
    real = np.random.default_rng(2).integers(0, 5, n).astype(np.uint8)
    poison = np.full(n, 4, np.uint8)
    want = orc.windows_f32(real, T, s, w0, nw)
    for elem, dt in ((4, np.float32), (2, np.float16)):
        sent = np.full((nw, T, 5), fill, np.uint8).repeat(elem, axis=2).view(dt)
        late, *_ = H.run(lambda b, w, st, t: (L.dgrp_windows_onehot(b["idx"].data_ptr(), n, T, s, w0, nw, elem, b["out"].data_ptr(), st), None),
                         {"idx": (real, poison)}, {"out": sent}, fill=fill)
        np.testing.assert_array_equal(late["out"].astype(np.float32), want)


@fills
def test_async_get_max(H, L, orc, fill):
    b_, d0, d1, stride, rows = 9, 20, 5, 3, 60
    real = np.random.default_rng(3).random((b_, d0, d1)).astype(np.float32)
    poison = np.random.default_rng(30).random((b_, d0, d1)).astype(np.float32)
    init = np.random.default_rng(31).random((rows, d1)).astype(np.float32) * 0.5
    init_poison = np.full((rows, d1), 0.75, np.float32)
    want = orc.get_max(init.copy(), real, stride)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_get_max(b["out"].data_ptr(), rows, b["in"].data_ptr(), d0, d1, stride, b_, s), None),
                     {"in": (real, poison), "out": (init, init_poison)}, {"out": None}, fill=fill)
    np.testing.assert_array_equal(_bits(late["out"]), _bits(want))


# ---------------------------------------------------------------------------------------------------------- async: A7 / A8 / A11 / N2
def _probs(seed, n, c):
    p = np.random.default_rng(seed).random((n, c)).astype(np.float32) ** 3
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


@fills
def test_async_scores(H, L, orc, fill):
    n, c = 4099, 5
    real, poison = _probs(4, n, c), _probs(40, n, c)
    sc, cl = orc.scores(real)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_scores(b["p"].data_ptr(), n, c, b["sc"].data_ptr(), b["cl"].data_ptr(), s), None),
                     {"p": (real, poison)}, {"sc": np.full(n * 8, fill, np.uint8).view(np.float64), "cl": np.full(n, fill, np.uint8).view(np.int8)},
                     fill=fill)
    np.testing.assert_array_equal(late["sc"].view(np.int64), sc.view(np.int64))
    np.testing.assert_array_equal(late["cl"], cl)


@fills
def test_async_softmax_labels(H, L, orc, fill):
    n, c = 4099, 5
    real, poison = _probs(5, n, c), _probs(50, n, c)
    from numpy_post import np_softmax
    sm, cl = np_softmax(real)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_softmax_labels(b["p"].data_ptr(), n, c, b["sm"].data_ptr(), b["lab"].data_ptr(), w.data_ptr(), w.numel(), s), None),
                     {"p": (real, poison)}, {"sm": np.full((n, c), 7.0, np.float32), "lab": np.full(n, 0x55, np.int8)}, work_bytes=4096, fill=fill)
    np.testing.assert_array_equal(late["sm"].view(np.int32), sm.view(np.int32))
    np.testing.assert_array_equal(late["lab"], cl)


def _run_labels(seed, n, ncls=5):
    rng = np.random.default_rng(seed)
    return np.resize(np.repeat(rng.integers(0, ncls, size=n // 20 + 2), rng.integers(1, 60, size=n // 20 + 2)), n).astype(np.int8)


@fills
def test_async_segments(H, L, orc, fill):
    n, cap, offset = 6001, 1024, 17
    real, poison = _run_labels(6, n), _run_labels(60, n)
    want = orc.segments(real, offset)
    wb = L.dgrp_segments_workspace_bytes(n)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_segments(b["lab"].data_ptr(), n, offset, 3, b["rec"].data_ptr(), cap, b["cnt"].data_ptr(), w.data_ptr(), wb, s), None),
                     {"lab": (real, poison)}, {"rec": np.full(cap * SEG.itemsize, 0xAB, np.uint8), "cnt": np.full(1, -9, np.int64)}, work_bytes=wb, fill=fill)
    k = int(late["cnt"][0])
    assert k == len(want) and 0 < k <= cap
    rows = late["rec"][:k * SEG.itemsize].view(SEG)
    np.testing.assert_array_equal(np.stack([rows["start"], rows["end"], rows["label"]], 1), want)
    assert (rows["contig"] == 3).all() and (late["rec"][k * SEG.itemsize:] == 0xAB).all()


@fills
def test_async_confusion_and_filter(H, L, orc, fill):
    n, ncls, min_len = 50_003, 5, 9
    t_real, t_poison = _run_labels(7, n), _run_labels(70, n)
    p_real, p_poison = _run_labels(8, n), _run_labels(80, n)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_confusion_matrix(b["t"].data_ptr(), b["p"].data_ptr(), n, ncls, b["cnf"].data_ptr(), b["bad"].data_ptr(), s), None),
                     {"t": (t_real, t_poison), "p": (p_real, p_poison)},
                     {"cnf": np.full((ncls, ncls), -3, np.int64), "bad": np.full(1, 77, np.int32)}, fill=fill)
    np.testing.assert_array_equal(late["cnf"], orc.confusion_matrix(t_real, p_real))
    assert late["bad"][0] == 0
    want = orc.filter_segments(t_real, min_len).astype(np.int8)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_filter_segments(b["in"].data_ptr(), b["out"].data_ptr(), n, min_len, s), None),
                     {"in": (t_real, t_poison)}, {"out": np.full(n, fill, np.uint8).view(np.int8)}, fill=fill)
    np.testing.assert_array_equal(late["out"], want)
    late, *_ = H.run(lambda b, w, s, t: (L.dgrp_filter_segments(b["io"].data_ptr(), b["io"].data_ptr(), n, min_len, s), None),      # in place
                     {"io": (t_real, t_poison)}, {"io": None}, fill=fill)
    np.testing.assert_array_equal(late["io"], want)


# ---------------------------------------------------------------------------------------------------------- async: the forward family
# (family, cell, units, T, attention, C, step, level): one small model per recurrent kernel, without attention (modes 1 and 0) and,
# where the family has a pre-pass (mode 2), with it
MODELS = [
    ("wave", "GRU", 16, 40, False, 5, 4, 1), ("wave", "GRU", 16, 40, True, 5, 4, 1),
    ("split", "GRU", 80, 40, False, 5, 4, 1), ("split", "GRU", 32, 40, True, 5, 4, 1),
    ("split2", "GRU", 128, 40, False, 5, 4, 1), ("split2", "GRU", 128, 40, True, 5, 4, 1),
    ("stream64", "GRU", 160, 40, False, 5, 4, 1), ("stream64", "GRU", 192, 40, True, 5, 4, 1),
    ("stream", "LSTM", 48, 40, False, 5, 4, 1),
    ("lstm", "LSTM", 64, 40, False, 5, 4, 0),
    ("fused", "GRU", 32, 40, False, 5, 4, 0), ("fused", "GRU", 32, 40, True, 5, 4, 0),
    ("fp32", "GRU", 40, 40, False, 17, 4, 1), ("fp32", "GRU", 24, 40, True, 17, 4, 1),
]
NW, BATCH = 36, 7


def _mid(m):
    fam, cell, u, T, att, c, s, level = m
    return f"{fam}-{cell}{u}{'att' if att else ''}-C{c}-L{level}"


def _forward_cases():
    out = []
    for m in MODELS:
        for fill in (FILLS if m[0] == "wave" else FILLS[:1]):
            out.append(pytest.param(m, fill, id=f"{_mid(m)}-{_fid(fill)}"))
    return out


def _make_model(orc, m, seed=11, gain=1.5):
    from deepgrp_amd.pipeline import DeviceModel
    fam, cell, u, T, att, c, s, level = m
    if cell == "LSTM":
        w = orc.LSTMWeights.random(u, c, T, seed=seed, gain=gain)
        dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T, rnn="LSTM")
    else:
        w = orc.Weights.random(u, c, T, att, seed=seed, gain=gain)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            dm = DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, w.scale, vecsize=T)
    view = dm.view(level)
    for mode in ((2,) if att else (1, 0)):
        assert dm.plan(mode, s, handle=view).kernel == fam, f"mode {mode}: {dm.plan(mode, s, handle=view)} instead of {fam}"
    return w, dm, view


def _forward_suite(H, L, orc, m, fill, lanes):
    """dgrp_forward_windows, dgrp_forward_merge and dgrp_forward_merge_record of one model behind the late producer."""
    fam, cell, u, T, att, c, s, level = m
    w, dm, view = _make_model(orc, m)
    try:
        N = T + NW * s
        assert orc.window_count(N, T, s) == NW
        real, poison = _idx(np.random.default_rng(u + c), N), np.full(N, 4, np.uint8)
        want = (orc.lstm_forward if cell == "LSTM" else orc.nn_forward)(real, w, s, 0, NW, np.float64)
        tol = 1e-3 if level == 0 else 5e-5 if fam == "fp32" else 1e-5
        zeros, junk = np.zeros((N, c), np.float32), np.full((N, c), 0.75, np.float32)
        if not lanes:
            wb = max(L.dgrp_forward_workspace_bytes(view, NW), 256)
            late, *_ = H.run(lambda b, wk, st, t: (L.dgrp_forward_windows(view, b["idx"].data_ptr(), N, s, 0, NW, b["probs"].data_ptr(), wk.data_ptr(), wb, st), None),
                             {"idx": (real, poison)}, {"probs": np.full((NW, T, c), 7.0, np.float32)}, work_bytes=wb, fill=fill)
            probs = late["probs"]
            err = float(np.abs(probs - want).max())
            print(f"{_mid(m)}: max |dp| = {err:.2e}")
            assert err < tol
            merged_want = orc.merge_all(probs, N, s, BATCH)
            # the caller zeroes d_out in front of the call: that memset is late too (the poison holds 0.75 everywhere)
            late, *_ = H.run(lambda b, wk, st, t: (L.dgrp_forward_merge(view, b["idx"].data_ptr(), N, s, BATCH, 0, NW, b["out"].data_ptr(), wk.data_ptr(), wb, st), None),
                             {"idx": (real, poison), "out": (zeros, junk)}, {"out": None}, work_bytes=wb, fill=fill)
            np.testing.assert_array_equal(late["out"].view(np.uint32), merged_want.view(np.uint32))
        else:
            probs = dm.forward_windows(dev_of(real, H.dev), s, 0, NW, handle=view).cpu().numpy()
            merged_want = orc.merge_all(probs, N, s, BATCH)
        wr = max(L.dgrp_forward_merge_record_workspace_bytes(view, N, s), 256)
        if lanes:
            assert wr >= 3 * L.dgrp_forward_workspace_bytes(view, 16) and NW > 16 * 2
        late, *_ = H.run(lambda b, wk, st, t: (L.dgrp_forward_merge_record(view, b["idx"].data_ptr(), N, s, BATCH, b["out"].data_ptr(), wk.data_ptr(), wr, st), None),
                         {"idx": (real, poison), "out": (zeros, junk)}, {"out": None}, work_bytes=wr, fill=fill)
        np.testing.assert_array_equal(late["out"].view(np.uint32), merged_want.view(np.uint32))
        assert np.abs(late["out"] - orc.merge_all(want.astype(np.float32), N, s, BATCH)).max() < tol
    finally:
        L.dgrp_model_destroy(view)
        dm.close()


@pytest.mark.parametrize("m,fill", _forward_cases())
def test_async_forward(H, L, orc, m, fill, monkeypatch):
    monkeypatch.delenv("DGRP_LANE_CHUNK", raising=False)
    _forward_suite(H, L, orc, m, fill, lanes=False)


def _lane_cases():
    att = [x for x in MODELS if x[4] and x[0] != "fp32"]
    return [pytest.param(m, fill, id=f"{_mid(m)}-{_fid(fill)}") for m in att for fill in (FILLS if m[0] == "wave" else FILLS[:1])]


@pytest.mark.parametrize("m,fill", _lane_cases())
def test_async_forward_merge_record_on_lanes(H, L, orc, m, fill, monkeypatch):
    """The record's chunks alternate between the library's three lane streams (forced with DGRP_LANE_CHUNK as test_lanes_merge_identical
    does): the lanes must start behind the caller's stream (late d_idx, late zeroing of d_out) and be joined back into it (the clone)."""
    monkeypatch.setenv("DGRP_LANE_CHUNK", "16")
    _forward_suite(H, L, orc, m, fill, lanes=True)


@pytest.mark.parametrize("m", [MODELS[0], MODELS[1], MODELS[9], MODELS[12]], ids=_mid)
@fills
def test_async_forward_windows_reference(H, L, orc, m, fill):
    fam, cell, u, T, att, c, s, level = m
    w, dm, view = _make_model(orc, m)
    try:
        nw = 12
        N = T + nw * s
        real, poison = _idx(np.random.default_rng(u), N), np.full(N, 4, np.uint8)
        want = (orc.lstm_forward if cell == "LSTM" else orc.nn_forward)(real, w, s, 0, nw, np.float64)
        wb = max(L.dgrp_forward_reference_workspace_bytes(dm.handle, nw), 256)
        late, *_ = H.run(lambda b, wk, st, t: (L.dgrp_forward_windows_reference(dm.handle, b["idx"].data_ptr(), N, s, 0, nw, b["probs"].data_ptr(), wk.data_ptr(), wb, st), None),
                         {"idx": (real, poison)}, {"probs": np.full((nw, T, c), 7.0, np.float32)}, work_bytes=wb, fill=fill)
        assert np.abs(late["probs"] - want).max() < 5e-5
    finally:
        L.dgrp_model_destroy(view)
        dm.close()


# ---------------------------------------------------------------------------------------------------------- async: training
@fills
def test_async_train_step(H, L, fill):
    """dgrp_train_step behind the late producer.  The poison is another valid batch of the same shapes (other weights, a record of N,
    an all-background truth, starts of 0, masks of 1).  A workspace of 0xFF is NaN in every float: a workspace float that is read
    before this call wrote it shows in the gradients.  The harness proves late == idle; the checker proves both are right."""
    import train_oracle as tro
    from deepgrp_amd import synthetic
    from deepgrp_amd.training import flatten_weights, unflatten_weights
    units, T, batch, classes = 20, 7, 17, 5
    case = tro.make_case(units, T, batch, classes, True, seed=units + T + batch)
    n = case["idx"].size
    params = flatten_weights(case["weights"])
    other = flatten_weights(synthetic.synthetic_weights(units, classes, True, seed=99))
    background = np.zeros_like(case["truth"])
    background[0] = 1
    inputs = {"params": (params, other), "idx": (case["idx"], np.full(n, 4, np.uint8)), "truth": (case["truth"], background),
              "starts": (case["starts"], np.zeros(batch, np.int64)), "masks": (case["masks"], np.ones((batch, 2, 5), np.float32))}
    wb = L.dgrp_train_workspace_bytes(T, units, classes, 1, batch)
    assert wb > 0 and L.dgrp_train_param_count(units, classes, 1) == params.size

    def call(b, wk, st, t):
        return L.dgrp_train_step(T, units, classes, 1, b["params"].data_ptr(), b["idx"].data_ptr(), b["truth"].data_ptr(), n,
                                 b["starts"].data_ptr(), batch, b["masks"].data_ptr(), b["loss"].data_ptr(), b["grads"].data_ptr(),
                                 wk.data_ptr(), wb, st), None
    late, *_ = H.run(call, inputs, {"loss": np.full(1, 7.0, np.float32), "grads": np.full(params.size, 7.0, np.float32)},
                     work_bytes=wb, fill=fill)
    args = (case["weights"], case["idx"], case["truth"], case["starts"], T, case["masks"])
    l64, g64, _ = tro.loss_and_grads(*args, torch.float64)
    l32, g32, _ = tro.loss_and_grads(*args, torch.float32)
    e, e32 = abs(float(late["loss"][0]) - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    print(f"loss: hip {e:.3e} float32 {e32:.3e}")
    assert e <= tro.bound(e32)
    grads = unflatten_weights(late["grads"], units, classes, True)
    for name, want in g64.items():
        e, e32 = tro.rel_err(grads[name], want), tro.rel_err(g32[name], want)
        print(f"{name}: hip {e:.3e} float32 {e32:.3e}")
        assert e <= tro.bound(e32), f"{name}: {e:.3e} > {tro.bound(e32):.3e}"


@pytest.mark.parametrize("kind", ("RMSprop", "Adam"))
@fills
def test_async_optimizer_step(H, L, fill, kind):
    """dgrp_optimizer_step has no workspace: parameters and both states are in/out buffers, and the poison of all three is the fill
    (0xFF: NaN; 0x00: the state of a first step; 0xA5: small negative numbers), late-overwritten by the real values."""
    import train_oracle as tro
    from deepgrp_amd.training import OPTIMIZERS
    count, step, lr, eps = 1000, 3, 1e-3, 1e-7
    rho, momentum = (0.9, 0.9) if kind == "RMSprop" else (0.999, 0.9)
    rng = np.random.default_rng(19)
    w = rng.normal(size=count).astype(np.float32)
    g = rng.normal(scale=0.1, size=count).astype(np.float32)
    s1 = rng.normal(scale=0.03, size=count).astype(np.float32) if kind == "Adam" else (0.01 * rng.random(count) + 1e-4).astype(np.float32)
    s2 = (0.01 * rng.random(count) + 1e-4).astype(np.float32) if kind == "Adam" else rng.normal(scale=0.003, size=count).astype(np.float32)
    junk = np.full(count * 4, fill, np.uint8).view(np.float32)
    late, *_ = H.run(lambda b, wk, st, t: (L.dgrp_optimizer_step(OPTIMIZERS[kind.lower()], b["w"].data_ptr(), b["g"].data_ptr(), b["s1"].data_ptr(),
                                                                 b["s2"].data_ptr(), count, lr, rho, momentum, eps, step, st), None),
                     {"w": (w, junk), "g": (g, np.full(count, 0.5, np.float32)), "s1": (s1, junk), "s2": (s2, junk)},
                     {"w": None, "s1": None, "s2": None}, fill=fill)
    ref = {}
    for f in (np.float64, np.float32):
        a = (w.astype(f), g, s1.astype(f), s2.astype(f))
        ref[f] = tro.rmsprop_step(*a, lr, rho, momentum, eps, f) if kind == "RMSprop" else tro.adam_step(*a, lr, momentum, rho, eps, step, f)
    for name, want, f32 in zip(("w", "s1", "s2"), ref[np.float64], ref[np.float32]):
        e, e32 = tro.rel_err(late[name], want), tro.rel_err(f32, want)
        print(f"{kind} {name}: hip {e:.3e} float32 {e32:.3e}")
        assert e <= tro.bound(e32), f"{name}: {e:.3e} > {tro.bound(e32):.3e}"


# ---------------------------------------------------------------------------------------------------------- synchronising: FASTA
def _wrap(seq: bytes, width=60, nl=b"\n"):
    return nl.join(seq[i:i + width] for i in range(0, len(seq), width)) + nl


def _seq(rng, n):
    return rng.choice(np.frombuffer(b"ACGTNacgtnRY", np.uint8), size=n).tobytes()


def _want_record(orc, body: bytes):
    seq = body.replace(b"\r", b"").replace(b"\n", b"")
    st, kept = orc.strip_n(seq.upper())
    lead = len(seq) - len(seq.lstrip(b"Nn"))
    assert lead == st or kept < 0
    return seq, lead, kept


@fills
def test_sync_fasta_encode(H, L, orc, fill):
    rng = np.random.default_rng(9)
    body = _wrap(b"NNnn" + _seq(rng, 3000) + b"nN")
    nb = len(body)
    real, poison = np.frombuffer(body, np.uint8), np.full(nb, ord("N"), np.uint8)
    wb = L.dgrp_fasta_workspace_bytes(nb)

    def call(b, wk, st, t):
        info = (C.c_int64 * 4)(-1, -1, -1, -1)
        rc = L.dgrp_fasta_encode(b["raw"].data_ptr(), nb, b["idx"].data_ptr(), info, wk.data_ptr(), wb, st)
        return rc, list(info)
    late, info, _, info_idle = H.run(call, {"raw": (real, poison)}, {"idx": np.full(nb, 0x77, np.uint8)}, work_bytes=wb, fill=fill, sync=True)
    seq, lead, kept = _want_record(orc, body)
    assert info == info_idle and info[0] == 1 and info[1] == len(seq) and info[2] == lead and info[3] == kept
    np.testing.assert_array_equal(late["idx"][lead:lead + kept], orc.encode_idx(seq[lead:lead + kept]))


@fills
def test_sync_fasta_encode_batch_and_chunks(H, L, orc, fill):
    rng = np.random.default_rng(10)
    bodies = [_wrap(_seq(rng, n), 70, nl) for n, nl in ((1, b"\n"), (777, b"\n"), (2500, b"\r\n"), (64, b"\n"), (1203, b"\n"))]
    text, off = b"", []
    for k, b_ in enumerate(bodies):
        text += b">rec%d some text\n" % k
        off.append(len(text))
        text += b_
    real = np.frombuffer(text, np.uint8)
    poison = np.full(real.size, ord("N"), np.uint8)
    h_off, h_len = np.array(off, np.int64), np.array([len(b_) for b_ in bodies], np.int64)
    nrec = len(bodies)
    wb = L.dgrp_fasta_batch_workspace_bytes(nrec, int(h_len.sum()))

    def call(b, wk, st, t):
        info = np.full((nrec, 4), -1, np.int64)
        rc = L.dgrp_fasta_encode_batch(b["raw"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), b["idx"].data_ptr(), info.ctypes.data, wk.data_ptr(), wb, st)
        return rc, info
    late, info, _, info_idle = H.run(call, {"raw": (real, poison)}, {"idx": np.full(real.size, 0x77, np.uint8)}, work_bytes=wb, fill=fill, sync=True,
                                     tables={"off": h_off, "len": h_len})
    np.testing.assert_array_equal(info, info_idle)
    for r, body in enumerate(bodies):
        seq, lead, kept = _want_record(orc, body)
        assert info[r].tolist() == [1, len(seq), lead, kept], r
        a, k = off[r] + lead, max(kept, 0)
        np.testing.assert_array_equal(late["idx"][a:a + k], orc.encode_idx(seq[lead:lead + k]))
    # ---- dgrp_fasta_chunks on the same file: the table of test_fasta_chunks_table's definition
    starts = [0] + [i + 1 for i in range(len(text) - 1) if text[i] == 10 and text[i + 1] == 62]
    lfs = [text.find(b"\n", a) for a in starts]
    cap = len(starts)
    wc = L.dgrp_fasta_chunks_workspace_bytes(cap)
    poison2 = np.frombuffer((b">x\n" + b"N" * 61) * (real.size // 64 + 1), np.uint8)[:real.size].copy()      # another valid file: more chunks

    def chunks(b, wk, st, t):
        h_st, h_lf, n = np.full(cap, -7, np.int64), np.full(cap, -7, np.int64), C.c_int64(-1)
        rc = L.dgrp_fasta_chunks(b["raw"].data_ptr(), real.size, cap, h_st.ctypes.data, h_lf.ctypes.data, C.byref(n), wk.data_ptr(), wc, st)
        return rc, (n.value, h_st.tolist(), h_lf.tolist())
    _, got, _, got_idle = H.run(chunks, {"raw": (real, poison2)}, {}, work_bytes=wc, fill=fill, sync=True)
    assert got == got_idle == (len(starts), starts, lfs)


@pytest.mark.parametrize("with_rows", (True, False), ids=("rows", "zero-rows"))
@fills
def test_sync_fasta_mask_batch(H, L, fill, with_rows):
    from test_gpu_mask import brute_mask
    rng = np.random.default_rng(11)
    seqs = [_seq(rng, n) for n in (500, 3000, 61)]
    bodies = [_wrap(sq, 60, nl) for sq, nl in zip(seqs, (b"\n", b"\r\n", b"\n"))]
    text, off = b"", []
    for k, b_ in enumerate(bodies):
        text += b">r%d\n" % k
        off.append(len(text))
        text += b_
    real = np.frombuffer(text, np.uint8)
    poison = np.full(real.size, ord("c"), np.uint8)
    rowsets = []
    for sq in seqs:
        rows, p = [], 3
        while with_rows and p + 40 < len(sq):
            rows.append((p, p + int(rng.integers(1, 40)), int(rng.integers(1, 5))))
            p = rows[-1][1] + int(rng.integers(0, 90))
        rowsets.append(rows)
    flat = segs([(a, b_, lab, k) for k, rows in enumerate(rowsets) for a, b_, lab in rows])
    row_off = np.cumsum([0] + [len(r) for r in rowsets]).astype(np.int64)
    nrec, nrows = len(bodies), len(flat)
    h_off, h_len = np.array(off, np.int64), np.array([len(b_) for b_ in bodies], np.int64)
    wb = L.dgrp_fasta_mask_workspace_bytes(nrec, int(h_len.sum()), nrows)
    classes = (1, 3)
    bits = sum(1 << c for c in classes)
    inputs = {"raw": (real, poison)}
    if nrows:
        other = flat.copy()
        other["label"] = 1 + other["label"] % 4                                # in-range rows of other classes
        inputs["rows"] = (flat.view(np.uint8), other.view(np.uint8))

    def call(b, wk, st, t):
        rc = L.dgrp_fasta_mask_batch(b["raw"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), b["rows"].data_ptr() if nrows else None,
                                     i64ptr(t["row_off"]), 0, bits, b["out"].data_ptr(), wk.data_ptr(), wb, st)
        return rc, None
    # "stream-ordered after the row check": the masked bytes are ready behind the stream, not necessarily at return
    late, *_ = H.run(call, inputs, {"out": np.full(real.size, 7, np.uint8)}, work_bytes=wb, fill=fill, sync=True, drained=False,
                     tables={"off": h_off, "len": h_len, "row_off": row_off})
    got = late["out"].tobytes()
    outside = np.ones(real.size, bool)
    for k, body in enumerate(bodies):
        assert got[off[k]:off[k] + len(body)] == brute_mask(b">h\n" + body, [rowsets[k]], "soft", classes)[3:], k
        outside[off[k]:off[k] + len(body)] = False
    assert (late["out"][outside] == 7).all()


# ---------------------------------------------------------------------------------------------------------- synchronising: MSS
def _mss_input(seed, n):
    rng = np.random.default_rng(seed)
    lab = np.resize(np.repeat(rng.integers(0, 5, size=n // 40 + 2), rng.integers(1, 120, size=n // 40 + 2)), n)
    m = np.clip(rng.uniform(0.4, 0.999, n), None, 0.99).astype(np.float32)
    t = np.abs(np.log(m / (1 - m)))
    return np.where(lab > 0, t, -10 * t).astype(np.float64), lab.astype(np.int8)


@pytest.mark.parametrize("ml,xd", [(3, 10), (0, -1)], ids=("stretches", "one-stretch"))
@fills
def test_sync_mss_labels_and_segments_host(H, L, orc, fill, ml, xd):
    n = 20_011
    (s_real, c_real), (s_poison, c_poison) = _mss_input(12, n), _mss_input(120, n)
    want, want_segs = orc.find_mss_labels(s_real, c_real, 5, ml, xd, return_segments=True)
    wb = L.dgrp_mss_workspace_bytes(n)

    def call(b, wk, st, t):
        rc = L.dgrp_mss_labels(b["s"].data_ptr(), b["c"].data_ptr(), n, 5, ml, xd, b["lab"].data_ptr(), b["nseg"].data_ptr(), wk.data_ptr(), wb, st)
        if rc:
            return rc, None
        # the segments of this call, read back by the synchronous companion while the labels are still being voted on `st`
        buf, cnt = np.full((len(want_segs) + 8, 2), -1, np.int32), C.c_int64(-1)
        rc = L.dgrp_mss_segments_host(wk.data_ptr(), wb, buf.ctypes.data, len(buf), C.byref(cnt))
        return rc, (cnt.value, buf[:max(cnt.value, 0)].copy())
    # the synchronisation is inside the call (the fixed-point loop): the vote is enqueued behind it
    late, (cnt, pairs), *_ = H.run(call, {"s": (s_real, s_poison), "c": (c_real, c_poison)},
                                   {"lab": np.full(n, 0x55, np.int8), "nseg": np.full(1, -9, np.int64)}, work_bytes=wb, fill=fill, sync=True, drained=False)
    np.testing.assert_array_equal(late["lab"], want)
    assert int(late["nseg"][0]) == len(want_segs) == cnt
    np.testing.assert_array_equal(pairs, np.array([(a, b) for a, b, _ in want_segs], np.int32).reshape(-1, 2))


@fills
def test_sync_mss_labels_batch(H, L, orc, fill):
    lens = [1, 63, 64, 65, 1000, 4097, 300, 2222]
    starts = np.zeros(len(lens) + 1, np.int64)
    for i, n in enumerate(lens):
        starts[i + 1] = starts[i] + (n + 63) // 64 * 64
    total = int(starts[-1])
    S, cls, Sp, clsp, want = np.zeros(total), np.zeros(total, np.int8), np.zeros(total), np.zeros(total, np.int8), np.zeros(total, np.int8)
    for i, n in enumerate(lens):
        a = int(starts[i])
        S[a:a + n], cls[a:a + n] = _mss_input(200 + i, n)
        Sp[a:a + n], clsp[a:a + n] = _mss_input(300 + i, n)
        want[a:a + n] = orc.find_mss_labels(S[a:a + n], cls[a:a + n], 5, 3, 10)
    wb = L.dgrp_mss_batch_workspace_bytes(total, len(lens))

    def call(b, wk, st, t):
        return L.dgrp_mss_labels_batch(b["s"].data_ptr(), b["c"].data_ptr(), total, len(lens), i64ptr(t["start"]), 5, 3, 10, b["lab"].data_ptr(),
                                       wk.data_ptr(), wb, st), None
    late, *_ = H.run(call, {"s": (S, Sp), "c": (cls, clsp)}, {"lab": np.full(total, 0x55, np.int8)}, work_bytes=wb, fill=fill, sync=True,
                     tables={"start": starts})
    for i, n in enumerate(lens):
        a = int(starts[i])
        np.testing.assert_array_equal(late["lab"][a:a + n], want[a:a + n], err_msg=f"record {i}")


# ---------------------------------------------------------------------------------------------------------- synchronising: tracks
@fills
def test_sync_track_text(H, L, fill):
    from deepgrp_amd.tracks import reference_text
    n, c, cls, digits, bin_, offset, name = 5000, 5, 2, 2, 7, 123, b"chr\xce\xb1 1"
    real, poison = _probs(13, n, c), _probs(130, n, c)
    real[1000:1500, cls] = 0.0
    real[2000:2600, cls] = 0.5
    want = reference_text(real[:, cls], offset, name, digits, bin_)
    cap = len(want) + 64
    wb = L.dgrp_track_workspace_bytes(n, bin_)

    def call(b, wk, st, t):
        total = C.c_int64(-1)
        nm = C.create_string_buffer(name, len(name))
        rc = L.dgrp_track_text(b["p"].data_ptr(), n, c, cls, digits, bin_, offset, nm, len(name), b["text"].data_ptr(), cap, C.byref(total),
                               wk.data_ptr(), wb, st)
        C.memset(nm, ord("#"), len(name))                                     # the name is a host table too
        return rc, total.value
    late, total, _, total_idle = H.run(call, {"p": (real, poison)}, {"text": np.full(cap, 0x5A, np.uint8)}, work_bytes=wb, fill=fill, sync=True)
    assert total == total_idle == len(want)
    assert late["text"][:total].tobytes() == want and (late["text"][total:] == 0x5A).all()


@fills
def test_sync_track_text_batch(H, L, fill):
    from deepgrp_amd.tracks import reference_text
    c, digits, bin_ = 5, 2, 7
    n = np.array([1, 65, 4097], np.int64)
    row0 = np.r_[0, np.cumsum((n[:-1] + 63) // 64 * 64)].astype(np.int64)
    rows = int(row0[-1] + n[-1])
    spos = np.array([0, 10 ** 11 + 3, 123], np.int64)
    names = [b"a", b"chr\xce\xb1 1", b"scaffold_3"]
    noff = np.r_[0, np.cumsum([len(x) for x in names])].astype(np.int64)
    blob = b"".join(names)
    cls = np.array([0, 3], np.int32)
    real, poison = _probs(13, rows, c), _probs(130, rows, c)
    real[row0[2] + 1000:row0[2] + 1500, 0] = 0.0
    real[row0[2] + 2000:row0[2] + 2600, 3] = 0.5
    want = [b"".join(reference_text(real[row0[r]:row0[r] + n[r], k], int(spos[r]), names[r], digits, bin_) for r in range(len(n))) for k in cls]
    total = sum(len(w) for w in want)
    cap = total + 64
    wb = L.dgrp_track_batch_workspace_bytes(len(n), n.ctypes.data, spos.ctypes.data, bin_, len(cls), len(blob))

    def call(b, wk, st, t):
        off = np.full(len(cls) + 1, -1, np.int64)
        nm = C.create_string_buffer(blob, len(blob))
        rc = L.dgrp_track_text_batch(b["p"].data_ptr(), c, len(n), i64ptr(t["row0"]), i64ptr(t["n"]), i64ptr(t["spos"]), nm, i64ptr(t["noff"]),
                                     t["cls"].ctypes.data, len(cls), digits, bin_, b["text"].data_ptr(), cap, off.ctypes.data, wk.data_ptr(), wb, st)
        C.memset(nm, ord("#"), len(blob))                                     # the names are a host table too
        return rc, off.tolist()
    late, off, _, off_idle = H.run(call, {"p": (real, poison)}, {"text": np.full(cap, 0x5A, np.uint8)}, work_bytes=wb, fill=fill, sync=True,
                                   tables={"row0": row0, "n": n.copy(), "spos": spos, "noff": noff, "cls": cls})
    assert off == off_idle == np.r_[0, np.cumsum([len(w) for w in want])].tolist()
    assert late["text"][:total].tobytes() == b"".join(want) and (late["text"][total:] == 0x5A).all()
    assert total > 3000


# ---------------------------------------------------------------------------------------------------------- synchronising: predict
def _rows3(a):
    return np.stack([a["start"], a["end"], a["label"]], 1).reshape(-1, 3)


PREDICT_MODELS = [MODELS[0], MODELS[1], MODELS[9]]
# every model with the 0xA5 workspace, the other fills on the first one
PREDICT_CASES = [pytest.param(m, fill, id=f"{_mid(m)}-{_fid(fill)}") for m in PREDICT_MODELS for fill in (FILLS if m is MODELS[0] else FILLS[:1])]


@pytest.mark.parametrize("m,fill", PREDICT_CASES)
@pytest.mark.parametrize("use_mss", (1, 0), ids=("mss", "softmax"))
def test_sync_predict_record(H, L, orc, m, use_mss, fill):
    fam, cell, u, T, att, c, s, level = m
    w, dm, view = _make_model(orc, m, gain=3.0)
    try:
        N, cap, offset = 2003, 2048, 17
        real, poison = _idx(np.random.default_rng(14), N), np.full(N, 4, np.uint8)
        nwin = orc.window_count(N, T, s)
        probs = dm.forward_windows(dev_of(real, H.dev), s, 0, nwin, handle=view).cpu().numpy()
        want = orc.segments(orc.labels_from_merged(orc.merge_all(probs, N, s, BATCH), 4, 6, bool(use_mss)), offset)
        wb = L.dgrp_record_workspace_bytes(view, N, s, use_mss)

        def call(b, wk, st, t):
            cnt = c_i64()
            rc = L.dgrp_predict_record(view, b["idx"].data_ptr(), N, s, BATCH, 4, 6, use_mss, offset, 3, b["rec"].data_ptr(), cap, C.byref(cnt),
                                       wk.data_ptr(), wb, st)
            return rc, cnt.value
        late, cnt, _, cnt_idle = H.run(call, {"idx": (real, poison)}, {"rec": np.full(cap * SEG.itemsize, 0xAB, np.uint8)}, work_bytes=wb, fill=fill, sync=True)
        assert cnt == cnt_idle == len(want) and 0 < cnt <= cap
        rows = late["rec"][:cnt * SEG.itemsize].view(SEG)
        np.testing.assert_array_equal(_rows3(rows), want)
        assert (rows["contig"] == 3).all() and (late["rec"][cnt * SEG.itemsize:] == 0xAB).all()
    finally:
        L.dgrp_model_destroy(view)
        dm.close()


def _batch_tables(rng, lens):
    offs, pos = [], 0
    for n in lens:
        pos += int(rng.integers(0, 20))
        offs.append(pos)
        pos += n
    return np.array(offs, np.int64), pos + 5


@pytest.mark.parametrize("m,fill", PREDICT_CASES)
def test_sync_predict_batch(H, L, orc, m, fill):
    fam, cell, u, T, att, c, s, level = m
    w, dm, view = _make_model(orc, m, gain=3.0)
    try:
        rng = np.random.default_rng(15)
        lens = np.array([1, T - 1, T, T + 1, 64, T + 16 * s, 1500, 333], np.int64)
        offs, size = _batch_tables(rng, lens)
        real, poison = _idx(rng, size), np.full(size, 4, np.uint8)
        spos = rng.integers(0, 1000, len(lens)).astype(np.int64)
        contig = np.arange(10, 10 + len(lens), dtype=np.int32)
        want = []
        for r, n in enumerate(lens):
            idx = real[offs[r]:offs[r] + n]
            nwin = orc.window_count(int(n), T, s)
            probs = dm.forward_windows(dev_of(idx, H.dev), s, 0, nwin, handle=view).cpu().numpy() if nwin else np.zeros((0, T, c), np.float32)
            for a, b_, lab in orc.segments(orc.labels_from_merged(orc.merge_all(probs, int(n), s, BATCH), 4, 6, True), int(spos[r])):
                want.append((a, b_, lab, contig[r]))
        want = segs(want)
        cap = 1024
        wb = L.dgrp_batch_workspace_bytes(view, len(lens), lens.ctypes.data, s)

        def call(b, wk, st, t):
            cnt = c_i64()
            rc = L.dgrp_predict_batch(view, b["idx"].data_ptr(), len(lens), i64ptr(t["off"]), i64ptr(t["n"]), i64ptr(t["spos"]), t["contig"].ctypes.data, s,
                                      BATCH, 4, 6, b["rec"].data_ptr(), cap, C.byref(cnt), wk.data_ptr(), wb, st)
            return rc, cnt.value
        late, cnt, _, cnt_idle = H.run(call, {"idx": (real, poison)}, {"rec": np.full(cap * SEG.itemsize, 0xAB, np.uint8)}, work_bytes=wb, fill=fill, sync=True,
                                       tables={"off": offs, "n": lens.copy(), "spos": spos, "contig": contig})
        assert cnt == cnt_idle == len(want) and len(want) > len(lens)
        np.testing.assert_array_equal(late["rec"][:cnt * SEG.itemsize].view(SEG), want)
    finally:
        L.dgrp_model_destroy(view)
        dm.close()


# ---------------------------------------------------------------------------------------------------------- synchronising: evaluate
@fills
def test_sync_paint_rows_and_row_hits(H, L, fill):
    from test_gpu_evaluate import brute_hits, brute_paint
    rng = np.random.default_rng(16)
    ln, org = [0, 17, 4097, 900], [0, 40, 1000, 7]
    off, p = [], 5
    for n in ln:
        off.append(p)
        p += n + int(rng.integers(0, 30))
    size = p + 9
    rows = []
    for n, o in zip(ln, org):
        rr = [(int(a), int(a) + int(rng.integers(0, 300)), int(rng.integers(1, 6))) for a in rng.integers(max(o - 20, 0), o + n + 20, 25)]
        rows.append(rr + [(o, o, 2), (0, o + n + 500, 5)])
    flat = segs([(a, b_, lab, 0) for rr in rows for a, b_, lab in rr])
    other = flat.copy()
    other["label"] = 1 + other["label"] % 5
    ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    nrec, nrows = len(ln), len(flat)
    tabs = {"off": np.array(off, np.int64), "len": np.array(ln, np.int64), "org": np.array(org, np.int64), "ro": ro}
    wb = L.dgrp_eval_workspace_bytes(nrec, nrows)
    buf = rng.integers(-128, 0, size).astype(np.int8)                          # sentinel: no valid label
    buf_poison = rng.integers(6, 100, size).astype(np.int8)

    def paint(b, wk, st, t):
        return L.dgrp_paint_rows_batch(b["lab"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), b["rows"].data_ptr(), i64ptr(t["ro"]),
                                       wk.data_ptr(), wb, st), None
    # "the check synchronises the stream once": the painting is ordered behind it on the stream
    late, *_ = H.run(paint, {"lab": (buf, buf_poison), "rows": (flat.view(np.uint8), other.view(np.uint8))}, {"lab": None}, work_bytes=wb, fill=fill,
                     sync=True, drained=False, tables=tabs)
    np.testing.assert_array_equal(late["lab"], brute_paint(buf, off, ln, org, rows))
    labels = rng.integers(0, 6, size).astype(np.int8)
    labels_poison = rng.integers(0, 6, size).astype(np.int8)

    def hits(b, wk, st, t):
        return L.dgrp_row_hits_batch(b["lab"].data_ptr(), nrec, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["org"]), b["rows"].data_ptr(), i64ptr(t["ro"]),
                                     b["hits"].data_ptr(), wk.data_ptr(), wb, st), None
    late, *_ = H.run(hits, {"lab": (labels, labels_poison), "rows": (flat.view(np.uint8), other.view(np.uint8))}, {"hits": np.full(nrows, -5, np.int64)},
                     work_bytes=wb, fill=fill, sync=True, drained=False, tables=tabs)
    np.testing.assert_array_equal(late["hits"], brute_hits(labels, off, ln, org, rows))


# ---------------------------------------------------------------------------------------------------------- synchronising: gzip
def _member(data: bytes, level: int) -> bytes:
    from deepgrp_amd.gz import bgzf_member
    return bgzf_member(data, level)


@fills
def test_sync_inflate_batch(H, L, fill):
    from deepgrp_amd.gz import inflate_host, walk_members
    rng = np.random.default_rng(17)
    shared = _wrap(_seq(rng, 30_000))
    # the poison is another valid BGZF file of the SAME member layout: the first member (dynamic Huffman codes, matches) is shared,
    # the others are stored blocks (level 0: their size follows from the length alone) of different bytes
    tails = [[_seq(np.random.default_rng(seed + k), n) for k, n in enumerate((5000, 1, 20_000))] for seed in (170, 1700)]
    files = [b"".join([_member(shared, 6)] + [_member(t, 0) for t in tl]) for tl in tails]
    assert len(files[0]) == len(files[1]) and files[0] != files[1]
    real, poison = (np.frombuffer(f, np.uint8) for f in files)
    mem = walk_members(files[0])
    assert mem.kind == "bgzf" and np.array_equal(mem.data_off, walk_members(files[1]).data_off)
    nmem = int(mem.start.size)
    out_off = np.zeros(nmem + 1, np.int64)
    np.cumsum(mem.isize, out=out_off[1:])
    total = int(out_off[-1])
    want = shared + b"".join(tails[0])
    assert len(want) == total and zlib.decompressobj(31).decompress(files[0][:int(mem.start[1])]) == shared      # zlib's statement
    assert bytes(inflate_host(files[0], "<real>", 1 << 30)) == want
    wb = L.dgrp_inflate_workspace_bytes(nmem)

    def call(b, wk, st, t):
        bad, reason = c_i64(), C.c_int(-1)
        rc = L.dgrp_inflate_batch(b["in"].data_ptr(), real.size, nmem, i64ptr(t["off"]), i64ptr(t["len"]), i64ptr(t["out_off"]), b["out"].data_ptr(), total,
                                  C.byref(bad), C.byref(reason), wk.data_ptr(), wb, st)
        return rc, (bad.value, reason.value)
    late, status, _, status_idle = H.run(call, {"in": (real, poison)}, {"out": np.full(total, 0x77, np.uint8)}, work_bytes=wb, fill=fill, sync=True,
                                         tables={"off": mem.data_off.copy(), "len": mem.data_len.copy(), "out_off": out_off})
    assert status == status_idle == (-1, 0)
    assert late["out"].tobytes() == want


@pytest.mark.parametrize("level", (0, 1))
@fills
def test_sync_bgzf_compress_level(H, L, fill, level):
    from deepgrp_amd.gz import bgzf_compress_host, inflate_host
    rng = np.random.default_rng(18)
    text = b"".join(b">c%d\n" % k + _wrap(_seq(rng, 3000)) * 4 for k in range(14))        # three members, repeats for level 1
    other = b"".join(b">d%d\n" % k + _wrap(_seq(rng, 3000)) * 4 for k in range(14))
    n = len(text)
    assert n == len(other) and n > 2 * 0xff00
    want = bgzf_compress_host(text, True, level)
    assert bytes(inflate_host(want, "<want>", 1 << 30)) == text
    cap = int(L.dgrp_bgzf_bound(n, 1))
    wb = int(L.dgrp_bgzf_workspace_bytes_level(n, level))

    def call(b, wk, st, t):
        got = c_i64()
        rc = L.dgrp_bgzf_compress_level(b["in"].data_ptr(), n, b["out"].data_ptr(), cap, C.byref(got), 1, level, wk.data_ptr(), wb, st)
        return rc, got.value
    late, got, _, got_idle = H.run(call, {"in": (np.frombuffer(text, np.uint8), np.frombuffer(other, np.uint8))}, {"out": np.full(cap, 0x77, np.uint8)},
                                   work_bytes=wb, fill=fill, sync=True)
    assert got == got_idle == len(want)
    assert late["out"][:got].tobytes() == want


# ---------------------------------------------------------------------------------------------------------- host threads
NTHREADS, ROUNDS = 4, 3


def test_threads_share_a_model(H, L, orc, monkeypatch):
    """Four host threads, each with a torch stream, a dgrp_model_view (levels 0 and 1 alternating), a workspace and records of its own,
    call through ctypes (which releases the GIL): rounds of dgrp_predict_record, one of dgrp_predict_batch, one with an attention model
    on forced lanes (the threads share the lane pool).  Every thread's rows are bit for bit those of the same calls made one after the
    other on one thread; the parent handles keep their level; dgrp_last_error and the kernel timer are the calling thread's own."""
    dev = H.dev
    s, cap = 4, 4096
    wp, plain, pv = _make_model(orc, MODELS[0], gain=3.0)
    wa, att, av = _make_model(orc, MODELS[1], gain=3.0)
    L.dgrp_model_destroy(pv)
    L.dgrp_model_destroy(av)
    T = plain.vecsize
    flags_before = (plain.kernel_flags, att.kernel_flags)
    streams = [torch.cuda.Stream(device=dev) for _ in range(NTHREADS)]
    views = [(plain.view(k % 2), att.view(k % 2)) for k in range(NTHREADS)]
    # ---- per thread: records of its own, the batch tables, the workspaces
    jobs = []
    for k in range(NTHREADS):
        rng = np.random.default_rng(900 + k)
        recs = [dev_of(_idx(rng, int(n)), dev) for n in rng.integers(600, 3000, ROUNDS)]
        lens = rng.integers(1, 900, 6).astype(np.int64)
        offs, size = _batch_tables(rng, lens)
        batch = {"idx": dev_of(_idx(rng, size), dev), "off": offs, "n": lens, "spos": rng.integers(0, 99, 6).astype(np.int64),
                 "contig": np.arange(6, dtype=np.int32) + 10 * k}
        lane_rec = dev_of(_idx(rng, T + 70 * s), dev)                          # 70 windows: more than one chunk of 16 per lane
        jobs.append({"recs": recs, "batch": batch, "lane_rec": lane_rec, "fw_idx": dev_of(_idx(rng, T + 40 * s), dev)})
    monkeypatch.setenv("DGRP_LANE_CHUNK", "16")                                # read per call; only attention models take lanes
    for k, j in enumerate(jobs):
        pvw, avw = views[k]
        need = [L.dgrp_record_workspace_bytes(pvw, r.numel(), s, 1) for r in j["recs"]]
        need.append(L.dgrp_batch_workspace_bytes(pvw, 6, j["batch"]["n"].ctypes.data, s))
        need.append(L.dgrp_record_workspace_bytes(avw, j["lane_rec"].numel(), s, 1))
        j["wb"] = int(max(need))
        j["work"] = torch.full((j["wb"],), 0xA5, dtype=torch.uint8, device=dev)
        j["rec"] = torch.empty(cap * SEG.itemsize, dtype=torch.uint8, device=dev)
        j["probs"] = torch.empty((40, T, 5), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def rows_of(j, cnt):
        assert 0 <= cnt <= cap
        return j["rec"][:cnt * SEG.itemsize].cpu().numpy().view(SEG).copy()

    def one_thread(k, stream_ptr, out):
        """The calls of thread k, in order; every call synchronises its stream, so the rows can be read right after it."""
        j, (pvw, avw) = jobs[k], views[k]
        b = j["batch"]
        for r in j["recs"]:
            cnt = c_i64()
            rc = L.dgrp_predict_record(pvw, r.data_ptr(), r.numel(), s, BATCH, 4, 6, 1, 5, k, j["rec"].data_ptr(), cap, C.byref(cnt), j["work"].data_ptr(),
                                       j["wb"], stream_ptr)
            assert rc == 0, last_error()
            out.append(rows_of(j, cnt.value))
        cnt = c_i64()
        rc = L.dgrp_predict_batch(pvw, b["idx"].data_ptr(), 6, i64ptr(b["off"]), i64ptr(b["n"]), i64ptr(b["spos"]), b["contig"].ctypes.data, s, BATCH, 4, 6,
                                  j["rec"].data_ptr(), cap, C.byref(cnt), j["work"].data_ptr(), j["wb"], stream_ptr)
        assert rc == 0, last_error()
        out.append(rows_of(j, cnt.value))
        cnt = c_i64()
        r = j["lane_rec"]
        rc = L.dgrp_predict_record(avw, r.data_ptr(), r.numel(), s, BATCH, 4, 6, 1, 5, k, j["rec"].data_ptr(), cap, C.byref(cnt), j["work"].data_ptr(),
                                   j["wb"], stream_ptr)
        assert rc == 0, last_error()
        out.append(rows_of(j, cnt.value))

    # ---- one after the other, on one thread and the default stream
    sequential = [[] for _ in range(NTHREADS)]
    for k in range(NTHREADS):
        one_thread(k, None, sequential[k])
    torch.cuda.synchronize()
    assert all(len(x) for rows in sequential for x in rows[:1]) and sum(len(x) for rows in sequential for x in rows) > 50

    # ---- the same calls on four threads at once; thread 1 also fails a call on purpose, thread 2 runs the kernel timer
    results = [[] for _ in range(NTHREADS)]
    notes = [dict() for _ in range(NTHREADS)]
    errors = []
    gate = threading.Barrier(NTHREADS)

    def worker(k):
        try:
            j, (pvw, _avw) = jobs[k], views[k]
            sp = streams[k].cuda_stream
            gate.wait(timeout=60)
            if k == 2:
                assert L.dgrp_kernel_timer_enable(1) == 0
            fw = j["fw_idx"]
            for _ in range(3):                                                 # one recurrent launch of 40 windows each (no attention)
                rc = L.dgrp_forward_windows(pvw, fw.data_ptr(), fw.numel(), s, 0, 40, j["probs"].data_ptr(), j["work"].data_ptr(), j["wb"], sp)
                assert rc == 0, last_error()
            if k == 2:
                ms, launches, windows = C.c_double(-1), C.c_int64(-1), C.c_int64(-1)
                assert L.dgrp_kernel_timer_read(C.byref(ms), C.byref(launches), C.byref(windows)) == 0
                notes[k]["timer"] = (launches.value, windows.value, ms.value)
                assert L.dgrp_kernel_timer_enable(0) == 0
            if k == 1:                                                         # a host-side refusal: nothing is launched
                rc = L.dgrp_forward_windows(pvw, fw.data_ptr(), fw.numel(), 0, 0, 40, j["probs"].data_ptr(), j["work"].data_ptr(), j["wb"], sp)
                notes[k]["bad_rc"] = rc
            one_thread(k, sp, results[k])
            notes[k]["err"] = L.dgrp_last_error()
            if k != 2:                                                         # never enabled here: whatever thread 2 timed is not theirs
                ms, launches, windows = C.c_double(-1), C.c_int64(-1), C.c_int64(-1)
                assert L.dgrp_kernel_timer_read(C.byref(ms), C.byref(launches), C.byref(windows)) == 0
                notes[k]["timer"] = (launches.value, windows.value, ms.value)
        except BaseException as e:                                             # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(e)))
            try:
                gate.abort()
            except Exception:                                                  # noqa: BLE001
                pass

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(NTHREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    torch.cuda.synchronize()
    assert not errors, errors
    for k in range(NTHREADS):
        assert len(results[k]) == len(sequential[k]) == ROUNDS + 2
        for r, (got, want) in enumerate(zip(results[k], sequential[k])):
            np.testing.assert_array_equal(got, want, err_msg=f"thread {k} round {r}")
    # the parents' level is untouched by the views
    assert (plain.kernel_flags, att.kernel_flags) == flags_before
    # errors are per thread: thread 1 sees its own refusal, the others never saw one of this round
    assert notes[1]["bad_rc"] == EINVAL and b"dgrp_forward" in notes[1]["err"]
    for k in (0, 2, 3):
        assert notes[k]["err"] == b"", (k, notes[k]["err"])
    # the timer is per thread: thread 2 enabled it around its 3 dgrp_forward_windows launches of 40 windows and reads exactly those,
    # while the other threads launched beside it; a read on a thread that never enabled it reports none
    for k in (0, 1, 3):
        assert notes[k]["timer"] == (0, 0, 0.0), (k, notes[k]["timer"])
    launches, windows, ms = notes[2]["timer"]
    assert (launches, windows) == (3, 120) and ms > 0.0, notes[2]
    for pvw, avw in views:
        L.dgrp_model_destroy(pvw)
        L.dgrp_model_destroy(avw)
    plain.close()
    att.close()
