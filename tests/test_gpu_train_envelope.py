"""The training kernels over their stated envelope (units 1..256, windows 1..4096, classes 2..16), at the sizes where
csrc/train_kernels.hip changes path, against the float64 checker (tests/train_oracle.py).  The rule of every comparison is the one
of tests/test_gpu_train.py: per tensor e = max |g - g64| / max |g64|, at most tro.bound(e32) = 4 x the figure of the checker run in
float32 on the CPU on the same inputs, floor 1e-6.  Every pair is printed (`pytest -s`).

T = 4096 is not run: the checker alone needs some 10 s for it at 4 units."""
import numpy as np
import pytest
import torch

import train_oracle as tro

pytestmark = pytest.mark.gpu

SWEEP = [  # units, T, batch, classes, attention                      what it reaches
    (1, 1, 1, 2, True),          # smallest of everything: empty wgrad loop, no backward product, softmax over one step
    (1, 2, 16, 2, False),        # G = 256; one exactly full tile
    (16, 33, 17, 3, True),       # Up = u; a one-step tail chunk; a second tile holding one window
    (17, 32, 15, 16, False),     # 15 padded units; T of exactly one chunk; C = 16; a tile one row short
    (64, 64, 32, 5, True),       # last 256-thread launch; two exact chunks; two full tiles
    (65, 65, 5, 5, False),       # first 512-thread launch, Up = 80; ntc = 3
    (85, 7, 33, 5, True),        # G = 3: 255 of 256 head threads work
    (86, 7, 33, 5, True),        # G = 2
    (129, 2, 32, 5, True),       # first G = 1; Up = 144
    (200, 50, 5, 16, True),      # middle of the upper half
    (256, 50, 5, 16, True),      # largest units: forward and backward LDS above 64 KB
    (60, 342, 17, 5, True),      # the defaults.toml window: strided head loops; ntc = 11
    (16, 600, 3, 5, False),      # strided loops without attention
    (4, 1024, 2, 2, True),       # long backward chain
    (256, 1300, 1, 16, True),    # head LDS of 65 888 B, just above 64 KB
]


def _run(case, tr=None, starts=None, masks="case", with_grads=True):
    """(loss bytes, gradient bytes, loss, gradients by name, trainer) of one dgrp_train_step on `case`."""
    from deepgrp_amd import training
    if tr is None:
        tr = training.DeviceTrainer(case["weights"], case["T"], len(case["starts"]))
    rec = training.DeviceRecord(case["idx"], case["truth"])
    loss = tr.run(rec, case["starts"] if starts is None else starts, case["masks"] if isinstance(masks, str) else masks,
                  with_grads=with_grads).cpu().numpy()
    flat = tr.grads.cpu().numpy()
    return loss.tobytes(), flat.tobytes(), float(loss[0]), training.unflatten_weights(flat, tr.units, tr.classes, tr.attention), tr


def _reference(case, masks="case"):
    """(float64 loss, gradients, probabilities; float32 loss, gradients) of the checker on `case`."""
    m = case["masks"] if isinstance(masks, str) else masks
    args = (case["weights"], case["idx"], case["truth"], case["starts"], case["T"], m)
    l64, g64, p64 = tro.loss_and_grads(*args, torch.float64)
    l32, g32, _ = tro.loss_and_grads(*args, torch.float32)
    return l64, g64, p64, l32, g32


def _compare(what, loss, grads, ref):
    l64, g64, _p64, l32, g32 = ref
    problems = []
    e32, e = abs(l32 - l64) / abs(l64), abs(loss - l64) / abs(l64)
    print(f"{what} loss: hip {e:.3e} float32 {e32:.3e}")
    if not e <= tro.bound(e32):
        problems.append(f"loss: {e:.3e} > {tro.bound(e32):.3e}")
    for name, want in g64.items():
        e32, e = tro.rel_err(g32[name], want), tro.rel_err(grads[name], want)
        print(f"{what} {name}: hip {e:.3e} float32 {e32:.3e}")
        if not e <= tro.bound(e32):
            problems.append(f"{name}: {e:.3e} > {tro.bound(e32):.3e}")
    assert not problems, f"{what}: " + "; ".join(problems)


def _away_from_the_clip(p64):
    assert p64.min() > 1e-5 and p64.max() < 1 - 1e-5


# ------------------------------------------------------------------------------------------------------------ a. shapes
@pytest.mark.parametrize("units,T,batch,classes,attention", SWEEP)
def test_shape_sweep(units, T, batch, classes, attention):
    case = tro.make_case(units, T, batch, classes, attention, seed=units + T + batch)
    assert (case["masks"] == 0).any() and (case["idx"] == 4).any() and (case["truth"].sum(0) > 1).any()
    assert batch == 1 or len(set(case["starts"].tolist())) < batch
    ref = _reference(case)
    _away_from_the_clip(ref[2])
    _lb, _gb, loss, grads, _tr = _run(case)
    _compare(f"{units}/{T}/{batch}/{classes}/{int(attention)}", loss, grads, ref)
    if T == 1:
        # no step has a predecessor: d recurrent_kernel is a sum over nothing; the softmax over one step is constant: d scale = 0
        for name in ("recurrent_kernel", "scale"):
            assert not ref[1][name].any() and not ref[4][name].any(), name
            assert not grads[name].view(np.uint8).any(), f"d {name} at T = 1 is not all-zero bytes"


# ---------------------------------------------------------------------------------------- b. inputs the sweep does not vary
SHAPE = (36, 20, 17, 5)
both = pytest.mark.parametrize("attention", [False, True], ids=["plain", "attention"])


def _case(attention):
    return tro.make_case(*SHAPE, attention, seed=sum(SHAPE[:3]))


def _window_positions(case):
    """Positions of the record that lie inside some window of the batch (sorted, unique)."""
    return np.unique(case["starts"][:, None] + np.arange(case["T"])[None, :])


@both
def test_without_masks(attention):
    """masks = NULL: the validation path and dropout = 0."""
    case = _case(attention)
    ref = _reference(case, masks=None)
    _away_from_the_clip(ref[2])
    _lb, _gb, loss, grads, _tr = _run(case, masks=None)
    _compare("masks=None", loss, grads, ref)
    ones = _run(case, masks=np.ones_like(case["masks"]))
    assert (_lb, _gb) == ones[:2], "no masks and masks of 1 differ"


@both
def test_class_indices_above_4_are_read_as_n(attention):
    case = _case(attention)
    inside = _window_positions(case)
    idx = case["idx"].copy()
    idx[inside[[1, len(inside) // 2, -2]]] = (5, 200, 255)
    assert idx[inside].max() == 255 and (idx[inside] == 5).any() and (idx[inside] == 200).any()
    high, clamped = dict(case, idx=idx), dict(case, idx=np.minimum(idx, 4))
    ref = _reference(high)
    _away_from_the_clip(ref[2])
    lb, gb, loss, grads, _tr = _run(high)
    _compare("idx > 4", loss, grads, ref)
    assert (lb, gb) == _run(clamped)[:2], "indices above 4 and the same record after np.minimum(idx, 4) differ"


@both
def test_bases_without_a_class_contribute_nothing(attention):
    """Window bases whose truth column is all zero: no loss term and no gradient, for the checker and the kernel alike."""
    case = _case(attention)
    inside = _window_positions(case)
    truth = case["truth"].copy()
    truth[:, inside[[0, 3, len(inside) // 2, -1]]] = 0
    first = int(case["starts"][0])
    truth[:, first + 2] = 0                                               # one of them in the repeated window
    assert (truth[:, inside].sum(0) == 0).sum() >= 4 and (truth[:, inside].sum(0) > 1).any()
    case = dict(case, truth=truth)
    ref = _reference(case)
    _away_from_the_clip(ref[2])
    _lb, _gb, loss, grads, _tr = _run(case)
    _compare("empty truth columns", loss, grads, ref)


@both
def test_both_ends_of_the_record_in_one_tile(attention):
    case = _case(attention)
    n, T = case["idx"].size, case["T"]
    starts = case["starts"].copy()
    starts[2], starts[3] = 0, n - T
    assert starts.min() == 0 and starts.max() == n - T and len(starts) > 16      # both in the first tile of two
    case = dict(case, starts=starts)
    ref = _reference(case)
    _away_from_the_clip(ref[2])
    _lb, _gb, loss, grads, _tr = _run(case)
    _compare("offsets 0 and n - T", loss, grads, ref)


@both
def test_device_starts_outside_the_record_are_clamped(attention):
    """include/deepgrp_hip.h: "a start outside [0, n - T] is clamped into it (no access leaves the arrays)".  Every read of the
    record and of the truth goes through tr_start's clamped value, so the run below reads inside both arrays."""
    case = _case(attention)
    n, T = case["idx"].size, case["T"]
    starts = case["starts"].copy()
    starts[4], starts[9], starts[16] = -5, n - T + 3, n                     # the last one alone in the second tile
    clamped = np.minimum(np.maximum(starts, 0), n - T)
    assert (clamped != starts).sum() == 3
    ref = _reference(dict(case, starts=clamped))
    _away_from_the_clip(ref[2])
    lb, gb, loss, grads, _tr = _run(case, starts=torch.from_numpy(starts).cuda())
    _compare("clamped starts", loss, grads, ref)
    assert (lb, gb) == _run(case, starts=clamped)[:2], "starts outside the record and their clamped values differ"
    assert (lb, gb) == _run(case, starts=torch.from_numpy(clamped).cuda())[:2]


# ------------------------------------------------------------------------------------------------------------ c. the clip
def _clip_case(classes, cls, shift):
    case = tro.make_case(20, 20, 5, classes, True, seed=7)
    w = dict(case["weights"])
    w["ff_bias"] = w["ff_bias"].copy()
    w["ff_bias"][cls] += shift
    return dict(case, weights=w)


def test_clip_low_side():
    """Every probability of the last class is far below 1e-7 and the truth names that class: Keras clips those terms, so they
    enter the loss as -log 1e-7 and have no gradient.  A kernel that let them through would be off by order 1."""
    case = _clip_case(5, -1, -40.0)
    ref = _reference(case)
    p64 = ref[2]
    y = case["truth"][:, case["starts"][:, None] + np.arange(case["T"])[None, :]]            # [C, B, T]
    assert p64[..., -1].max() < 1e-9 and p64[..., :-1].min() > 1e-5 and p64[..., :-1].max() < 1 - 1e-5
    assert y[-1].sum() >= 1
    print(f"clip, low side: last class <= {p64[..., -1].max():.3e}, others {p64[..., :-1].min():.3f} .. {p64[..., :-1].max():.3f}, "
          f"{int(y[-1].sum())} clipped terms, loss {ref[0]:.4f}")
    _lb, _gb, loss, grads, _tr = _run(case)
    _compare("clip low", loss, grads, ref)


def test_clip_high_side():
    """Two classes, class 0 at 1 - 1e-12 or closer: both probabilities of every step are clipped, every gradient is exactly 0."""
    case = _clip_case(2, 0, 40.0)
    ref = _reference(case)
    l64, g64, p64, _l32, g32 = ref
    assert p64[..., 0].min() > 1 - 1e-9 and p64[..., 1].max() < 1e-9
    for name in g64:
        assert not g64[name].any() and not g32[name].any(), name
    print(f"clip, high side: class 1 <= {p64[..., 1].max():.3e}, loss {l64:.4f}")
    _lb, gb, loss, grads, _tr = _run(case)
    _compare("clip high", loss, grads, ref)
    assert not np.frombuffer(gb, np.uint8).any(), "gradients of an all-clipped batch are not all-zero bytes"


# ------------------------------------------------------------------------------------------------- d. state between calls
def test_a_smaller_batch_in_a_larger_workspace():
    """DeviceTrainer keeps the workspace of the larger batch: every buffer of the second run is carved at another offset of bytes
    the first run wrote."""
    big = tro.make_case(36, 20, 33, 5, True, seed=3)
    small = dict(big, starts=big["starts"][:5].copy(), masks=big["masks"][:5].copy())
    *_, tr = _run(big)
    work = tr._work
    lb, gb, loss, grads, _ = _run(small, tr=tr)
    assert tr._work is work, "the workspace was not reused"
    fresh = _run(small)
    assert fresh[4]._work.numel() < work.numel()
    assert (lb, gb) == fresh[:2], "batch 5 after batch 33 differs from batch 5 alone"
    _compare("batch 5 after 33", loss, grads, _reference(small))


def test_loss_only_mode_leaves_the_gradients_alone():
    from deepgrp_amd import training
    case = tro.make_case(36, 20, 17, 5, True, seed=4)
    tr = training.DeviceTrainer(case["weights"], case["T"], 17)
    sentinel = np.random.default_rng(0).integers(0, 256, tr.grads.numel() * 4, dtype=np.uint8)
    tr.grads.copy_(torch.from_numpy(sentinel.view(np.float32)))
    lb, gb, *_ = _run(case, tr=tr, with_grads=False)
    assert gb == sentinel.tobytes()
    assert lb == _run(case)[0]


def test_the_same_call_gives_the_same_bytes_at_200_units():
    """512 threads per recurrent workgroup, G = 1 in the head, C = 16."""
    case = tro.make_case(200, 50, 17, 16, True, seed=2)
    lb, gb, _loss, _grads, tr = _run(case)
    tr.grads.zero_()
    assert (lb, gb) == _run(case, tr=tr)[:2]


# ------------------------------------------------------------------------------------------------------------ e. optimizer
OPT = [  # kind, rho, momentum, epsilon, first step (Adam: rho = beta_2, momentum = beta_1)
    pytest.param("RMSprop", 0.9, 0.0, 1e-7, 1, id="RMSprop-keras-defaults"),
    pytest.param("RMSprop", 0.9, 0.9, 1e-10, 1, id="RMSprop-momentum"),
    pytest.param("Adam", 0.999, 0.9, 1e-7, 1, id="Adam-keras-defaults"),
    pytest.param("Adam", 0.999, 0.9, 1e-7, 1000, id="Adam-steps-1000-1002"),
]


@pytest.mark.parametrize("kind,rho,momentum,eps,first", OPT)
@pytest.mark.parametrize("count", [255, 256, 257])
def test_optimizer_steps(kind, rho, momentum, eps, first, count):
    """Three steps as in tests/test_gpu_train.py, at the counts around one workgroup, with a tenth of the gradient exactly 0 (at
    the same places in every step, so that zero state meets a zero gradient), and from non-zero state at a late step."""
    from deepgrp_amd import _lib
    from deepgrp_amd.training import OPTIMIZERS
    rng = np.random.default_rng(count + first)
    lr = 1e-3
    w0 = rng.normal(size=count).astype(np.float32)
    zero = rng.permutation(count)[:count // 10]
    gs = [rng.normal(scale=0.1, size=count).astype(np.float32) for _ in range(3)]
    for g in gs:
        g[zero] = 0.0
    if first > 1:                                                         # a first and a second moment as a long run leaves them
        s10 = rng.normal(scale=0.03, size=count).astype(np.float32)
        s20 = (0.01 * rng.random(count) + 1e-4).astype(np.float32)
    else:
        s10, s20 = np.zeros(count, np.float32), np.zeros(count, np.float32)
    ref = {}
    for f in (np.float64, np.float32):
        w, s1, s2 = w0.astype(f), s10.astype(f), s20.astype(f)
        for step, g in enumerate(gs, first):
            if kind == "RMSprop":
                w, s1, s2 = tro.rmsprop_step(w, g, s1, s2, lr, rho, momentum, eps, f)
            else:
                w, s1, s2 = tro.adam_step(w, g, s1, s2, lr, momentum, rho, eps, step, f)
        ref[f] = (w, s1, s2)
    d = [torch.from_numpy(a.copy()).cuda() for a in (w0, s10, s20)]
    for step, g in enumerate(gs, first):
        dg = torch.from_numpy(g).cuda()
        _lib.check(_lib.lib().dgrp_optimizer_step(OPTIMIZERS[kind.lower()], d[0].data_ptr(), dg.data_ptr(), d[1].data_ptr(),
                                                  d[2].data_ptr(), count, lr, rho, momentum, eps, step,
                                                  torch.cuda.current_stream().cuda_stream), "dgrp_optimizer_step")
    for name, got, want, f32 in zip(("w", "state1", "state2"), d, ref[np.float64], ref[np.float32]):
        e, e32 = tro.rel_err(got.cpu().numpy(), want), tro.rel_err(f32, want)
        print(f"{kind} {name}: hip {e:.3e} float32 {e32:.3e}")
        assert e <= tro.bound(e32), f"{name}: {e:.3e} > {tro.bound(e32):.3e}"
    if first == 1:                                                        # zero state and zero gradients: nothing moves there
        assert np.array_equal(d[0].cpu().numpy()[zero], w0[zero])
        assert not d[1].cpu().numpy()[zero].any() and not d[2].cpu().numpy()[zero].any()
