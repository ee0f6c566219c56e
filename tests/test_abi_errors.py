"""Error behaviour of the C ABI (include/deepgrp_hip.h): bad arguments come back as DGRP_EINVAL with a message in
dgrp_last_error(), before any device work -- so this half runs without a GPU.  The reference raises
ValueError/TypeError from its Cython argument checks at the same places (deepgrp/sequence.pyx:25-36,
deepgrp/mss.pyx:24-27); the mirror package turns these codes into exceptions."""
import ctypes as C

import pytest

from deepgrp_amd._lib import lib

EINVAL = -1
P = 0x10000                    # a non-NULL pointer value that is never dereferenced: an earlier check fails
i64x1 = (C.c_int64 * 1)(0)


def info4():
    return (C.c_int64 * 4)()


def plan_out(null=None):
    """The four output pointers of dgrp_model_plan (kernel, lds_bytes, ospan, avg_up), the one at index `null` NULL."""
    out = [C.pointer(C.c_int()), C.pointer(C.c_int64()), C.pointer(C.c_int()), C.pointer(C.c_int())]
    if null is not None:
        out[null] = None
    return out


def train_args(T=50, u=20, C=5, attention=1, params=P, idx=P, truth=P, n=1000, starts=P, B=4, masks=None, loss=P, grads=None, work=P,
               work_bytes=1 << 40, stream=None):
    """The arguments of dgrp_train_step: a call that would be accepted (P is 16-byte aligned), but for the ones given."""
    return (T, u, C, attention, params, idx, truth, n, starts, B, masks, loss, grads, work, work_bytes, stream)


def train_layout(T, u, C, attention, B):
    """(parameter count, workspace bytes) as csrc/train_kernels.hip lays them out: the Keras tensors back to back; the
    workspace's ten float buffers, each rounded up to 256 bytes."""
    Up, F, nt, ntc = (u + 15) // 16 * 16, (2 if attention else 1) * u, (B + 15) // 16, (T + 31) // 32
    total = 15 * u + 3 * u * u + 6 * u + (u if attention else 0) + F * C + C
    nh = total - (15 * u + 3 * u * u + 6 * u)
    floats = [Up * 3 * Up, Up * 3 * Up, 2 * nt * T * 5 * 16 * Up, B * T * u, B * T * u, B * T * C, B * nh, B, 2 * nt * Up * 3 * Up,
              2 * nt * ntc * 7 * 3 * Up]
    return total, sum((4 * f + 255) // 256 * 256 for f in floats)


CASES = [
    ("dgrp_strip_n", lambda: (None, 5, i64x1, i64x1), "dgrp_strip_n"),
    ("dgrp_strip_n", lambda: (P, -1, i64x1, i64x1), "dgrp_strip_n"),
    ("dgrp_encode", lambda: (None, 10, P, None), "dgrp_encode"),
    ("dgrp_encode", lambda: (P, -1, P, None), "dgrp_encode"),
    ("dgrp_onehot", lambda: (P, 3, None, None), "dgrp_onehot"),
    ("dgrp_fasta_encode", lambda: (P, -1, P, info4(), P, 0, None), "dgrp_fasta_encode"),
    ("dgrp_fasta_encode", lambda: (P, 10, P, None, P, 1 << 20, None), "dgrp_fasta_encode"),
    ("dgrp_fasta_encode", lambda: (None, 10, P, info4(), P, 1 << 20, None), "NULL pointer"),
    ("dgrp_fasta_encode_batch", lambda: (P, -1, None, None, P, None, P, 0, None), "dgrp_fasta_encode_batch"),
    ("dgrp_fasta_encode_batch", lambda: (P, 2, None, None, P, None, P, 0, None), "dgrp_fasta_encode_batch"),
    ("dgrp_windows_onehot", lambda: (P, 100, 10, 5, 0, 1, 3, P, None), "elem"),
    ("dgrp_windows_onehot", lambda: (P, 100, 0, 5, 0, 1, 4, P, None), "bad T/s/w0/nw"),
    ("dgrp_windows_onehot", lambda: (P, 100, 10, 0, 0, 1, 4, P, None), "bad T/s/w0/nw"),
    ("dgrp_windows_onehot", lambda: (None, 100, 10, 5, 0, 1, 4, P, None), "NULL pointer"),
    ("dgrp_windows_onehot", lambda: (P, 100, 10, 5, 18, 2, 4, P, None), "runs past"),
    ("dgrp_model_create", lambda: (None, 200, 32, 5, 0, P, P, P, P, P, None), "NULL out"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 0, 32, 5, 0, P, P, P, P, P, None), "window size"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 70000, 32, 5, 0, P, P, P, P, P, None), "window size"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 0, 5, 0, P, P, P, P, P, None), "units"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 2049, 5, 0, P, P, P, P, P, None), "units"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 32, 1, 0, P, P, P, P, P, None), "classes"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 32, 65, 0, P, P, P, P, P, None), "classes"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 32, 5, 0, P, None, P, None, P, P), "NULL tensor"),
    ("dgrp_model_create", lambda: (C.pointer(C.c_void_p()), 200, 32, 5, 1, P, P, P, None, P, P), "NULL tensor"),   # attention without a scale
    ("dgrp_model_create_lstm", lambda: (None, 200, 32, 5, P, P, P, P, P), "NULL out"),
    ("dgrp_model_create_lstm", lambda: (C.pointer(C.c_void_p()), 200, 2049, 5, P, P, P, P, P), "units"),
    ("dgrp_model_create_lstm", lambda: (C.pointer(C.c_void_p()), 200, 32, 5, P, P, None, P, P), "NULL tensor"),
    ("dgrp_model_dims", lambda: (None, None, None, None, None), "NULL model"),
    ("dgrp_model_flags", lambda: (None,), "NULL model"),
    ("dgrp_forward_windows", lambda: (None, P, 1000, 50, 0, 1, P, P, 0, None), "dgrp_forward"),
    ("dgrp_forward_merge", lambda: (None, P, 1000, 50, 256, 0, 1, P, P, 0, None), "dgrp_forward"),
    ("dgrp_forward_windows_reference", lambda: (None, P, 1000, 50, 0, 1, P, P, 1 << 20, None), "bad arguments"),
    ("dgrp_get_max", lambda: (P, 10, P, 0, 5, 5, 1, None), "bad shape"),
    ("dgrp_get_max", lambda: (P, 10, P, 2, 5, 0, 1, None), "bad shape"),
    ("dgrp_get_max", lambda: (None, 10, P, 2, 5, 5, 1, None), "NULL pointer"),
    ("dgrp_scores", lambda: (P, -1, 5, P, P, None), "bad n/C"),
    ("dgrp_scores", lambda: (P, 10, 0, P, P, None), "bad n/C"),
    ("dgrp_scores", lambda: (P, 10, 65, P, P, None), "bad n/C"),
    ("dgrp_scores", lambda: (P, 10, 5, None, P, None), "NULL pointer"),
    ("dgrp_softmax_labels", lambda: (P, 10, 0, P, P, P, 1 << 20, None), "bad n/C"),
    ("dgrp_softmax_labels", lambda: (P, 10, 5, P, P, P, 16, None), "workspace"),
    ("dgrp_mss_labels", lambda: (P, P, -1, 5, 50, 50, P, None, P, 1 << 30, None), "out of range"),
    ("dgrp_mss_labels", lambda: (P, P, 1 << 31, 5, 50, 50, P, None, P, 1 << 30, None), "out of range"),
    ("dgrp_mss_labels", lambda: (P, P, 100, 1, 50, 50, P, None, P, 1 << 30, None), "nof_labels"),
    ("dgrp_mss_labels", lambda: (P, P, 100, 65, 50, 50, P, None, P, 1 << 30, None), "nof_labels"),
    ("dgrp_mss_labels", lambda: (None, P, 100, 5, 50, 50, P, None, P, 1 << 30, None), "NULL pointer"),
    ("dgrp_mss_segments_host", lambda: (None, 0, None, 0, None), "NULL pointer"),
    ("dgrp_mss_labels_batch", lambda: (P, P, -1, 1, i64x1, 5, 50, 50, P, P, 1 << 30, None), "bad arguments"),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, None, 5, 50, 50, P, P, 1 << 30, None), "bad arguments"),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, (C.c_int64 * 3)(0, 64, 128), 1, 50, 50, P, P, 1 << 30, None), "nof_labels"),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, (C.c_int64 * 3)(0, 64, 100), 5, 50, 50, P, P, 1 << 30, None), "from 0 to total_n"),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, (C.c_int64 * 3)(0, 50, 128), 5, 50, 50, P, P, 1 << 30, None), "multiples of 64"),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, (C.c_int64 * 3)(0, 0, 128), 5, 50, 50, P, P, 1 << 30, None), "increasing"),
    ("dgrp_segments", lambda: (P, -1, 0, 0, P, 10, P, P, 1 << 20, None), "bad arguments"),
    ("dgrp_segments", lambda: (P, 10, 0, 0, P, 10, None, P, 1 << 20, None), "bad arguments"),
    ("dgrp_segments", lambda: (None, 10, 0, 0, P, 10, P, P, 1 << 20, None), "NULL pointer"),
    ("dgrp_predict_record", lambda: (None, P, 1000, 50, 256, 50, 50, 1, 0, 0, P, 10, i64x1, P, 1 << 30, None), "bad arguments"),
    ("dgrp_predict_batch", lambda: (None, P, 1, P, P, P, P, 50, 256, 50, 50, P, 10, i64x1, P, 1 << 30, None), "bad arguments"),
    ("dgrp_confusion_matrix", lambda: (P, P, 10, 0, P, P, None), "classes"),
    ("dgrp_confusion_matrix", lambda: (P, P, 10, 65, P, P, None), "classes"),
    ("dgrp_confusion_matrix", lambda: (P, P, -1, 5, P, P, None), "bad arguments"),
    ("dgrp_confusion_matrix", lambda: (P, P, 10, 5, None, P, None), "bad arguments"),
    ("dgrp_filter_segments", lambda: (P, P, -1, 50, None), "negative length"),
    ("dgrp_filter_segments", lambda: (None, P, 10, 50, None), "NULL pointer"),
    ("dgrp_filter_segments", lambda: (P, P, 1 << 39, 50, None), "too long"),
    # (mode 2 on a model without attention needs a model: tests/test_gpu_classes.py)
    ("dgrp_model_plan", lambda: (None, 0, 50, *plan_out()), "NULL model"),
    ("dgrp_model_plan", lambda: (P, 0, 50, *plan_out(0)), "NULL output"),
    ("dgrp_model_plan", lambda: (P, 0, 50, *plan_out(1)), "NULL output"),
    ("dgrp_model_plan", lambda: (P, 0, 50, *plan_out(2)), "NULL output"),
    ("dgrp_model_plan", lambda: (P, 0, 50, *plan_out(3)), "NULL output"),
    ("dgrp_model_plan", lambda: (P, -1, 50, *plan_out()), "mode -1"),
    ("dgrp_model_plan", lambda: (P, 3, 50, *plan_out()), "mode 3"),
    ("dgrp_model_plan", lambda: (P, 1, 0, *plan_out()), "step 0"),
    ("dgrp_model_plan", lambda: (P, 2, -5, *plan_out()), "step -5"),
    # dgrp_train_step(T, u, C, attention, params, idx, truth, n, starts, B, masks, loss, grads, work, work_bytes, stream): masks and grads
    # may be NULL, every other pointer in turn
    ("dgrp_train_step", lambda: train_args(params=None), "NULL parameter, index, truth, start or loss"),
    ("dgrp_train_step", lambda: train_args(idx=None), "NULL parameter, index, truth, start or loss"),
    ("dgrp_train_step", lambda: train_args(truth=None), "NULL parameter, index, truth, start or loss"),
    ("dgrp_train_step", lambda: train_args(starts=None), "NULL parameter, index, truth, start or loss"),
    ("dgrp_train_step", lambda: train_args(loss=None), "NULL parameter, index, truth, start or loss"),
    ("dgrp_train_step", lambda: train_args(work=None), "workspace NULL or not 16-byte aligned"),
    ("dgrp_train_step", lambda: train_args(work=P + 8), "workspace NULL or not 16-byte aligned"),
    ("dgrp_train_step", lambda: train_args(n=49), "record of 49 bases is shorter than the window (50)"),
    ("dgrp_train_step", lambda: train_args(T=0), "vecsize 0 outside 1..4096"),
    ("dgrp_train_step", lambda: train_args(T=4097, n=5000), "vecsize 4097 outside 1..4096"),
    ("dgrp_train_step", lambda: train_args(u=0), "0 units outside 1..256"),
    ("dgrp_train_step", lambda: train_args(u=257), "257 units outside 1..256"),
    ("dgrp_train_step", lambda: train_args(C=1), "1 classes outside 2..16"),
    ("dgrp_train_step", lambda: train_args(C=17), "17 classes outside 2..16"),
    ("dgrp_train_step", lambda: train_args(B=0), "batch size 0 outside 1..2^18"),
    ("dgrp_train_step", lambda: train_args(B=(1 << 18) + 1), "batch size 262145 outside 1..2^18"),
    # dgrp_optimizer_step(kind, params, grads, state1, state2, count, lr, rho, momentum, epsilon, step, stream)
    ("dgrp_optimizer_step", lambda: (2, P, P, P, P, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "optimizer kind 2"),
    ("dgrp_optimizer_step", lambda: (-1, P, P, P, P, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "optimizer kind -1"),
    ("dgrp_optimizer_step", lambda: (0, P, P, P, P, 0, 1e-3, 0.9, 0.9, 1e-7, 1, None), "optimizer: 0 parameters"),
    ("dgrp_optimizer_step", lambda: (1, P, P, P, P, 4, 1e-3, 0.9, 0.9, 1e-7, 0, None), "step 0 (the first step is 1)"),
    ("dgrp_optimizer_step", lambda: (0, None, P, P, P, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "NULL parameter, gradient or state"),
    ("dgrp_optimizer_step", lambda: (0, P, None, P, P, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "NULL parameter, gradient or state"),
    ("dgrp_optimizer_step", lambda: (1, P, P, None, P, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "NULL parameter, gradient or state"),
    ("dgrp_optimizer_step", lambda: (1, P, P, P, None, 4, 1e-3, 0.9, 0.9, 1e-7, 1, None), "NULL parameter, gradient or state"),
]


@pytest.mark.parametrize("name,make,fragment", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_bad_arguments_are_refused_before_any_device_work(name, make, fragment):
    L = lib()
    rc = getattr(L, name)(*make())
    assert rc == EINVAL, (name, rc)
    msg = L.dgrp_last_error().decode()
    assert fragment in msg, msg


ENOMEM = -3
SMALL_WORKSPACE = [
    ("dgrp_fasta_encode", lambda: (P, 1000, P, info4(), P, 8, None)),
    ("dgrp_fasta_encode_batch", lambda: (P, 2, (C.c_int64 * 2)(0, 500), (C.c_int64 * 2)(500, 500), P, (C.c_int64 * 8)(), P, 8, None)),
    ("dgrp_mss_labels", lambda: (P, P, 1000, 5, 50, 50, P, None, P, 8, None)),
    ("dgrp_mss_labels_batch", lambda: (P, P, 128, 2, (C.c_int64 * 3)(0, 64, 128), 5, 50, 50, P, P, 8, None)),
    ("dgrp_segments", lambda: (P, 1000, 0, 0, P, 10, P, P, 8, None)),
    ("dgrp_train_step", lambda: train_args(work_bytes=8)),
    ("dgrp_train_step", lambda: train_args(work_bytes=train_layout(50, 20, 5, 1, 4)[1] - 1)),
]


@pytest.mark.parametrize("name,make", SMALL_WORKSPACE, ids=[f"{c[0]}-{i}" if c[0] == "dgrp_train_step" else c[0] for i, c in enumerate(SMALL_WORKSPACE)])
def test_short_workspace_is_refused_before_any_device_work(name, make):
    """The sizes come from the matching *_workspace_bytes call; a shorter buffer is DGRP_ENOMEM, never a partial run."""
    L = lib()
    assert getattr(L, name)(*make()) == ENOMEM
    assert "workspace" in L.dgrp_last_error().decode()


@pytest.mark.parametrize("shape", [(50, 20, 5, 1, 4), (1, 1, 2, 0, 1), (342, 60, 5, 1, 256), (4096, 256, 16, 1, 17)], ids=str)
def test_train_workspace_one_byte_short_names_both_sizes(shape):
    L = lib()
    need = L.dgrp_train_workspace_bytes(*shape)
    assert need == train_layout(*shape)[1]
    T, u, C, att, B = shape
    assert L.dgrp_train_step(*train_args(T=T, u=u, C=C, attention=att, B=B, n=T, work_bytes=need - 1)) == ENOMEM
    msg = L.dgrp_last_error().decode()
    assert f"workspace of {need - 1} bytes, {need} needed" in msg, msg


def test_train_size_queries_follow_the_layout_and_are_0_outside_the_envelope():
    """Units 1..256, classes 2..16, windows 1..4096, batch 1..2^18: the formula of train_layout inside, 0 one step outside."""
    L = lib()
    for u in (0, 1, 2, 15, 16, 17, 60, 128, 255, 256, 257, -1):
        for C in (1, 2, 3, 5, 16, 17, 0):
            for att in (0, 1):
                inside = 1 <= u <= 256 and 2 <= C <= 16
                assert L.dgrp_train_param_count(u, C, att) == (train_layout(1, u, C, att, 1)[0] if inside else 0), (u, C, att)
    assert L.dgrp_train_param_count(20, 5, 7) == L.dgrp_train_param_count(20, 5, 1)          # attention is a flag: non-zero is yes
    for T in (0, 1, 31, 32, 33, 342, 4096, 4097, -1):
        for u in (0, 1, 16, 17, 256, 257):
            for C in (1, 2, 16, 17):
                for B in (0, 1, 15, 16, 17, 256, 1 << 18, (1 << 18) + 1, -1):
                    inside = 1 <= T <= 4096 and 1 <= u <= 256 and 2 <= C <= 16 and 1 <= B <= 1 << 18
                    for att in (0, 1):
                        want = train_layout(T, u, C, att, B)[1] if inside else 0
                        assert L.dgrp_train_workspace_bytes(T, u, C, att, B) == want, (T, u, C, att, B)


def test_size_queries_are_total_functions():
    """The *_bytes / count helpers take any int64 without failing; non-positive sizes give a small non-negative answer."""
    L = lib()
    for n in (0, 1, 199, 200, 201, 249, 250, 251, 1000, 10 ** 6 + 7):      # deepgrp/prediction.py:31: range(0, n - T, s)
        assert L.dgrp_window_count(n, 200, 50) == len(range(0, n - 200, 50)), n
    assert L.dgrp_window_count(1000, 0, 50) == 0 and L.dgrp_window_count(1000, 200, 0) == 0
    for f, args in (("dgrp_fasta_workspace_bytes", (0,)), ("dgrp_fasta_batch_workspace_bytes", (0, 0)),
                    ("dgrp_mss_workspace_bytes", (0,)), ("dgrp_mss_batch_workspace_bytes", (0, 0)),
                    ("dgrp_segments_workspace_bytes", (0,))):
        assert getattr(L, f)(*args) >= 0, f
    for f, args in (("dgrp_train_param_count", (0, 0, 0)), ("dgrp_train_workspace_bytes", (0, 0, 0, 0, 0)),
                    ("dgrp_train_workspace_bytes", (50, 20, 5, 1, 2 ** 62)), ("dgrp_train_workspace_bytes", (50, 20, 5, 1, -2 ** 62)),
                    ("dgrp_train_workspace_bytes", (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 1, 4))):
        assert getattr(L, f)(*args) == 0, (f, args)                         # "0 on sizes the step refuses"
    sizes = [L.dgrp_train_workspace_bytes(342, 60, 5, 1, b) for b in (1, 16, 17, 256, 1 << 18)]
    assert sizes == sorted(sizes) and sizes[0] > 0, sizes
    # monotone in n: a caller may size for the largest record once
    for f in ("dgrp_fasta_workspace_bytes", "dgrp_mss_workspace_bytes", "dgrp_segments_workspace_bytes"):
        sizes = [getattr(L, f)(n) for n in (1, 1000, 10 ** 6, 10 ** 8, 2 ** 31 - 1)]
        assert sizes == sorted(sizes) and sizes[0] > 0, (f, sizes)


# dgrp_mss_workspace_bytes / dgrp_mss_batch_workspace_bytes as commit 6461cd0 (the parent of the labels driver's split into rungs)
# answered: dgrp_mss_segments_host recovers n from the byte count by bisection over the carve, so the carve is part of the ABI.
MSS_WORKSPACE_BYTES = {0: 27136, 1: 29952, 63: 31488, 64: 31488, 65: 31488, 4095: 151040, 4096: 151040, 4097: 153088,
                       16384 * 3 + 1: 1539840, 1 << 20: 32243456, (1 << 31) - 1: 65979181568}
MSS_BATCH_WORKSPACE_BYTES = {(0, 0): 31488, (128, 2): 35328, (1 << 20, 400): 32291840}


def test_mss_workspace_carve_is_pinned():
    L = lib()
    assert {n: L.dgrp_mss_workspace_bytes(n) for n in MSS_WORKSPACE_BYTES} == MSS_WORKSPACE_BYTES
    assert {a: L.dgrp_mss_batch_workspace_bytes(*a) for a in MSS_BATCH_WORKSPACE_BYTES} == MSS_BATCH_WORKSPACE_BYTES
