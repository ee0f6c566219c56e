"""The training kernels against the float64 checker (tests/train_oracle.py).  Bounds: per tensor e = max |g - g64| / max |g64|; the
HIP figure may be at most 4 x the figure of the checker run in float32 on the CPU on the same inputs (floor 1e-6)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import train_oracle as tro

pytestmark = pytest.mark.gpu

CASES = [  # units, T, batch, classes, attention
    (5, 7, 1, 2, True), (20, 50, 5, 5, True), (36, 50, 33, 5, False), (60, 7, 33, 2, True),
    (128, 50, 5, 5, False), (128, 7, 33, 5, True), (60, 50, 1, 5, False), (20, 7, 33, 2, False),
]


def _trainer(case):
    from deepgrp_amd import training
    tr = training.DeviceTrainer(case["weights"], case["T"], len(case["starts"]))
    return tr, training.DeviceRecord(case["idx"], case["truth"])


def _hip(case, masks="case"):
    from deepgrp_amd import training
    tr, rec = _trainer(case)
    m = case["masks"] if masks == "case" else masks
    loss = float(tr.run(rec, case["starts"], m).cpu()[0])
    u, C = tr.units, tr.classes
    return loss, training.unflatten_weights(tr.grads.cpu().numpy(), u, C, tr.attention), tr, rec


@pytest.mark.parametrize("units,T,batch,classes,attention", CASES)
def test_loss_and_gradients_against_float64(units, T, batch, classes, attention):
    case = tro.make_case(units, T, batch, classes, attention, seed=units + T + batch)
    assert (case["masks"] == 0).any() and (case["idx"] == 4).any() and (case["truth"].sum(0) > 1).any()
    assert batch == 1 or len(set(case["starts"].tolist())) < batch
    args = (case["weights"], case["idx"], case["truth"], case["starts"], T, case["masks"])
    l64, g64, p64 = tro.loss_and_grads(*args, torch.float64)
    l32, g32, _ = tro.loss_and_grads(*args, torch.float32)
    assert p64.min() > 1e-5 and p64.max() < 1 - 1e-5                     # nowhere near the 1e-7 clip
    loss, grads, _tr, _rec = _hip(case)
    problems = []
    e32, e = abs(l32 - l64) / abs(l64), abs(loss - l64) / abs(l64)
    print(f"loss: hip {e:.3e} float32 {e32:.3e}")
    if e > tro.bound(e32):
        problems.append(f"loss: {e:.3e} > {tro.bound(e32):.3e}")
    for name, want in g64.items():
        e32, e = tro.rel_err(g32[name], want), tro.rel_err(grads[name], want)
        print(f"{name}: hip {e:.3e} float32 {e32:.3e}")
        if not e <= tro.bound(e32):
            problems.append(f"{name}: {e:.3e} > {tro.bound(e32):.3e}")
    assert not problems, "; ".join(problems)


@pytest.mark.parametrize("attention", [False, True])
def test_loss_only_mode(attention):
    from deepgrp_amd.pipeline import DeviceModel
    units, T, batch, classes = 36, 20, 3, 5
    case = tro.make_case(units, T, batch, classes, attention, seed=11)
    tr, rec = _trainer(case)
    with_grads = tr.run(rec, case["starts"], case["masks"]).cpu().numpy()
    alone = tr.run(rec, case["starts"], case["masks"], with_grads=False).cpu().numpy()
    assert with_grads.tobytes() == alone.tobytes()
    # the probability the loss implies: a truth with a single one at (window i, step t, class c) makes loss * B * T = -log p[i, t, c]
    w = case["weights"]
    model = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], w["scale"], vecsize=T)
    starts = np.array([0, T, 2 * T], np.int64)                          # windows 0, 1, 2 at stride T
    probs = model.forward_windows(torch.from_numpy(case["idx"]).cuda(), T, 0, batch).cpu().numpy()
    from deepgrp_amd import training
    worst = 0.0
    for i, t, c in [(0, 0, 0), (1, T - 1, classes - 1), (2, T // 2, 2), (0, 3, 1), (2, T - 1, 0), (1, 1, 3)]:
        truth = np.zeros_like(case["truth"])
        truth[c, starts[i] + t] = 1
        loss = float(tr.run(training.DeviceRecord(case["idx"], truth), starts, np.ones((batch, 2, 5), np.float32), with_grads=False).cpu()[0])
        worst = max(worst, abs(np.exp(-loss * batch * T) - probs[i, t, c]))
    print(f"loss-implied probabilities vs dgrp_forward_windows: {worst:.3e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("kind,momentum", [("RMSprop", 0.0), ("RMSprop", 0.9), ("Adam", 0.0), ("Adam", 0.9)])
@pytest.mark.parametrize("count", [1, 63, 10007])
def test_optimizer_steps(kind, momentum, count):
    from deepgrp_amd import _lib
    from deepgrp_amd.training import OPTIMIZERS
    rng = np.random.default_rng(count)
    lr, rho, eps = 1e-3, 0.9, 1e-10
    w0 = rng.normal(size=count).astype(np.float32)
    gs = [rng.normal(scale=0.1, size=count).astype(np.float32) for _ in range(3)]
    ref = {}
    for f in (np.float64, np.float32):
        w, s1, s2 = w0.astype(f), np.zeros(count, f), np.zeros(count, f)
        for step, g in enumerate(gs, 1):
            if kind == "RMSprop":
                w, s1, s2 = tro.rmsprop_step(w, g, s1, s2, lr, rho, momentum, eps, f)
            else:
                w, s1, s2 = tro.adam_step(w, g, s1, s2, lr, momentum, rho, eps, step, f)
        ref[f] = (w, s1, s2)
    d = [torch.from_numpy(a).cuda() for a in (w0, np.zeros(count, np.float32), np.zeros(count, np.float32))]
    for step, g in enumerate(gs, 1):
        dg = torch.from_numpy(g).cuda()
        _lib.check(_lib.lib().dgrp_optimizer_step(OPTIMIZERS[kind.lower()], d[0].data_ptr(), dg.data_ptr(), d[1].data_ptr(),
                                                  d[2].data_ptr(), count, lr, rho, momentum, eps, step,
                                                  torch.cuda.current_stream().cuda_stream), "dgrp_optimizer_step")
    for name, got, want, f32 in zip(("w", "state1", "state2"), d, ref[np.float64], ref[np.float32]):
        e, e32 = tro.rel_err(got.cpu().numpy(), want), tro.rel_err(f32, want)
        print(f"{kind} {name}: hip {e:.3e} float32 {e32:.3e}")
        assert e <= tro.bound(e32), f"{name}: {e:.3e} > {tro.bound(e32):.3e}"


def test_five_training_steps_follow_the_float64_trajectory():
    units, T, batch, classes = 20, 30, 16, 5
    hp = dict(lr=1e-3, rho=0.9, momentum=0.9, epsilon=1e-10)             # defaults.toml of the reference (RMSprop)
    case = tro.make_case(units, T, batch, classes, True, seed=5)
    rng = np.random.default_rng(9)
    n = case["idx"].size
    batches = [rng.integers(0, n - T, batch).astype(np.int64) for _ in range(5)]
    masks = [((rng.random((batch, 2, 5)) >= 0.25) / 0.75).astype(np.float32) for _ in range(5)]

    def helper(dtype, f):
        w = {k: (None if v is None else v.astype(f)) for k, v in case["weights"].items()}
        flat = tro.flat(w).astype(f)
        ms, mom, losses = np.zeros_like(flat), np.zeros_like(flat), []
        from deepgrp_amd.training import unflatten_weights
        for st, m in zip(batches, masks):
            cur = {k: v for k, v in unflatten_weights(flat.astype(np.float32), units, classes, True).items()} if f is np.float32 else None
            if cur is None:                                               # float64: unflatten without rounding
                cur, pos = {}, 0
                for k in tro.NAMES:
                    size = case["weights"][k].size
                    cur[k] = flat[pos:pos + size].reshape(case["weights"][k].shape)
                    pos += size
            loss, g, _ = tro.loss_and_grads(cur, case["idx"], case["truth"], st, T, m, dtype)
            losses.append(loss)
            flat, ms, mom = tro.rmsprop_step(flat, tro.flat(g), ms, mom, hp["lr"], hp["rho"], hp["momentum"], hp["epsilon"], f)
        return np.array(losses), flat

    l64, w64 = helper(torch.float64, np.float64)
    l32, w32 = helper(torch.float32, np.float32)
    tr, rec = _trainer(case)
    got = []
    for st, m in zip(batches, masks):
        got.append(float(tr.run(rec, st, m).cpu()[0]))
        tr.apply("RMSprop", hp["lr"], hp["rho"], hp["momentum"], hp["epsilon"])
    e_l, e32_l = tro.rel_err(got, l64), tro.rel_err(l32, l64)
    e_w, e32_w = tro.rel_err(tr.params.cpu().numpy(), w64), tro.rel_err(w32, w64)
    print(f"losses: hip {e_l:.3e} float32 {e32_l:.3e}; weights: hip {e_w:.3e} float32 {e32_w:.3e}")
    assert e_l <= tro.bound(e32_l) and e_w <= tro.bound(e32_w)


def test_the_same_call_gives_the_same_bytes():
    case = tro.make_case(60, 50, 33, 5, True, seed=2)
    tr, rec = _trainer(case)
    first = (tr.run(rec, case["starts"], case["masks"]).cpu().numpy().tobytes(), tr.grads.cpu().numpy().tobytes())
    tr.grads.zero_()
    second = (tr.run(rec, case["starts"], case["masks"]).cpu().numpy().tobytes(), tr.grads.cpu().numpy().tobytes())
    assert first == second


def test_bad_arguments_are_refused_before_device_work():
    from deepgrp_amd import _lib
    L = _lib.lib()
    assert L.dgrp_train_workspace_bytes(50, 257, 5, 0, 4) == 0 and L.dgrp_train_workspace_bytes(50, 20, 17, 0, 4) == 0
    assert L.dgrp_train_param_count(20, 5, 1) == 15 * 20 + 3 * 400 + 6 * 20 + 20 + 40 * 5 + 5
    assert L.dgrp_train_step(50, 20, 5, 0, None, None, None, 100, None, 4, None, None, None, None, 0, None) == -1
    assert b"NULL" in L.dgrp_last_error()
    assert L.dgrp_optimizer_step(2, None, None, None, None, 4, 1e-3, 0.9, 0.9, 1e-10, 1, None) == -1
    assert b"kind" in L.dgrp_last_error()


def _inputs(tmp, n_train=60_000, n_valid=30_000):
    from deepgrp_amd import synthetic
    paths = {}
    lines = []
    for role, n, contig in (("train", n_train, 1), ("valid", n_valid, 2)):
        idx, _lab = synthetic.synthetic_truth(n, contig=contig, flank=500)
        fwd = np.zeros((5, n), np.int8)
        fwd[idx, np.arange(n)] = 1
        paths[role] = os.path.join(tmp, f"chr{role}.fa.gz.npz")
        np.savez(paths[role], fwd=fwd)
        lines += synthetic.synthetic_annotation(n, contig=contig, name=f"chr{role}", flank=500)
        if role == "valid":
            paths["fasta"] = os.path.join(tmp, "valid.fa")
            with open(paths["fasta"], "w") as fh:
                fh.write(">chrvalid\n" + synthetic.synthetic_chromosome(n, contig=contig, flank=500).decode() + "\n")
    paths["bed"] = os.path.join(tmp, "rm.bed")
    with open(paths["bed"], "w") as fh:
        fh.writelines(lines)
    return paths


def _toml(tmp, n_batches, n_epochs):
    path = os.path.join(tmp, "p.toml")
    with open(path, "w") as fh:
        fh.write(f"units = 16\nvecsize = 50\nbatch_size = 32\nn_batches = {n_batches}\nn_epochs = {n_epochs}\nattention = true\n"
                 "dropout = 0.25\nlearning_rate = 0.005\n")
    return path


def test_host_starts_outside_the_record_are_an_error():
    case = tro.make_case(20, 7, 5, 2, False, seed=1)
    tr, rec = _trainer(case)
    for bad in (-1, rec.n - 7 + 1):
        starts = case["starts"].copy()
        starts[2] = bad
        with pytest.raises(ValueError, match="start positions"):
            tr.run(rec, starts, None)
    tr.run(rec, np.array([0, rec.n - 7], np.int64), None)                # both ends are windows


def test_train_with_a_contig_absent_from_the_bed_trains_on_background(tmp_path):
    """The command's own path: contig names from the file names, a BED table that names other contigs.  The truth is then all
    background, as with an empty table: with one seed the two runs write the same history and the same model, byte for byte, and
    a table that does name the contigs gives another one."""
    from deepgrp_amd.__main__ import main
    tmp = str(tmp_path)
    paths, toml = _inputs(tmp, 20_000, 10_000), _toml(tmp, 3, 2)
    empty = os.path.join(tmp, "empty.bed")
    open(empty, "w").close()
    other = {role: os.path.join(tmp, f"other{role}.fa.gz.npz") for role in ("train", "valid")}
    for role in other:                                                    # the same arrays under names the table does not hold
        with open(paths[role], "rb") as src, open(other[role], "wb") as dst:
            dst.write(src.read())
    out = {}
    for run, files, bed in (("absent", other, paths["bed"]), ("empty", other, empty), ("named", paths, paths["bed"])):
        model, logdir = os.path.join(tmp, f"{run}.hdf5"), os.path.join(tmp, run)
        main(["train", toml, files["train"], files["valid"], bed, "--logdir", logdir, "--modelfile", model, "--seed", "2"])
        out[run] = (open(os.path.join(logdir, "history.tsv")).read(), open(model, "rb").read())
    assert len(out["absent"][0].splitlines()) == 3
    assert out["absent"] == out["empty"]
    assert out["absent"][0] != out["named"][0]


def test_train_twice_with_one_seed_writes_identical_files(tmp_path):
    from deepgrp_amd.__main__ import main
    tmp = str(tmp_path)
    paths, toml = _inputs(tmp, 20_000, 10_000), _toml(tmp, 3, 2)
    out = []
    for run in ("a", "b"):
        model = os.path.join(tmp, f"{run}.hdf5")
        main(["train", toml, paths["train"], paths["valid"], paths["bed"], "--logdir", os.path.join(tmp, run), "--modelfile", model,
              "--seed", "4"])
        out.append(open(model, "rb").read())
    assert out[0] == out[1]


def test_train_end_to_end_in_a_child_process(tmp_path):
    from deepgrp_amd.model import Options, keras_config, read_keras_hdf5
    from deepgrp_amd.prediction import setup_prediction_from_options_checkpoint
    tmp = str(tmp_path)
    paths, toml = _inputs(tmp), _toml(tmp, 20, 3)
    logdir, model = os.path.join(tmp, "log"), os.path.join(tmp, "model.hdf5")
    res = subprocess.run([sys.executable, "-m", "deepgrp_amd", "train", toml, paths["train"], paths["valid"], paths["bed"],
                          "--logdir", logdir, "--modelfile", model, "--seed", "1"], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rows = [l.split("\t") for l in open(os.path.join(logdir, "history.tsv")).read().splitlines()]
    assert rows[0] == ["epoch", "loss", "val_loss"] and [r[0] for r in rows[1:]] == ["1", "2", "3"]
    print("history:", rows[1:])
    assert float(rows[-1][1]) < float(rows[1][1])
    assert any(f.endswith(".hdf5") for f in os.listdir(logdir))
    options = Options.from_toml(toml)
    loaded = setup_prediction_from_options_checkpoint(options, logdir)
    assert loaded.units == 16 and loaded.vecsize == 50
    assert read_keras_hdf5(model)["config"] == keras_config(50, 16, 5, True, 0.25)
    res = subprocess.run([sys.executable, "-m", "deepgrp_amd", "predict", model, paths["fasta"]], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
