"""dgrp_train_step_multi, training_multi and the search on the device.  A job of a multi call must receive the BYTES that
dgrp_train_step gives for the same arguments, whatever else is in the call; the float64 comparison uses the rule of
tests/test_gpu_train.py (at most 4 x the float32 figure of the checker, floor 1e-6)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import train_oracle as tro

pytestmark = pytest.mark.gpu

SHAPES = [  # units, T, batch, attention, classes: block widths 256 / 512, 1..3 tiles of 16 windows, 1 and 2 step chunks, 2..16 classes
    (20, 7, 33, True, 5), (70, 12, 5, False, 3), (4, 1, 1, False, 2), (36, 40, 17, True, 5), (130, 5, 2, True, 16),
]
NAN = float("nan")
LEARNING_RATE_OF_THE_THIRD = 0.3     # with it the third model runs all 4 epochs; the first stops after 3, the second after 2


@functools.lru_cache(maxsize=None)
def _case(shape, seed=None):
    u, T, B, att, C = SHAPES[shape]
    return tro.make_case(u, T, B, C, att, seed=100 + shape if seed is None else seed)


class Job:
    """The device arguments of one job; `record` (another Job of the same shape) lends its d_idx / d_truth."""

    def __init__(self, shape, seed=None, record=None, masks=True, grads=True):
        from deepgrp_amd import _lib, training
        self.u, self.T, self.B, self.att, self.C = SHAPES[shape]
        self.case = dict(_case(shape, seed))
        if record is not None:
            self.case["idx"], self.case["truth"] = record.case["idx"], record.case["truth"]
            self.d_idx, self.d_truth = record.d_idx, record.d_truth
        else:
            self.d_idx, self.d_truth = torch.from_numpy(self.case["idx"]).cuda(), torch.from_numpy(self.case["truth"]).cuda()
        if not masks:
            self.case["masks"] = None
        self.with_grads = grads
        self.n = int(self.case["idx"].size)
        self.params = torch.from_numpy(training.flatten_weights(self.case["weights"])).cuda()
        self.starts = torch.from_numpy(self.case["starts"]).cuda()
        self.masks = torch.from_numpy(self.case["masks"]).cuda() if masks else None
        self.work_bytes = _lib.lib().dgrp_train_workspace_bytes(self.T, self.u, self.C, int(self.att), self.B)
        assert self.work_bytes > 0
        self.out = {}

    def outputs(self, key):
        """Fresh NaN-filled loss, gradients and workspace under `key`."""
        self.out[key] = (torch.full((1,), NAN, device="cuda"), torch.full_like(self.params, NAN),
                         torch.full(((self.work_bytes + 3) // 4,), NAN, device="cuda"))
        return self.out[key]

    def struct(self, key, **change):
        from deepgrp_amd import _lib
        loss, grads, work = self.outputs(key)
        f = dict(T=self.T, u=self.u, C=self.C, attention=int(self.att), d_params=self.params.data_ptr(), d_idx=self.d_idx.data_ptr(),
                 d_truth=self.d_truth.data_ptr(), n=self.n, d_starts=self.starts.data_ptr(), B=self.B,
                 d_masks=self.masks.data_ptr() if self.masks is not None else None, d_loss=loss.data_ptr(),
                 d_grads=grads.data_ptr() if self.with_grads else None, d_work=work.data_ptr(), work_bytes=self.work_bytes)
        f.update(change)
        return _lib.TrainJob(**f)

    def single(self):
        from deepgrp_amd import _lib
        j = self.struct("single")
        rc = _lib.lib().dgrp_train_step(j.T, j.u, j.C, j.attention, j.d_params, j.d_idx, j.d_truth, j.n, j.d_starts, j.B, j.d_masks,
                                        j.d_loss, j.d_grads, j.d_work, j.work_bytes, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "dgrp_train_step")

    def host(self, key):
        loss, grads, _work = self.out[key]
        return loss.cpu().numpy(), grads.cpu().numpy()


def _multi(jobs, key="multi", count=None, structs=None):
    from deepgrp_amd import _lib
    structs = [j.struct(key) for j in jobs] if structs is None else structs
    table = (_lib.TrainJob * len(structs))(*structs)
    return _lib.lib().dgrp_train_step_multi(table, len(structs) if count is None else count, torch.cuda.current_stream().cuda_stream)


def _cohort(name):
    five = lambda: [Job(s) for s in range(5)]
    if name.startswith("alone"):
        return [Job(int(name[-1]))]
    if name == "two":
        return [Job(0), Job(1)]
    if name == "five":
        return five()
    if name == "reversed":
        return five()[::-1]
    if name == "eight":                                                   # the repeats read the record of the first job of their shape
        jobs = five()
        return jobs + [Job(0, seed=7, record=jobs[0]), Job(3, seed=8, record=jobs[3]), Job(1, seed=9, record=jobs[1])]
    if name == "loss_only":
        return [Job(s, grads=s not in (1, 3)) for s in range(5)]
    if name == "no_masks":
        return [Job(s, masks=False) for s in range(5)]
    raise KeyError(name)


COHORTS = ["alone0", "alone1", "alone2", "alone3", "alone4", "two", "five", "reversed", "eight", "loss_only", "no_masks"]


@pytest.mark.parametrize("name", COHORTS)
def test_every_job_gets_the_bytes_of_the_single_call(name):
    from deepgrp_amd import _lib
    jobs = _cohort(name)
    if name == "eight":
        assert jobs[5].d_idx.data_ptr() == jobs[0].d_idx.data_ptr() and jobs[6].d_truth.data_ptr() == jobs[3].d_truth.data_ptr()
        assert not np.array_equal(jobs[5].case["starts"], jobs[0].case["starts"])
    for j in jobs:
        j.single()
    _lib.check(_multi(jobs), "dgrp_train_step_multi")
    for k, j in enumerate(jobs):
        (l1, g1), (lk, gk) = j.host("single"), j.host("multi")
        assert np.isfinite(l1).all() and l1.tobytes() == lk.tobytes(), f"job {k}: loss {l1} vs {lk}"
        if j.with_grads:
            assert np.isfinite(g1).all() and g1.tobytes() == gk.tobytes(), f"job {k}: {int((g1 != gk).sum())} gradient elements differ"
        else:
            assert np.isnan(g1).all() and np.isnan(gk).all(), f"job {k}: a loss-only job wrote gradients"


@pytest.fixture(scope="module")
def float64_reference():
    """(float64, float32) loss and gradients of the checker for the five shapes, computed once."""
    out = []
    for s in range(5):
        c = _case(s)
        args = (c["weights"], c["idx"], c["truth"], c["starts"], c["T"], c["masks"])
        out.append((tro.loss_and_grads(*args, torch.float64)[:2], tro.loss_and_grads(*args, torch.float32)[:2]))
    return out


def test_five_jobs_against_float64(float64_reference):
    from deepgrp_amd import _lib, training
    jobs = _cohort("five")
    _lib.check(_multi(jobs), "dgrp_train_step_multi")
    problems = []
    for k, (j, ((l64, g64), (l32, g32))) in enumerate(zip(jobs, float64_reference)):
        loss, flat = j.host("multi")
        grads = training.unflatten_weights(flat, j.u, j.C, j.att)
        e32, e = abs(l32 - l64) / abs(l64), abs(float(loss[0]) - l64) / abs(l64)
        print(f"job {k} loss: hip {e:.3e} float32 {e32:.3e}")
        if not e <= tro.bound(e32):
            problems.append(f"job {k} loss: {e:.3e} > {tro.bound(e32):.3e}")
        for name, want in g64.items():
            e32, e = tro.rel_err(g32[name], want), tro.rel_err(grads[name], want)
            print(f"job {k} {name}: hip {e:.3e} float32 {e32:.3e}")
            if not e <= tro.bound(e32):
                problems.append(f"job {k} {name}: {e:.3e} > {tro.bound(e32):.3e}")
    assert not problems, "; ".join(problems)


def test_a_second_call_gives_the_same_bytes():
    from deepgrp_amd import _lib
    jobs = _cohort("eight")
    _lib.check(_multi(jobs, "first"), "dgrp_train_step_multi")
    _lib.check(_multi(jobs, "second"), "dgrp_train_step_multi")
    for j in jobs:
        assert [a.tobytes() for a in j.host("first")] == [a.tobytes() for a in j.host("second")]


def _untouched(jobs, key):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for j in jobs for t in j.out[key])


def test_refusals_launch_nothing():
    from deepgrp_amd import _lib
    L = _lib.lib()
    jobs = [Job(0), Job(1), Job(3)]
    cases = [
        ("no jobs", dict(count=0), "0 jobs outside 1..8"),
        ("nine jobs", dict(structs=[j.struct("nine jobs") for j in jobs] * 3), "9 jobs outside 1..8"),
        ("units", dict(change=dict(u=257)), "job 1: training: 257 units outside 1..256"),
        ("short record", dict(change=dict(n=jobs[1].T - 1)), "job 1: training: record of 11 bases is shorter than the window"),
        ("unaligned", dict(change="unaligned"), "job 1: training: workspace NULL or not 16-byte aligned"),
        ("one byte short", dict(change=dict(work_bytes=jobs[1].work_bytes - 1)), f"job 1: training: workspace of {jobs[1].work_bytes - 1} bytes"),
        ("same workspace", dict(change="shared"), "job 2: training: workspace overlaps the workspace of job 1"),
    ]
    for key, kw, fragment in cases:
        structs = kw.get("structs") or [j.struct(key) for j in jobs]
        change = kw.get("change")
        if change == "unaligned":
            structs[1].d_work += 4
        elif change == "shared":
            shared = torch.full(((max(structs[1].work_bytes, structs[2].work_bytes) + 3) // 4,), NAN, device="cuda")
            structs[1].d_work = structs[2].d_work = shared.data_ptr()                # room for either job, were it to run
        elif change:
            for name, value in change.items():
                setattr(structs[1], name, value)
        rc = _multi(jobs, key, count=kw.get("count"), structs=structs)
        msg = L.dgrp_last_error().decode()
        assert rc != 0 and fragment in msg, (key, rc, msg)
        if key in ("units", "short record", "unaligned"):
            assert msg.startswith("job 1:"), msg
        assert _untouched(jobs, key), f"{key}: a refused call wrote to a job's outputs"
    assert L.dgrp_train_step_multi(None, 2, torch.cuda.current_stream().cuda_stream) != 0
    assert "NULL job list" in L.dgrp_last_error().decode()


# ------------------------------------------------------------------------------------------------ the trainer
def _record(n=3000):
    """A record with planted tandem repeats: class c is a run of period c, so that there is something to learn."""
    from deepgrp_amd import preprocessing
    rng = np.random.default_rng(42)
    idx = rng.integers(0, 4, n).astype(np.uint8)
    truth = np.zeros((5, n), np.int8)
    for c, (a, b) in zip((1, 2, 3, 4, 1, 2, 3, 4), ((150, 330), (500, 640), (800, 1010), (1200, 1330), (1500, 1700), (1900, 2100),
                                                     (2300, 2450), (2600, 2800))):
        idx[a:b] = np.resize(rng.integers(0, 4, c).astype(np.uint8), b - a)
        truth[c, a:b] = 1
    idx[rng.random(n) < 0.01] = 4
    truth[0, truth[1:].sum(0) == 0] = 1
    fwd = np.zeros((5, n), np.int8)
    fwd[idx, np.arange(n)] = 1
    return preprocessing.Data(fwd, truth)


def _files(logdir):
    return {name: open(os.path.join(logdir, name), "rb").read() for name in sorted(os.listdir(logdir))}


def _against_separate_runs(tmp, data, options, seeds):
    from deepgrp_amd import model, training
    weights = [model.initial_weights(o, s) for o, s in zip(options, seeds)]
    joint = training.training_multi((data, data), options, weights, [os.path.join(tmp, f"multi{k}") for k in range(len(options))], seeds)
    lengths = []
    for k, (o, s) in enumerate(zip(options, seeds)):
        alone = training.training((data, data), o, model.initial_weights(o, s), os.path.join(tmp, f"single{k}"), seed=s)
        assert joint[k]["history"] == alone["history"]
        for name in tro.NAMES:
            if alone[name] is None:
                assert joint[k][name] is None
            else:
                assert joint[k][name].tobytes() == alone[name].tobytes(), f"model {k}: {name}"
        a, b = _files(os.path.join(tmp, f"multi{k}")), _files(os.path.join(tmp, f"single{k}"))
        assert list(a) == list(b) and "history.tsv" in a and any(n.endswith(".hdf5") for n in a)
        assert a == b, f"model {k}: files differ"
        lengths.append(len(alone["history"]))
    return lengths


def test_training_multi_is_training_model_by_model(tmp_path):
    from deepgrp_amd.model import Options
    common = dict(n_epochs=4, n_batches=3, batch_size=16, early_stopping_th=1)
    options = [Options(units=8, vecsize=20, optimizer="RMSprop", dropout=0.25, **common),
               Options(units=12, vecsize=30, optimizer="Adam", attention=True, momentum=0.9, rho=0.999, epsilon=1e-7, **common),
               Options(units=8, vecsize=20, optimizer="RMSprop", dropout=0.25, learning_rate=LEARNING_RATE_OF_THE_THIRD, **common)]
    lengths = _against_separate_runs(str(tmp_path), _record(), options, [11, 12, 13])
    print("epochs run:", lengths)
    assert len(set(lengths)) > 1, "the models stopped in the same epoch: the early leaver is not exercised"


def test_training_multi_runs_more_models_than_one_launch_takes(tmp_path):
    from deepgrp_amd import _lib
    from deepgrp_amd.model import Options
    options = [Options(units=4 + 2 * (k % 3), vecsize=10 + k, n_epochs=2, n_batches=2, batch_size=4, attention=bool(k % 2),
                       learning_rate=0.001 * (k + 1)) for k in range(10)]
    assert len(options) > _lib.TRAIN_MAX_JOBS
    _against_separate_runs(str(tmp_path), _record(), options, list(range(20, 30)))


# ------------------------------------------------------------------------------------------------ the search
def _same(a, b):
    return (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b)) or a == b


def test_grouping_of_trials_does_not_matter(tmp_path, monkeypatch):
    from deepgrp_amd import optimization as dgopt
    from deepgrp_amd.model import Options
    data = _record()
    space = {"gru_units": ["qnormal", 8, 2, 2], "vecsize": ["qnormal", 24, 4, 2], "learning_rate": ["loguniform", -7.0, -3.0],
             "gru_dropout": ["uniform", 0.0, 0.4]}
    models = {}
    evaluate = dgopt._evaluate

    def recording(val_data, step_size, options, logdir):
        with open(dgopt._best_model_file(logdir), "rb") as fh:
            models[(options.project_root_dir, int(logdir[-4:]))] = (os.path.basename(dgopt._best_model_file(logdir)), fh.read())
        return evaluate(val_data, step_size, options, logdir)

    monkeypatch.setattr(dgopt, "_evaluate", recording)
    roots = {}
    for cohort in (3, 1):
        roots[cohort] = str(tmp_path / f"cohort{cohort}")
        base = Options(project_root_dir=roots[cohort], n_epochs=2, n_batches=3, batch_size=16, early_stopping_th=1)
        run = dgopt.build_and_optimize_cohort if cohort > 1 else dgopt.build_and_optimize
        done = dgopt.run_a_trial(space, functools.partial(run, data, data, 10, base), roots[cohort], 6, seed=3, cohort=cohort)
        assert 0 <= done <= 6
    with open(os.path.join(roots[3], "results.json")) as fa, open(os.path.join(roots[1], "results.json")) as fb:
        a, b = json.load(fa), json.load(fb)
    assert [t["tid"] for t in a] == [t["tid"] for t in b] == list(range(6))
    trained = 0
    for ta, tb in zip(a, b):
        print(ta["tid"], ta["status"], ta["loss"], ta["params"], ta["error"])
        assert ta["params"] == tb["params"] and ta["seed"] == tb["seed"] and ta["status"] == tb["status"], (ta, tb)
        assert _same(ta["loss"], tb["loss"]), (ta["loss"], tb["loss"])
        assert ta["error"] == tb["error"]
        ma, mb = models.get((roots[3], ta["tid"])), models.get((roots[1], ta["tid"]))
        assert (ma is None) == (mb is None) and ma == mb, f"trial {ta['tid']}: the best-epoch model files differ"
        trained += ma is not None
        if ta["status"] == "ok":
            assert os.path.isdir(ta["logdir"]) and ta["Metrics"]["MCC"] == -ta["loss"]
        else:
            assert ta["logdir"] is None
    assert trained >= 4, "most draws of this space are models the trainer takes"
