"""Host side of the hyper-parameter search (no GPU): the space, the bookkeeping of run_a_trial with stub objectives, the status
rules of a trial with the device work replaced, the refusals of training_multi and of the `optimize` command."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from deepgrp_amd import optimization as dgopt
from deepgrp_amd import preprocessing, synthetic, training
from deepgrp_amd.model import Options, create_logdir

SPACE = {"gru_units": ["qnormal", 34, 5, 2], "vecsize": ["quniform", 100, 300, 10], "learning_rate": ["loguniform", -9.0, -4.0],
         "momentum": ["uniform", 0.5, 1.0], "rho": ["normal", 0.9, 0.01], "epsilon": ["lognormal", -20.0, 1.0],
         "optimizer": ["choice", "RMSprop", "Adam"]}


def test_update_options_folds_aliases_and_casts():
    opt = dgopt._update_options(Options(), {"gru_units": 36.0, "vecsize": 198.0, "gru_dropout": 0.1, "learning_rate": 0.01})
    assert opt.units == 36 and type(opt.units) is int and opt.vecsize == 198 and type(opt.vecsize) is int
    assert opt.dropout == 0.1 and opt.learning_rate == 0.01
    assert "gru_units" not in opt.todict() and "gru_dropout" not in opt.todict()


def test_create_logdir_names():
    opt = Options(project_root_dir="/x")
    plain, numbered = create_logdir(opt), create_logdir(opt, 7)
    assert os.path.dirname(plain) == os.path.join("/x", "tf_logs") and os.path.basename(plain).startswith("run-")
    assert len(os.path.basename(plain)) == len("run-") + 14 and numbered.endswith("-0007")


def test_sample_space_seed_ranges_and_steps():
    a = dgopt.sample_space(SPACE, np.random.default_rng(4))
    assert a == dgopt.sample_space(SPACE, np.random.default_rng(4))
    assert a != dgopt.sample_space(SPACE, np.random.default_rng(5))
    assert list(a) == list(SPACE)
    draws = [dgopt.sample_space(SPACE, np.random.default_rng(s)) for s in range(300)]
    units = np.array([d["gru_units"] for d in draws])
    vec = np.array([d["vecsize"] for d in draws])
    assert np.all(units % 2 == 0) and 30 < units.mean() < 38 and len(set(units.tolist())) > 5
    assert np.all(vec % 10 == 0) and vec.min() >= 100 and vec.max() <= 300 and len(set(vec.tolist())) > 10
    lr = np.array([d["learning_rate"] for d in draws])
    assert lr.min() >= math.exp(-9.0) and lr.max() <= math.exp(-4.0)
    assert -7.0 < np.log(lr).mean() < -6.0                              # uniform in the exponent
    mom = np.array([d["momentum"] for d in draws])
    assert mom.min() >= 0.5 and mom.max() < 1.0
    assert abs(np.mean([d["rho"] for d in draws]) - 0.9) < 0.005
    eps = np.array([d["epsilon"] for d in draws])
    assert eps.min() > 0 and abs(np.log(eps).mean() + 20.0) < 0.3
    assert {d["optimizer"] for d in draws} == {"RMSprop", "Adam"}
    assert all(type(d["gru_units"]) is float for d in draws)


@pytest.mark.parametrize("entry,word", [
    (["gaussian", 0, 1], "unknown kind"), (["uniform", 0], "2 arguments"), (["qnormal", 1, 2], "3 arguments"),
    (["choice"], "at least one"), ("uniform", "list"), (["uniform", 2, 1], "low <= high"), (["quniform", 0, 1, 0], "q > 0"),
    (["normal", 0, "x"], "numbers"),
])
def test_sample_space_names_the_key(entry, word):
    with pytest.raises(ValueError, match="my_key") as exc:
        dgopt.sample_space({"learning_rate": ["uniform", 0, 1], "my_key": entry}, np.random.default_rng(0))
    assert word in str(exc.value)


# ------------------------------------------------------------------------------------------------ run_a_trial
def _stub(calls, fail=()):
    def one(draw):
        calls.append(draw)
        bad = draw.tid in fail
        return {"loss": np.inf if bad else -draw["momentum"], "Metrics": None if bad else {"MCC": draw["momentum"], "TPR": np.array([1.0, np.nan])},
                "options": {"units": 3}, "logdir": None if bad else f"run-{draw.tid}", "status": "fail" if bad else "ok",
                "error": "boom" if bad else ""}

    def objective(arg):
        if isinstance(arg, list):
            calls.append(len(arg))
            return [one(d) for d in arg]
        return one(arg)
    return objective


def _load(path):
    with open(os.path.join(path, "results.json")) as fh:
        return json.load(fh)


def test_run_a_trial_fresh_and_resumed(tmp_path):
    root, calls = str(tmp_path / "a"), []
    assert dgopt.run_a_trial(SPACE, _stub(calls), root, 3, seed=1) == 3
    first = _load(root)
    assert [t["tid"] for t in first] == [0, 1, 2] and all(isinstance(c, dgopt.Draw) for c in calls)
    assert all(set(t) >= {"loss", "Metrics", "options", "logdir", "status", "error", "tid", "params", "seed"} for t in first)
    assert first[0]["Metrics"]["TPR"][0] == 1.0 and math.isnan(first[0]["Metrics"]["TPR"][1])          # arrays as lists
    assert dgopt.run_a_trial(SPACE, _stub(calls), root, 2, seed=1) == 5
    second = _load(root)
    assert [t["tid"] for t in second] == [0, 1, 2, 3, 4] and second[:3] == first


def test_run_a_trial_grouping_and_resuming_do_not_change_a_trial(tmp_path):
    roots = {name: str(tmp_path / name) for name in ("one", "four", "resumed", "other")}
    calls = {name: [] for name in roots}
    assert dgopt.run_a_trial(SPACE, _stub(calls["one"]), roots["one"], 10, seed=9) == 10
    assert dgopt.run_a_trial(SPACE, _stub(calls["four"]), roots["four"], 10, seed=9, cohort=4) == 10
    assert [c for c in calls["four"] if isinstance(c, int)] == [4, 4, 2]
    assert dgopt.run_a_trial(SPACE, _stub(calls["resumed"]), roots["resumed"], 5, seed=9, cohort=4) == 5
    assert dgopt.run_a_trial(SPACE, _stub(calls["resumed"]), roots["resumed"], 5, seed=9) == 10
    dgopt.run_a_trial(SPACE, _stub(calls["other"]), roots["other"], 10, seed=10)
    want = _load(roots["one"])
    for name in ("four", "resumed"):
        got = _load(roots[name])
        assert [(t["tid"], t["params"], t["seed"]) for t in got] == [(t["tid"], t["params"], t["seed"]) for t in want]
    assert len({t["seed"] for t in want}) == 10 and all(isinstance(t["seed"], int) and t["seed"] >= 0 for t in want)
    assert [t["params"] for t in _load(roots["other"])] != [t["params"] for t in want]
    tids = [d.tid for d in calls["four"] if not isinstance(d, int)]
    assert tids == list(range(10))


def test_run_a_trial_keeps_failed_trials_but_does_not_count_them(tmp_path):
    root, calls = str(tmp_path), []
    assert dgopt.run_a_trial(SPACE, _stub(calls, fail=(1, 4)), root, 6, seed=2, cohort=3) == 4
    trials = _load(root)
    assert [t["status"] for t in trials] == ["ok", "fail", "ok", "ok", "fail", "ok"]
    assert trials[1]["loss"] == math.inf and trials[1]["error"] == "boom"
    with pytest.raises(ValueError, match="results for"):
        dgopt.run_a_trial(SPACE, lambda draws: [], root, 2, seed=2, cohort=2)


# ------------------------------------------------------------------------------------------------ one trial, device work replaced
def _data(n=600, classes=3):
    fwd = np.zeros((5, n), np.int8)
    fwd[np.arange(n) % 4, np.arange(n)] = 1
    y = np.zeros((classes, n), np.int8)
    y[1, 100:200] = 1
    y[0, y[1:].sum(0) == 0] = 1
    return preprocessing.Data(fwd, y)


@pytest.fixture
def patched(monkeypatch, tmp_path):
    """training, predict_complete, filter_segments and calculate_metrics replaced; `state` steers them and records the calls."""
    from deepgrp_amd import prediction
    state = {"mcc": 1.0, "raise": None, "trained": [], "filtered": [], "predicted": []}

    def fake_training(data, options, weights, logdir, seed=None, log=None):
        state["trained"].append((options.units, options.vecsize, logdir, seed))
        os.makedirs(logdir, exist_ok=True)
        for name in ("01.hdf5", "03.hdf5"):
            open(os.path.join(logdir, name), "w").close()
        if state["raise"] == "training":
            raise RuntimeError("training broke")
        return {}

    def fake_predict(step_size, options, logdir, data, use_mss=False):
        state["predicted"].append((step_size, logdir, use_mss))
        if state["raise"] == "predict":
            raise RuntimeError("prediction broke")
        out = np.zeros((data.truelbl.shape[1], data.truelbl.shape[0]))
        out[:, 0] = 1.0
        out[-5:] = np.nan
        return out

    def fake_filter(array, min_len=50):
        state["filtered"].append((len(array), min_len))

    def fake_metrics(pred, true):
        assert len(pred) == len(true)
        return np.eye(2), {"MCC": state["mcc"], "TPR": np.array([1.0, 0.5])}

    monkeypatch.setattr(training, "training", fake_training)
    monkeypatch.setattr(prediction, "predict_complete", fake_predict)
    monkeypatch.setattr(prediction, "filter_segments", fake_filter)
    monkeypatch.setattr(prediction, "calculate_metrics", fake_metrics)
    state["options"] = Options(project_root_dir=str(tmp_path), repeats_to_search=[1, 2], min_mss_len=40)
    return state


def test_build_and_optimize_ok(patched):
    data, base = _data(), patched["options"]
    res = dgopt.build_and_optimize(data, data, 25, base, dgopt.Draw({"gru_units": 12.0, "vecsize": 30.0}, tid=3, seed=77))
    assert res["status"] == "ok" and res["loss"] == -1.0 and res["error"] == "" and res["Metrics"]["MCC"] == 1.0
    assert res["options"]["units"] == 12 and res["options"]["vecsize"] == 30
    assert base.units == 32                                               # the caller's options are left alone
    assert os.path.isdir(res["logdir"]) and res["logdir"].endswith("-0003")
    assert os.path.dirname(res["logdir"]) == os.path.join(base.project_root_dir, "tf_logs")
    assert patched["trained"] == [(12, 30, res["logdir"], 77)]
    assert patched["predicted"] == [(25, os.path.join(res["logdir"], "03.hdf5"), True)]           # the best epoch's file
    assert patched["filtered"] == [(600 - 5, 40)]                         # rows of NaN are dropped first


def test_build_and_optimize_nan_mcc_fails(patched):
    patched["mcc"] = float("nan")
    data = _data()
    res = dgopt.build_and_optimize(data, data, 25, patched["options"], {"gru_units": 8})
    assert res["status"] == "fail" and res["loss"] == np.inf
    assert not os.path.exists(patched["trained"][0][2])                   # a failed trial's logdir is removed


@pytest.mark.parametrize("where", ["training", "predict"])
def test_build_and_optimize_exception_fails(patched, where):
    patched["raise"] = where
    data = _data()
    res = dgopt.build_and_optimize(data, data, 25, patched["options"], {"gru_units": 8})
    assert res["status"] == "fail" and res["loss"] == np.inf and "broke" in res["error"] and res["logdir"] is None
    assert len(patched["trained"]) == 1 and not os.path.exists(patched["trained"][0][2])


@pytest.mark.parametrize("values,word", [({"gru_units": 0.4}, "units"), ({"vecsize": -2.0}, "vecsize"), ({"gru_units": 300}, "units")])
def test_build_and_optimize_refused_options_fail_without_training(patched, values, word):
    data = _data()
    res = dgopt.build_and_optimize(data, data, 25, patched["options"], values)
    assert res["status"] == "fail" and res["loss"] == np.inf and word in res["error"] and res["logdir"] is None
    assert patched["trained"] == [] and patched["predicted"] == []
    assert not os.path.exists(os.path.join(patched["options"].project_root_dir, "tf_logs"))
    many = dgopt.build_and_optimize_cohort(data, data, 25, patched["options"], [values, values])
    assert [r["status"] for r in many] == ["fail", "fail"] and all(word in r["error"] for r in many)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", ["n_batches", "n_epochs"])
def test_training_multi_refuses_unequal_schedules_by_name(name, tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(training, "DeviceRecord", type("R", (), {"from_data": staticmethod(no_device)}))
    monkeypatch.setattr(training, "DeviceTrainer", no_device)
    data = _data()
    a, b = Options(repeats_to_search=[1, 2], vecsize=20), Options(repeats_to_search=[1, 2], vecsize=20, **{name: 7})
    with pytest.raises(training.TrainingRefused, match=name):
        training.training_multi((data, data), [a, b], [{}, {}], [str(tmp_path / "a"), str(tmp_path / "b")], [1, 2])
    assert not os.path.exists(str(tmp_path / "a"))
    with pytest.raises(training.TrainingRefused, match="units"):
        training.training_multi((data, data), [a, Options(units=0)], [{}, {}], ["x", "y"], [1, 2])
    with pytest.raises(ValueError, match="one length"):
        training.training_multi((data, data), [a, b], [{}], ["x", "y"], [1, 2])


def _write_inputs(tmp, space_text):
    n = 3000
    idx, _lab = synthetic.synthetic_truth(n, contig=3, flank=50)
    fwd = np.zeros((5, n), np.int8)
    fwd[idx, np.arange(n)] = 1
    paths = {}
    for role in ("train", "valid"):
        paths[role] = os.path.join(tmp, f"chrA{role}.fa.gz.npz")
        np.savez(paths[role], fwd=fwd)
    paths["bed"] = os.path.join(tmp, "rm.bed")
    with open(paths["bed"], "w") as fh:
        fh.writelines(synthetic.synthetic_annotation(n, contig=3, name="chrAtrain", flank=50))
    paths["toml"] = os.path.join(tmp, "p.toml")
    with open(paths["toml"], "w") as fh:
        fh.write("units = 4\nvecsize = 20\nn_epochs = 1\nn_batches = 1\n")
    paths["space"] = os.path.join(tmp, "space.toml")
    with open(paths["space"], "w") as fh:
        fh.write(space_text)
    return paths


GOOD_SPACE = '[space]\ngru_units = ["qnormal", 34, 5, 2]\n'


@pytest.mark.parametrize("space,env,extra,missing,words", [
    (GOOD_SPACE, None, [], "bed", ("no such file", "rm.bed")),
    (GOOD_SPACE, None, [], "space", ("no such file", "space.toml")),
    ('[space]\ngru_units = ["qgauss", 34, 5, 2]\n', None, [], None, ("gru_units", "unknown kind", "qgauss")),
    ('[space]\nvecsize = ["qnormal", 200, 20]\n', None, [], None, ("vecsize", "3 arguments")),
    ('gru_units = ["qnormal", 34, 5, 2]\n', None, [], None, ("[space]",)),
    (GOOD_SPACE, {"WORLD_SIZE": "2"}, [], None, ("WORLD_SIZE",)),
    (GOOD_SPACE, None, ["--cohort", "65"], None, ("--cohort", "65")),
    (GOOD_SPACE, None, ["--cohort", "0"], None, ("--cohort", "0")),
])
def test_optimize_refuses_before_device_work(tmp_path, space, env, extra, missing, words):
    tmp = str(tmp_path)
    paths = _write_inputs(tmp, space)
    if missing:
        os.remove(paths[missing])
    root = os.path.join(tmp, "root")
    cmd = [sys.executable, "-m", "deepgrp_amd", "optimize", paths["space"], paths["toml"], paths["train"], paths["valid"], paths["bed"],
           "--project_root_dir", root, "--max_evals", "2"] + extra
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env={**os.environ, **(env or {})})
    assert res.returncode != 0
    for word in words:
        assert word in res.stderr, res.stderr
    assert "Traceback" not in res.stderr
    assert not os.path.exists(os.path.join(root, "results.json")) and not os.path.exists(os.path.join(root, "tf_logs"))


def test_symbols_and_the_job_struct():
    import ctypes as C
    from deepgrp_amd import _lib
    assert "dgrp_train_step_multi" in _lib.exported_symbols()
    assert _lib.TRAIN_MAX_JOBS == 8
    names = [f[0] for f in _lib.TrainJob._fields_]
    assert names == ["T", "u", "C", "attention", "d_params", "d_idx", "d_truth", "n", "d_starts", "B", "d_masks", "d_loss", "d_grads",
                     "d_work", "work_bytes"]
    assert C.sizeof(_lib.TrainJob) == 104                                 # 4 ints, 11 eight-byte fields
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    assert "#define DGRP_TRAIN_MAX_JOBS 8" in header and "} dgrp_train_job;" in header


def test_refusals_of_the_multi_entry_need_no_device():
    """Counts, NULL and a job's sizes are refused on the host; the message names the job."""
    from deepgrp_amd import _lib
    L = _lib.lib()
    job = lambda u=20, n=100, work=0x1000: _lib.TrainJob(7, u, 5, 1, 0x1000, 0x1000, 0x1000, n, 0x1000, 4, None, 0x1000, 0x1000, work, 1 << 40)
    table = lambda *jobs: (_lib.TrainJob * len(jobs))(*jobs)
    for k, word in ((0, "0 jobs"), (9, "9 jobs")):
        assert L.dgrp_train_step_multi(table(*[job()] * 9), k, None) == -1 and word.encode() in L.dgrp_last_error()
    assert L.dgrp_train_step_multi(None, 1, None) == -1 and b"NULL job list" in L.dgrp_last_error()
    for bad, word in ((job(u=257), "257 units outside 1..256"), (job(n=6), "shorter than the window"), (job(work=0x1004), "aligned")):
        assert L.dgrp_train_step_multi(table(job(), bad, job(work=0x100000)), 3, None) != 0
        msg = L.dgrp_last_error().decode()
        assert msg.startswith("job 1: training: ") and word in msg, msg
    assert L.dgrp_train_step_multi(table(job(), job(work=0x2000000), job()), 3, None) == -1
    assert L.dgrp_last_error().decode().startswith("job 2: training: workspace overlaps the workspace of job 0")
