"""deepgrp_amd.optimization -- mirror of deepgrp/optimization.py: the hyper-parameter search.

The reference drives hyperopt's TPE over a space of hyperopt expressions, trains every trial with Keras and keeps the trials in
a pickle.  Here the search is SEEDED RANDOM SEARCH: trial `tid` is drawn from ``default_rng(SeedSequence([seed, tid]))``, so a
trial depends neither on the trials before it nor on how a run was split or resumed, and any number of trials can be trained
side by side (``training.training_multi``: up to eight models per launch chain).  TPE is not built.  A space is a dict
``name -> (kind, *args)`` with hyperopt's definitions of the kinds (``sample_space``); the trials are kept in
``<project_root_dir>/results.json``.  No TensorBoard output.
"""
from __future__ import annotations

import json
import logging
import os
import shutil
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

from . import model as dgmodel
from . import training as dgtrain
from .model import Options
from .preprocessing import Data

_LOG = logging.getLogger(__name__)

STATUS_OK, STATUS_FAIL = "ok", "fail"                # hyperopt's strings

# kind -> number of arguments (None: one or more)
KINDS = {"uniform": 2, "quniform": 3, "normal": 2, "qnormal": 3, "loguniform": 2, "lognormal": 2, "choice": None}


class Draw(dict):
    """The values drawn for one trial, with the trial's number and the seed of its training."""

    def __init__(self, values: Dict[str, Any], tid: Optional[int] = None, seed: Optional[int] = None):
        super().__init__(values)
        self.tid, self.seed = tid, seed


def _update_options(options: Options, dictionary: Dict[str, Any]) -> Options:
    for key, value in dictionary.items():
        options[key] = value
    options.vecsize = int(options.vecsize)
    options.units = int(options.units)
    return options


# ------------------------------------------------------------------------------------------------ space
def check_space(space: Dict[str, Sequence[Any]]) -> None:
    """Raises ValueError naming the key of an entry that is no ``(kind, *args)`` of a known kind and argument count."""
    for key, entry in space.items():
        if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__") or len(entry) < 1 or not isinstance(entry[0], str):
            raise ValueError(f"{key}: an entry of the space is a list [kind, arguments ...], found {entry!r}")
        kind, args = entry[0], list(entry[1:])
        if kind not in KINDS:
            raise ValueError(f"{key}: unknown kind {kind!r}; the kinds are {', '.join(KINDS)}")
        if KINDS[kind] is None:
            if not args:
                raise ValueError(f"{key}: choice needs at least one value")
            continue
        if len(args) != KINDS[kind]:
            raise ValueError(f"{key}: {kind} takes {KINDS[kind]} arguments, {len(args)} given")
        if not all(isinstance(a, (int, float)) and not isinstance(a, bool) for a in args):
            raise ValueError(f"{key}: {kind} takes numbers, found {args!r}")
        if kind in ("uniform", "quniform", "loguniform") and not args[0] <= args[1]:
            raise ValueError(f"{key}: {kind} needs low <= high, found {args[0]} and {args[1]}")
        if kind in ("normal", "qnormal", "lognormal") and not args[1] >= 0:
            raise ValueError(f"{key}: {kind} needs sigma >= 0, found {args[1]}")
        if kind in ("quniform", "qnormal") and not args[2] > 0:
            raise ValueError(f"{key}: {kind} needs q > 0, found {args[2]}")


def sample_space(space: Dict[str, Sequence[Any]], rng: np.random.Generator) -> Dict[str, Any]:
    """One draw of every entry, in the order of the dict.  Kinds, as hyperopt defines them: uniform(lo, hi); quniform(lo, hi, q) =
    round(uniform / q) * q; normal(mu, sigma); qnormal(mu, sigma, q) = round(normal / q) * q; loguniform(lo, hi) =
    exp(uniform(lo, hi)); lognormal(mu, sigma) = exp(normal(mu, sigma)); choice(v0, v1, ...).  Numbers come back as Python floats."""
    check_space(space)
    out: Dict[str, Any] = {}
    for key, entry in space.items():
        kind, args = entry[0], list(entry[1:])
        if kind == "choice":
            value = args[int(rng.integers(len(args)))]
        else:
            value = rng.uniform(args[0], args[1]) if "uniform" in kind else rng.normal(args[0], args[1])
            if kind.startswith("log"):
                value = np.exp(value)
            if kind.startswith("q"):
                value = np.round(value / args[2]) * args[2]
            value = float(value)
        out[key] = value
    return out


# ------------------------------------------------------------------------------------------------ one trial
def _new_result(options: Options) -> Dict[str, Any]:
    return {"loss": np.inf, "Metrics": None, "options": options.todict(), "logdir": None, "status": STATUS_FAIL, "error": ""}


def _prepare(options: Options, options_dict: Dict[str, Any]):
    """The trial's own options (the caller's are left alone) and its result dict; status "fail" with the refusal when
    check_options refuses them (a drawn qnormal can be below 1), else still to be trained (logdir set)."""
    options = _update_options(Options(**options.todict()), options_dict)
    result = _new_result(options)
    try:
        dgtrain.check_options(options)
    except dgtrain.TrainingRefused as err:
        result["error"] = str(err)
        return options, result
    result["logdir"] = dgmodel.create_logdir(options, getattr(options_dict, "tid", None))
    return options, result


def _best_model_file(logdir: str) -> str:
    """The best epoch is the last one written (save_best_only): the highest NN.hdf5."""
    files = sorted(f for f in os.listdir(logdir) if f.endswith(".hdf5"))
    if not files:
        raise FileNotFoundError(f"{logdir}: training wrote no model file")
    return os.path.join(logdir, files[-1])


def _evaluate(val_data: Data, step_size: int, options: Options, logdir: str) -> Dict[str, Any]:
    from . import prediction as dgpred
    predictions = dgpred.predict_complete(step_size, options, _best_model_file(logdir), val_data, use_mss=True)
    is_not_na = np.logical_not(np.isnan(predictions[:, 0]))
    predictions_class = predictions[is_not_na].argmax(axis=1)
    dgpred.filter_segments(predictions_class, options.min_mss_len)
    _, metrics = dgpred.calculate_metrics(predictions_class, val_data.truelbl[:, is_not_na].argmax(axis=0))
    return metrics


def _finish(result: Dict[str, Any], error: Optional[BaseException], metrics: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The reference's bookkeeping: loss = -MCC; an exception or a NaN MCC is a failed trial, whose logdir is removed."""
    logdir = result["logdir"]
    if error is not None:
        result.update(error=str(error), status=STATUS_FAIL, logdir=None)
    else:
        result.update(loss=-1 * metrics["MCC"], status=STATUS_OK, Metrics=metrics)
        if np.isnan(result["loss"]):
            result.update(status=STATUS_FAIL, loss=np.inf)
    if result["status"] == STATUS_FAIL and logdir:
        shutil.rmtree(logdir, ignore_errors=True)
    return result


def build_and_optimize(train_data: Data, val_data: Data, step_size: int, options: Options,
                       options_dict: Dict[str, Any]) -> Dict[str, Any]:
    """One trial (deepgrp/optimization.py:32-106): a model with `options` updated by `options_dict` is trained, the validation
    record is predicted (``predict_complete(..., use_mss=True)``), rows of NaN are dropped, segments shorter than `min_mss_len`
    are cleared and the metrics are taken against the truth's argmax.  Returns the reference's result dict: loss (-MCC),
    Metrics, options, logdir, status, error.  Options the trainer refuses make a failed trial before any device work.  A
    ``Draw`` brings the trial's number (for the logdir) and the seed of the initial weights and of the training."""
    options, result = _prepare(options, options_dict)
    if not result["logdir"]:
        return result
    seed = getattr(options_dict, "seed", None)
    try:
        dgmodel.reset_layer_names()
        weights = dgmodel.initial_weights(options, seed)
        dgtrain.training((train_data, val_data), options, weights, result["logdir"], seed=seed)
        metrics = _evaluate(val_data, step_size, options, result["logdir"])
    except Exception as err:  # pylint: disable=broad-except
        _LOG.exception("Error occurred while training")
        return _finish(result, err, None)
    return _finish(result, None, metrics)


def build_and_optimize_cohort(train_data: Data, val_data: Data, step_size: int, options: Options,
                              options_dicts: Sequence[Dict[str, Any]]) -> List[Dict[str, Any]]:
    """The trials of `options_dicts` trained side by side (``training.training_multi``), then evaluated one after another
    (prediction uses the whole device already).  Element k is what ``build_and_optimize`` returns for options_dicts[k], the name
    of the logdir apart.  Trials whose options are refused, or whose training or evaluation raises, fail alone: when the joint
    training raises, its trials are trained one by one."""
    prepared = [_prepare(options, d) for d in options_dicts]
    seeds = [getattr(d, "seed", None) for d in options_dicts]
    errors: Dict[int, BaseException] = {}
    groups: Dict[Any, List[int]] = {}
    for k, (opt, result) in enumerate(prepared):
        if result["logdir"]:
            groups.setdefault((int(opt.n_batches), int(opt.n_epochs)), []).append(k)

    def train(ks: List[int]) -> None:
        dgmodel.reset_layer_names()
        weights = [dgmodel.initial_weights(prepared[k][0], seeds[k]) for k in ks]
        dgtrain.training_multi((train_data, val_data), [prepared[k][0] for k in ks], weights,
                               [prepared[k][1]["logdir"] for k in ks], [seeds[k] for k in ks])

    for ks in groups.values():
        try:
            train(ks)
        except Exception as joint:  # pylint: disable=broad-except
            if len(ks) == 1:
                _LOG.exception("Error occurred while training")
                errors[ks[0]] = joint
                continue
            _LOG.warning("training %d trials side by side failed (%s): training them one by one", len(ks), joint)
            for k in ks:
                try:
                    shutil.rmtree(prepared[k][1]["logdir"], ignore_errors=True)
                    train([k])
                except Exception as err:  # pylint: disable=broad-except
                    _LOG.exception("Error occurred while training")
                    errors[k] = err
    results = []
    for k, (opt, result) in enumerate(prepared):
        if not result["logdir"]:
            results.append(result)
            continue
        metrics = None
        if k not in errors:
            try:
                metrics = _evaluate(val_data, step_size, opt, result["logdir"])
            except Exception as err:  # pylint: disable=broad-except
                _LOG.exception("Error occurred while evaluating")
                errors[k] = err
        results.append(_finish(result, errors.get(k), metrics))
    return results


# ------------------------------------------------------------------------------------------------ the search
def _jsonable(value: Any) -> Any:
    if isinstance(value, dict):
        return {str(k): _jsonable(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_jsonable(v) for v in value]
    if isinstance(value, np.ndarray):
        return _jsonable(value.tolist())
    if isinstance(value, np.generic):
        return value.item()
    return value


def trial_seed(seed: int, tid: int) -> np.random.SeedSequence:
    return np.random.SeedSequence([int(seed), int(tid)])


def run_a_trial(space: Dict[str, Sequence[Any]], objective: Callable[[Any], Any], project_root_dir, max_evals: int,
                seed: Optional[int] = None, cohort: int = 1) -> int:
    """Adds `max_evals` trials of seeded random search to ``<project_root_dir>/results.json`` (deepgrp/optimization.py:109-154
    with hyperopt's TPE and its pickle; TPE is not built), resuming that file if present.  Trial `tid` (its index in the file) is
    drawn by ``sample_space(space, default_rng(SeedSequence([seed, tid])))`` and carries a seed for its training derived from the
    same pair, so it depends neither on the grouping nor on where a run was resumed.  With ``cohort == 1`` the objective is
    called with one ``Draw`` (a dict) per trial and returns a result dict; otherwise with lists of at most `cohort` consecutive
    draws, returning a list of result dicts.  The file is rewritten after every call: a list of result dicts with `tid`,
    `params` and `seed` added, arrays as lists.  Returns the number of trials in the file whose loss is recorded (status ok);
    failed trials stay in the file and are not counted.  Without `seed` a fresh one is taken from the system."""
    check_space(space)
    if cohort < 1:
        raise ValueError(f"cohort = {cohort}: at least 1")
    os.makedirs(project_root_dir, exist_ok=True)
    results_path = os.path.join(project_root_dir, "results.json")
    _LOG.info("Attempt to resume a past training if it exists:")
    try:
        with open(results_path, "r") as file:
            trials = json.load(file)
    except FileNotFoundError:
        trials = []
        _LOG.info("Starting from scratch: new trials.")
    else:
        _LOG.warning("Found saved trials! Loading...")
        _LOG.info("Rerunning from %d trials to add another %d.", len(trials), max_evals)
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    first, last = len(trials), len(trials) + int(max_evals)
    for start in range(first, last, cohort):
        draws = []
        for tid in range(start, min(last, start + cohort)):
            sequence = trial_seed(seed, tid)
            values = sample_space(space, np.random.default_rng(sequence))
            draws.append(Draw(values, tid, int(sequence.generate_state(1, np.uint64)[0] >> np.uint64(1))))
        got = [objective(draws[0])] if cohort == 1 else list(objective(draws))
        if len(got) != len(draws):
            raise ValueError(f"the objective returned {len(got)} results for {len(draws)} trials")
        for draw, result in zip(draws, got):
            trials.append(_jsonable({**result, "tid": draw.tid, "params": dict(draw), "seed": draw.seed}))
        with open(results_path + ".tmp", "w") as file:
            json.dump(trials, file, indent=1)
        os.replace(results_path + ".tmp", results_path)
    return sum(1 for t in trials if t.get("status") == STATUS_OK)
