"""deepgrp_amd.training -- mirror of deepgrp/training.py: the class-balanced window sampler, and the training loop on the GPU.

The reference hands a Keras model to ``model.fit``; here the step (forward over a batch of windows, loss, backward through time,
optimizer) is libdeepgrp_hip's ``dgrp_train_step`` / ``dgrp_optimizer_step`` on one flat float32 parameter buffer.  The sampler
returns START POSITIONS into the record instead of copied windows: the record's class indices and its truth stay on the device.

Differences from the reference, all stated in DESIGN.md: no TensorBoard output and no TensorFlow checkpoint bundles (the best epoch
is written as ``<logdir>/<epoch:02d>.hdf5``, a Keras HDF5 file), the GRU cell's dropout mask is constant over the steps of a window,
and ``seed`` makes a run reproducible byte for byte.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Any, Callable, Dict, Iterator, List, Optional, Tuple

import numpy as np

from . import preprocessing
from .model import Options, keras_config, save_keras_hdf5

_LOG = logging.getLogger(__name__)

OPTIMIZERS = {"rmsprop": 0, "adam": 1}          # DGRP_OPT_* of include/deepgrp_hip.h
_TENSORS = ("kernel", "recurrent_kernel", "bias", "scale", "ff_kernel", "ff_bias")


class TrainingRefused(ValueError):
    """An option the trainer does not take; raised before any device work."""


def check_options(options: Options) -> None:
    """The refusals: each names the option."""
    if str(options.rnn).upper() != "GRU":
        raise TrainingRefused(f"rnn = {options.rnn!r}: only rnn = \"GRU\" can be trained here")
    if str(options.optimizer).lower() not in OPTIMIZERS:
        raise TrainingRefused(f"optimizer = {options.optimizer!r}: only optimizer = \"RMSprop\" or \"Adam\" can be trained here")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        raise TrainingRefused(f"WORLD_SIZE = {world}: training runs in one process on one GPU")
    classes = len(options.repeats_to_search) + 1
    if not 1 <= int(options.units) <= 256:
        raise TrainingRefused(f"units = {options.units}: the training kernels take 1..256 units")
    if not 2 <= classes <= 16:
        raise TrainingRefused(f"repeats_to_search gives {classes} classes: the training kernels take 2..16")
    if not 1 <= int(options.vecsize) <= 4096:
        raise TrainingRefused(f"vecsize = {options.vecsize}: the training kernels take windows of 1..4096 bases")
    if int(options.n_batches) < 1:
        raise TrainingRefused(f"n_batches = {options.n_batches}: an epoch needs at least one step")
    if int(options.n_epochs) < 1:
        raise TrainingRefused(f"n_epochs = {options.n_epochs}: at least one epoch is needed")
    if int(options.batch_size) < 1:
        raise TrainingRefused(f"batch_size = {options.batch_size}: at least one window is needed")
    if not 0.0 <= float(options.dropout) < 1.0:
        raise TrainingRefused(f"dropout = {options.dropout}: a rate in [0, 1) is needed")


# ------------------------------------------------------------------------------------------------ sampler
def _calc_indices(array: np.ndarray, vecsize: int) -> np.ndarray:
    """Starts of the windows that hold at least one base of the class row `array` (deepgrp/training.py:76-81), the reference's
    arithmetic kept: position p stands for the window (p - vecsize, p], and start 0 is left out."""
    sums = np.asarray(array).cumsum()
    sums[vecsize:] = sums[vecsize:] - sums[:-vecsize]
    indices = np.where(sums > 0)[0] - vecsize
    return indices[indices > 0]


def fetch_batch(options: Options, data: preprocessing.Data,
                rng: Optional[np.random.Generator] = None) -> Callable[[], Iterator[np.ndarray]]:
    """The class-balanced sampler of deepgrp/training.py:84-132, returning int64 START POSITIONS [batch_size] per batch instead of
    copied windows: ``int(batch_size * repeat_probability / (C - 1))`` starts from every repeat class whose index set is larger
    than that, the rest uniform over [0, N - vecsize), then shuffled.  Draws from `rng` (a seeded generator gives the same batches)."""
    rng = np.random.default_rng() if rng is None else rng
    nclass, length = data.truelbl.shape
    one_class_size = int(options.batch_size * options.repeat_probability / (nclass - 1))
    batch_indices = [idx for idx in (_calc_indices(data.truelbl[i], options.vecsize) for i in range(1, nclass))
                     if idx.size > one_class_size]
    filled = one_class_size * len(batch_indices)
    if length - options.vecsize < 1:
        raise ValueError(f"the record has {length} bases: no window of {options.vecsize} fits")

    def get_batch() -> Iterator[np.ndarray]:
        while True:
            indices = np.empty(options.batch_size, dtype=np.int64)
            for i, bindex in enumerate(batch_indices):
                indices[one_class_size * i:one_class_size * (i + 1)] = rng.choice(bindex, one_class_size)
            indices[filled:] = rng.integers(0, length - options.vecsize, size=options.batch_size - filled)
            rng.shuffle(indices)
            yield indices

    return get_batch


def dropout_masks(rng: np.random.Generator, batch_size: int, rate: float) -> Optional[np.ndarray]:
    """Input dropout masks of the GRU cell [batch, 2, 5] float32: 0 with probability `rate`, else 1 / (1 - rate); one value per
    (window, direction, input channel), constant over the steps.  None without dropout."""
    if rate <= 0.0:
        return None
    keep = rng.random((batch_size, 2, 5)) >= rate
    return (keep / (1.0 - rate)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ parameters
def flatten_weights(w: Dict[str, Any]) -> np.ndarray:
    """Keras tensors -> the flat float32 buffer of dgrp_train_step (kernel, recurrent_kernel, bias, scale, FF/kernel, FF/bias)."""
    return np.concatenate([np.asarray(w[k], np.float32).reshape(-1) for k in _TENSORS if w.get(k) is not None])


def unflatten_weights(flat: np.ndarray, units: int, classes: int, attention: bool) -> Dict[str, Any]:
    u, rows = int(units), (2 if attention else 1) * int(units)
    shapes = [("kernel", (5, 3 * u)), ("recurrent_kernel", (u, 3 * u)), ("bias", (2, 3 * u))]
    if attention:
        shapes.append(("scale", (u,)))
    shapes += [("ff_kernel", (rows, classes)), ("ff_bias", (classes,))]
    out: Dict[str, Any] = {"scale": None}
    pos = 0
    flat = np.asarray(flat, np.float32).reshape(-1)
    for name, shape in shapes:
        size = int(np.prod(shape))
        out[name] = flat[pos:pos + size].reshape(shape).copy()
        pos += size
    if pos != flat.size:
        raise ValueError(f"{flat.size} parameters, {pos} expected")
    return out


def onehot_to_index(fwd: np.ndarray) -> np.ndarray:
    """int8 one-hot [5, N] (preprocess_sequence's `fwd`) -> class index uint8 [N]; every column must hold exactly one 1."""
    fwd = np.asarray(fwd)
    if fwd.ndim != 2 or fwd.shape[0] != 5:
        raise ValueError(f"expected a one-hot array of shape [5, N], found {fwd.shape}")
    if not ((fwd.sum(axis=0) == 1).all() and ((fwd == 0) | (fwd == 1)).all()):
        raise ValueError("the sequence array is not one-hot: a column without exactly one 1")
    return fwd.argmax(axis=0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ device
class DeviceRecord:
    """A record's class indices and multi-hot truth on the device."""

    def __init__(self, idx: np.ndarray, truth: np.ndarray):
        import torch
        idx = np.ascontiguousarray(idx, np.uint8)
        truth = np.ascontiguousarray(truth, np.int8)
        if truth.ndim != 2 or truth.shape[1] != idx.size:
            raise ValueError(f"truth {truth.shape} does not match {idx.size} bases")
        self.n, self.classes = int(idx.size), int(truth.shape[0])
        self.d_idx = torch.from_numpy(idx).cuda()
        self.d_truth = torch.from_numpy(truth).cuda()

    @classmethod
    def from_data(cls, data: preprocessing.Data) -> "DeviceRecord":
        return cls(onehot_to_index(data.fwd), data.truelbl)


class DeviceTrainer:
    """Parameters, gradients, optimizer state and workspace of one model on the device, and the two entry points around them."""

    def __init__(self, weights: Dict[str, Any], vecsize: int, batch_size: int):
        import torch
        from . import _lib
        self._lib, self._torch = _lib, torch
        L = _lib.lib()
        self.units = int(np.asarray(weights["recurrent_kernel"]).shape[0])
        self.classes = int(np.asarray(weights["ff_bias"]).shape[0])
        self.attention = weights.get("scale") is not None
        self.vecsize, self.batch_size = int(vecsize), int(batch_size)
        flat = flatten_weights(weights)
        count = L.dgrp_train_param_count(self.units, self.classes, int(self.attention))
        if count != flat.size:
            raise ValueError(f"{flat.size} parameters in the tensors, {count} for units={self.units}, classes={self.classes}")
        self.params = torch.from_numpy(flat).cuda()
        self.grads = torch.zeros_like(self.params)
        self.state1 = torch.zeros_like(self.params)
        self.state2 = torch.zeros_like(self.params)
        self.steps = 0
        self._work = None
        self._work_batch = 0

    def _workspace(self, batch: int):
        if self._work is None or batch > self._work_batch:
            nbytes = self._lib.lib().dgrp_train_workspace_bytes(self.vecsize, self.units, self.classes, int(self.attention), batch)
            if nbytes <= 0:
                self._lib.check(-1, "dgrp_train_workspace_bytes")
            self._work = self._torch.empty(nbytes, dtype=self._torch.uint8, device="cuda")
            self._work_batch = batch
        return self._work

    def job(self, record: DeviceRecord, starts, masks=None, loss_out=None, with_grads: bool = True):
        """The arguments of one training step as a ``_lib.TrainJob`` (struct dgrp_train_job), with the loss tensor and the tensors
        the job points to, which the caller keeps until the step is enqueued.  `starts`: int64 array or device tensor; `masks`:
        [B, 2, 5] float32 or None."""
        torch = self._torch
        if record.classes != self.classes:
            raise ValueError(f"truth of {record.classes} classes for a model of {self.classes}")
        if not torch.is_tensor(starts):
            # the device entry clamps a start into [0, n - T]; host arrays are checked here so that a sampler bug is an error
            starts = np.ascontiguousarray(starts, np.int64)
            if starts.ndim != 1 or starts.size < 1 or starts.min() < 0 or starts.max() > record.n - self.vecsize:
                raise ValueError(f"start positions outside [0, {record.n - self.vecsize}] (record of {record.n} bases, "
                                 f"windows of {self.vecsize})")
        d_starts = starts if torch.is_tensor(starts) else torch.from_numpy(starts).cuda()
        d_masks = None
        if masks is not None:
            d_masks = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks, np.float32)).cuda()
            if tuple(d_masks.shape) != (d_starts.numel(), 2, 5):
                raise ValueError(f"masks of shape {tuple(d_masks.shape)}, ({d_starts.numel()}, 2, 5) expected")
        batch = int(d_starts.numel())
        work = self._workspace(batch)
        loss = torch.empty(1, dtype=torch.float32, device="cuda") if loss_out is None else loss_out
        job = self._lib.TrainJob(
            self.vecsize, self.units, self.classes, int(self.attention), self.params.data_ptr(), record.d_idx.data_ptr(),
            record.d_truth.data_ptr(), record.n, d_starts.data_ptr(), batch, d_masks.data_ptr() if d_masks is not None else None,
            loss.data_ptr(), self.grads.data_ptr() if with_grads else None, work.data_ptr(), work.numel())
        return job, loss, (d_starts, d_masks, work)

    def run(self, record: DeviceRecord, starts, masks=None, loss_out=None, with_grads: bool = True):
        """One dgrp_train_step on the current stream: the loss (a device scalar, `loss_out` if given) and, with `with_grads`,
        the gradients in ``self.grads``.  Arguments as job()."""
        j, loss, _keep = self.job(record, starts, masks, loss_out, with_grads)
        rc = self._lib.lib().dgrp_train_step(
            j.T, j.u, j.C, j.attention, j.d_params, j.d_idx, j.d_truth, j.n, j.d_starts, j.B, j.d_masks, j.d_loss, j.d_grads,
            j.d_work, j.work_bytes, self._torch.cuda.current_stream().cuda_stream)
        self._lib.check(rc, "dgrp_train_step")
        return loss

    def apply(self, optimizer: str, learning_rate: float, rho: float, momentum: float, epsilon: float) -> None:
        """One optimizer step with the gradients of the last run()."""
        self.steps += 1
        rc = self._lib.lib().dgrp_optimizer_step(
            OPTIMIZERS[optimizer.lower()], self.params.data_ptr(), self.grads.data_ptr(), self.state1.data_ptr(),
            self.state2.data_ptr(), self.params.numel(), float(learning_rate), float(rho), float(momentum), float(epsilon),
            self.steps, self._torch.cuda.current_stream().cuda_stream)
        self._lib.check(rc, "dgrp_optimizer_step")

    def weights(self) -> Dict[str, Any]:
        return unflatten_weights(self.params.cpu().numpy(), self.units, self.classes, self.attention)


def run_jobs(jobs) -> None:
    """One dgrp_train_step_multi per slice of DGRP_TRAIN_MAX_JOBS of `jobs` (the (job, loss, kept tensors) of DeviceTrainer.job),
    on the current stream."""
    import torch
    from . import _lib
    stream = torch.cuda.current_stream().cuda_stream
    for first in range(0, len(jobs), _lib.TRAIN_MAX_JOBS):
        part = [j[0] for j in jobs[first:first + _lib.TRAIN_MAX_JOBS]]
        table = (_lib.TrainJob * len(part))(*part)
        _lib.check(_lib.lib().dgrp_train_step_multi(table, len(part), stream), "dgrp_train_step_multi")


# ------------------------------------------------------------------------------------------------ loop
class _Run:
    """One model of training_multi: its generator, samplers, trainer, history file and early-stopping state."""

    def __init__(self, data, options: Options, weights: Dict[str, Any], logdir, seed, classes: int):
        import torch
        self.options, self.logdir = options, logdir
        os.makedirs(logdir, exist_ok=True)
        self.rng = np.random.default_rng(seed)
        self.batches = fetch_batch(options, data[0], self.rng)()
        self.val_batches = fetch_batch(options, data[1], self.rng)()
        self.trainer = DeviceTrainer(weights, options.vecsize, options.batch_size)
        self.config = keras_config(options.vecsize, options.units, classes, bool(options.attention), float(options.dropout))
        self.losses = torch.empty(max(1, int(options.n_batches)) + 1, dtype=torch.float32, device="cuda")
        self.best, self.best_weights, self.wait = float("inf"), self.trainer.weights(), 0
        self.history: List[Tuple[int, float, float]] = []
        self.hist = open(os.path.join(logdir, "history.tsv"), "w")
        self.hist.write("epoch\tloss\tval_loss\n")

    def step_job(self, record: DeviceRecord, i: int):
        o = self.options
        return self.trainer.job(record, next(self.batches), dropout_masks(self.rng, o.batch_size, float(o.dropout)),
                                loss_out=self.losses[i:i + 1])

    def apply(self) -> None:
        o = self.options
        self.trainer.apply(o.optimizer, o.learning_rate, o.rho, o.momentum, o.epsilon)

    def validation_job(self, record: DeviceRecord):
        return self.trainer.job(record, next(self.val_batches), None, loss_out=self.losses[-1:], with_grads=False)

    def end_epoch(self, epoch: int, log: Callable[[str], None]) -> bool:
        """Writes the epoch's line and, on an improvement, the model file; False when the run is over."""
        o = self.options
        host = self.losses.cpu().numpy().astype(np.float64)
        loss, val_loss = float(host[:int(o.n_batches)].mean()), float(host[-1])
        self.history.append((epoch, loss, val_loss))
        line = f"{epoch}\t{loss:.9g}\t{val_loss:.9g}"
        self.hist.write(line + "\n")
        self.hist.flush()
        log(f"epoch {line}")
        if val_loss < self.best:
            self.best, self.wait, self.best_weights = val_loss, 0, self.trainer.weights()
            w = self.best_weights
            save_keras_hdf5(os.path.join(self.logdir, f"{epoch:02d}.hdf5"), w["kernel"], w["recurrent_kernel"], w["bias"],
                            w["ff_kernel"], w["ff_bias"], w["scale"], vecsize=int(o.vecsize), config=self.config)
            return True
        self.wait += 1
        return self.wait < int(o.early_stopping_th)

    def close(self) -> Dict[str, Any]:
        self.hist.close()
        self.trainer = None                                               # the device buffers go back to the allocator
        self.best_weights["history"] = self.history
        return self.best_weights


def training_multi(data: Tuple[preprocessing.Data, preprocessing.Data], options_list, weights_list, logdirs, seeds,
                   log: Optional[Callable[[str], None]] = None) -> List[Dict[str, Any]]:
    """Trains ``len(options_list)`` models side by side on the same data: per step ONE dgrp_train_step_multi over the models still
    running (slices of DGRP_TRAIN_MAX_JOBS), then their optimizer steps; per epoch one loss-only multi step over their validation
    batches.  A model has its own units, vecsize, attention, batch_size, optimizer and hyper-parameters, its own generator
    ``default_rng(seeds[k])``, sampler, dropout masks, early stopping, ``history.tsv`` and model files in ``logdirs[k]``; only
    `n_batches` and `n_epochs` must agree.  A model that stops early leaves the step and the others go on.  The two records are
    uploaded once.  Element k of the result, and the files in logdirs[k], are byte for byte those of
    ``training(data, options_list[k], weights_list[k], logdirs[k], seed=seeds[k])``: a job's bytes do not depend on its cohort."""
    count = len(options_list)
    if not (len(weights_list) == len(logdirs) == len(seeds) == count) or count < 1:
        raise ValueError("training_multi: options, weights, logdirs and seeds must be lists of one length, at least 1")
    for options in options_list:
        check_options(options)
    for name in ("n_batches", "n_epochs"):
        values = [int(getattr(o, name)) for o in options_list]
        if len(set(values)) > 1:
            raise TrainingRefused(f"{name} = {values}: models trained side by side take the same {name}")
    for options in options_list:
        classes = len(options.repeats_to_search) + 1
        for d in data:
            if d.truelbl.shape[0] != classes:
                raise ValueError(f"truth of {d.truelbl.shape[0]} rows, {classes} expected from repeats_to_search")
    say = log or _LOG.info
    records = [DeviceRecord.from_data(d) for d in data]
    runs: List[Optional[_Run]] = [None] * count
    results: List[Optional[Dict[str, Any]]] = [None] * count
    try:
        for k in range(count):
            runs[k] = _Run(data, options_list[k], weights_list[k], logdirs[k], seeds[k], records[0].classes)
        active = list(range(count))
        n_batches, n_epochs = int(options_list[0].n_batches), int(options_list[0].n_epochs)
        for epoch in range(1, n_epochs + 1):
            for i in range(n_batches):
                run_jobs([runs[k].step_job(records[0], i) for k in active])
                for k in active:
                    runs[k].apply()
            run_jobs([runs[k].validation_job(records[1]) for k in active])
            still = []
            for k in active:
                if runs[k].end_epoch(epoch, say if count == 1 else (lambda msg, k=k: say(f"model {k}: {msg}"))):
                    still.append(k)
                else:
                    results[k], runs[k] = runs[k].close(), None
            active = still
            if not active:
                break
    finally:
        for k in range(count):
            if runs[k] is not None:
                results[k], runs[k] = runs[k].close(), None
    return results


def training(data: Tuple[preprocessing.Data, preprocessing.Data], options: Options, model_weights: Dict[str, Any], logdir,
             seed: Optional[int] = None, log: Optional[Callable[[str], None]] = None) -> Dict[str, Any]:
    """Runs training (deepgrp/training.py:15-73): `n_epochs` epochs of `n_batches` steps on data[0]; after each epoch the loss of
    one batch of data[1] without dropout.  An epoch whose validation loss improves writes ``<logdir>/<epoch:02d>.hdf5``
    (ModelCheckpoint, save_best_only); `early_stopping_th` epochs without improvement end the run; the best weights are
    returned (restore_best_weights).  ``<logdir>/history.tsv`` gets one line per epoch: epoch, loss (mean of the epoch's steps),
    val_loss.  Returns the best weights as Keras tensors, with ``history`` (list of (epoch, loss, val_loss)).  The one-model call
    of training_multi's loop."""
    return training_multi(data, [options], [model_weights], [logdir], [seed], log)[0]
