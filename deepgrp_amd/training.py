"""deepgrp_amd.training -- mirror of deepgrp/training.py: the class-balanced window sampler, and the training loop on the GPU.

The reference hands a Keras model to ``model.fit``; here the step (forward over a batch of windows, loss, backward through time,
optimizer) is libdeepgrp_hip's ``dgrp_train_step`` / ``dgrp_optimizer_step`` on one flat float32 parameter buffer.  The sampler
returns START POSITIONS into the record instead of copied windows: the record's class indices and its truth stay on the device.

Differences from the reference, all stated in DESIGN.md: no TensorBoard output and no TensorFlow checkpoint bundles (the best epoch
is written as ``<logdir>/<epoch:02d>.hdf5``, a Keras HDF5 file), the GRU cell's dropout mask is constant over the steps of a window,
and ``seed`` makes a run reproducible byte for byte.

A side of the data comes in one of two forms.  ``preprocessing.Data`` is the reference's: host arrays from a one-hot .npz, sampled by
``fetch_batch`` on the host.  ``DeviceData`` is a sequence file (FASTA, gzip, BGZF, .2bit) as the device ingest left it: the kept
records back to back in HBM, the multi-hot truth painted there from the annotation rows, the sampler's class index sets built there
(``DeviceSampler``); the host draws ranks from the generator in ``fetch_batch``'s order and the device turns them into starts.
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


# ------------------------------------------------------------------------------------------------ sequence files
SEGMENT_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])     # struct dgrp_segment


def is_npz(path) -> bool:
    """The file starts with a zip signature: what ``np.savez`` / ``preprocess_sequence`` write (False if it cannot be opened)."""
    try:
        with open(path, "rb") as fh:
            return fh.read(4) in (b"PK\x03\x04", b"PK\x05\x06")
    except OSError:
        return False


def first_word(header: str) -> str:
    """The name a record is matched by: the first whitespace-delimited word of its header (evaluation.record_name's rule)."""
    words = header.split()
    return words[0] if words else ""


def _header_lines(buf, line_start: bool):
    """(complete header lines of `buf` without their '>', offset of a header line still open at the end or -1): a header line opens
    with '>' at a line start, which `buf` begins with when `line_start`."""
    out = []
    if line_start and buf[:1] == b">":
        i = 0
    else:
        j = buf.find(b"\n>")
        i = j + 1 if j >= 0 else -1
    while i >= 0:
        nl = buf.find(b"\n", i)
        if nl < 0:
            return out, i
        out.append(buf[i + 1:nl])
        j = buf.find(b"\n>", nl)
        i = j + 1 if j >= 0 else -1
    return out, -1


def sequence_names(path) -> List[str]:
    """First words of the record headers of a sequence file in file order, read on the HOST (no device, no library): FASTA text by a
    scan for '>' at line starts, gzip / BGZF through zlib, .2bit from its index.  Records without a header are left out, as the
    ingest leaves them out.  `train` checks --train_contigs / --valid_contigs against this before any device work."""
    import mmap
    import zlib

    from . import gz, twobit
    heads: List[bytes] = []
    if twobit.is_twobit(path):
        heads = [b" ".join(nm.split(b"\n")[0].split()) for nm in twobit.open_twobit(path).names]
    elif gz.is_gzip(path):
        carry, line_start = b"", True
        with open(path, "rb") as fh:
            d = zlib.decompressobj(31)
            while True:
                data = fh.read(1 << 22)
                if not data:
                    break
                while data:
                    if d.eof:                                            # the next member
                        d = zlib.decompressobj(31)
                    try:
                        buf = carry + d.decompress(data)
                    except zlib.error as exc:
                        raise gz.GzipError(path, fh.tell() - len(data), str(exc)) from None
                    data = d.unused_data
                    if not buf:
                        continue
                    got, still = _header_lines(buf, line_start)
                    heads += got
                    carry = buf[still:] if still >= 0 else b""
                    line_start = True if still >= 0 else buf.endswith(b"\n")
        if carry:
            heads.append(carry[1:])
    elif os.path.getsize(path):
        with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            heads, still = _header_lines(mm, True)
            if still >= 0:
                heads.append(mm[still + 1:])
    names = [first_word(h.decode("utf-8", "surrogateescape").strip()) for h in heads if h.strip()]
    return names


def select_contigs(names: List[str], contigs: Optional[List[str]], what: str) -> List[str]:
    """The names of `names` (file order) that `contigs` selects (None: all of them).  ValueError naming a listed contig the file does
    not hold, and a first word that two selected records share."""
    if contigs is not None:
        have = set(names)
        for c in contigs:
            if c not in have:
                raise ValueError(f"{what}: no record named {c!r} (records: {', '.join(repr(n) for n in names[:5]) or 'none'}"
                                 f"{', ...' if len(names) > 5 else ''})")
        wanted = set(contigs)
        names = [n for n in names if n in wanted]
    seen = set()
    for n in names:
        if n in seen:
            raise ValueError(f"{what}: two records are named {n!r}: the annotation rows of {n!r} cannot be told apart")
        seen.add(n)
    return names


def read_truth_rows(bedfile, names: List[str], repeats_to_search) -> Dict[str, np.ndarray]:
    """The rows preprocess_y keeps for each contig of `names`, as SEGMENT_DTYPE arrays in file order: first column the contig, repeat
    number (fourth column) in `repeats_to_search`.  A kept number that has no truth row -- the reference's IndexError -- is a
    ValueError naming the line, as is a negative coordinate; a row that ends at or before its begin paints nothing and is dropped."""
    classes = len(repeats_to_search) + 1
    wanted = set(int(r) for r in repeats_to_search)
    per: Dict[str, List[Tuple[int, int, int]]] = {n: [] for n in names}
    with open(bedfile, "r") as fh:
        for lineno, line in enumerate(fh, 1):
            cols = line.split()
            if not cols or cols[0] not in per:
                continue
            number = int(cols[3])
            if number not in wanted:
                continue
            begin, end = int(cols[1]), int(cols[2])
            if not 1 <= number < classes:
                raise ValueError(f"{bedfile}:{lineno}: repeat number {number} has no row in a truth of {classes} classes "
                                 f"(repeats_to_search = {list(repeats_to_search)}): {line.rstrip()!r}")
            if begin < 0 or end < 0:
                raise ValueError(f"{bedfile}:{lineno}: negative coordinate: {line.rstrip()!r}")
            if end > begin:
                per[cols[0]].append((begin, end, number))
    out = {}
    for n, rows in per.items():
        arr = np.zeros(len(rows), SEGMENT_DTYPE)
        if rows:
            arr["start"], arr["end"], arr["label"] = np.asarray(rows, np.int64).T
        out[n] = arr
    return out


class DeviceData:
    """One side of the training data, resident: the class indices uint8 [n] of its records back to back, their multi-hot truth int8
    [classes, n], and the record table (`names`, `base` = position of each record in the buffer, `lengths`, `startpos` = original
    coordinate of each record's first base).  A record's bases are those from its first to its last non-N base without the last one
    (drop_start_end_n's span).  DeviceTrainer.job takes it where it takes a DeviceRecord."""

    def __init__(self, d_idx, d_truth, names, base, lengths, startpos):
        self.d_idx, self.d_truth = d_idx, d_truth
        self.n, self.classes = int(d_idx.numel()), int(d_truth.shape[0])
        self.names = list(names)
        self.base, self.lengths, self.startpos = (np.ascontiguousarray(a, np.int64) for a in (base, lengths, startpos))

    @classmethod
    def from_data(cls, data: preprocessing.Data) -> "DeviceData":
        """The host arrays of a .npz side, uploaded: one record."""
        rec = DeviceRecord.from_data(data)
        return cls(rec.d_idx, rec.d_truth, [None], [0], [rec.n], [0])

    @classmethod
    def from_sequence_file(cls, path, bedfile, repeats_to_search, contigs: Optional[List[str]] = None,
                           vecsize: Optional[int] = None) -> "DeviceData":
        """The records of a FASTA / gzip / BGZF / .2bit file that `contigs` names by the first word of their header (None: every
        record), in file order, and their truth from the parse_rm table `bedfile` (or the annotation.Listing of a RepeatMasker listing),
        painted on the device.  With `vecsize`, a record
        that holds no window of that length is left out with a warning.  ValueError: a listed contig the file does not hold, two
        selected records with one name, a kept annotation row whose repeat number has no truth row, no record left."""
        import torch

        from . import _lib
        from .fasta import read_multi_fasta_device
        from .pipeline import record_indices, stream_ptr
        wanted = None if contigs is None else set(contigs)
        found, names, parts, lengths, startpos = [], [], [], [], []
        for header, rec in read_multi_fasta_device(path):
            name = first_word(header)
            found.append(name)
            if wanted is not None and name not in wanted:
                continue
            try:
                st, d_idx = record_indices(rec)
            except ValueError:                                           # a record of N only
                st, d_idx = 0, None
            n = max(int(d_idx.numel()) - 1, 0) if d_idx is not None else 0
            if n - (int(vecsize) if vecsize is not None else 0) < 1:
                _LOG.warning("%s: record %r keeps %d bases: no window%s fits, it is left out", path, name, n,
                             f" of {vecsize}" if vecsize is not None else "")
                continue
            names.append(name)
            parts.append(d_idx[:n])
            lengths.append(n)
            startpos.append(int(st))
        select_contigs(found, contigs, str(path))                        # names the absent and the duplicated
        if not parts:
            raise ValueError(f"{path}: no window of {vecsize if vecsize is not None else 1} fits into a selected record")
        # (a RepeatMasker listing comes parsed, as an annotation.Listing: read_truth_rows' rules on its arrays)
        rows = (bedfile.truth_rows(names, repeats_to_search) if hasattr(bedfile, "truth_rows")
                else read_truth_rows(bedfile, names, repeats_to_search))
        classes = len(repeats_to_search) + 1
        d_idx = torch.cat(parts)
        del parts
        ln = np.asarray(lengths, np.int64)
        base = np.zeros(len(ln) + 1, np.int64)
        np.cumsum(ln, out=base[1:])
        n_total = int(base[-1])
        org = np.asarray(startpos, np.int64)
        row_off = np.zeros(len(ln) + 1, np.int64)
        np.cumsum([len(rows[nm]) for nm in names], out=row_off[1:])
        flat = np.concatenate([rows[nm] for nm in names])
        dev = d_idx.device
        d_rows = torch.from_numpy(flat.view(np.uint8)).to(dev) if flat.size else None
        d_truth = torch.empty((classes, n_total), dtype=torch.int8, device=dev)
        L = _lib.lib()
        wb = L.dgrp_truth_workspace_bytes(len(ln), int(row_off[-1]))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dgrp_truth_multihot_batch(d_truth.data_ptr(), classes, n_total, len(ln), base.ctypes.data, ln.ctypes.data,
                                               org.ctypes.data, d_rows.data_ptr() if d_rows is not None else None,
                                               row_off.ctypes.data, work.data_ptr(), wb, stream_ptr()), "dgrp_truth_multihot_batch")
        return cls(d_idx, d_truth, names, base[:-1], ln, org)


def draw_picks(rng: np.random.Generator, sizes: List[int], windows: int, batch_size: int, one_class_size: int) -> np.ndarray:
    """One batch of fetch_batch as (set, rank) pairs, int64 [batch_size, 2], drawn from `rng` exactly as fetch_batch draws: for every
    set (of `sizes[i]` starts, each larger than `one_class_size`) ``integers(0, size, one_class_size)`` -- what
    ``choice(indices, one_class_size)`` draws --, then ``integers(0, windows, rest)`` with set -1 for the uniform part, then one
    ``shuffle`` of the batch's order (a shuffle depends on the length alone)."""
    picks = np.empty((batch_size, 2), np.int64)
    q, filled = one_class_size, one_class_size * len(sizes)
    for i, size in enumerate(sizes):
        picks[q * i:q * (i + 1), 0] = i
        picks[q * i:q * (i + 1), 1] = rng.integers(0, size, q)
    picks[filled:, 0] = -1
    picks[filled:, 1] = rng.integers(0, windows, size=batch_size - filled)
    order = np.arange(batch_size)
    rng.shuffle(order)
    return picks[order]


class DeviceSampler:
    """fetch_batch on a DeviceData: the same draws from `rng` in the same order -- per class whose index set is larger than
    ``one_class_size`` that many RANKS into the set, then the uniform rest as ranks into the windows of all records, then one
    shuffle -- and the device resolves (set, rank) to start positions (dgrp_train_resolve_starts).  The sets are built on the device
    for this sampler's `vecsize` (dgrp_class_window_starts) and stay there; only their sizes come back.  For one record the starts
    are fetch_batch's, batch for batch."""

    def __init__(self, options: Options, data: DeviceData, rng: Optional[np.random.Generator] = None):
        import torch

        from . import _lib
        from .pipeline import stream_ptr
        self._torch, self._lib, self._stream = torch, _lib, stream_ptr
        self.rng = np.random.default_rng() if rng is None else rng
        self.data = data
        T, classes = int(options.vecsize), data.classes
        self.batch_size = int(options.batch_size)
        self.one_class_size = int(options.batch_size * options.repeat_probability / (classes - 1))
        windows = np.maximum(data.lengths - T, 0)
        wprefix = np.zeros(len(windows) + 1, np.int64)
        np.cumsum(windows, out=wprefix[1:])
        self.windows = int(wprefix[-1])
        if self.windows < 1:
            raise ValueError(f"the record{'s have' if len(windows) > 1 else ' has'} {', '.join(str(int(x)) for x in data.lengths)} "
                             f"bases: no window of {T} fits")
        L, dev = _lib.lib(), data.d_idx.device
        nrec = len(data.lengths)
        wb = L.dgrp_class_starts_workspace_bytes(nrec, data.n)
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        count = C.c_int64(0)

        def starts_of(c: int, d_out, cap: int) -> int:
            _lib.check(L.dgrp_class_window_starts(data.d_truth[c].data_ptr(), data.n, nrec, data.base.ctypes.data,
                                                  data.lengths.ctypes.data, T, d_out.data_ptr() if d_out is not None else None, cap,
                                                  C.byref(count), work.data_ptr(), wb, stream_ptr()), "dgrp_class_window_starts")
            return int(count.value)

        self.sets, self.sizes = [], []
        for c in range(1, classes):
            size = starts_of(c, None, 0)
            if size > self.one_class_size:                               # (fetch_batch leaves a class with fewer indices out)
                d_set = torch.empty(size, dtype=torch.int64, device=dev)
                starts_of(c, d_set, size)
                self.sets.append(d_set)
                self.sizes.append(size)
        table = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)
        self._set_ptr = table([t.data_ptr() for t in self.sets] or [0])
        self._set_size = table(self.sizes or [0])
        self._base, self._wprefix = table(data.base), table(wprefix)

    def batches(self) -> Iterator[Any]:
        """Device tensors int64 [batch_size] of start positions into the side's buffer, one per batch, without end."""
        torch, L = self._torch, self._lib.lib()
        B = self.batch_size
        while True:
            picks = draw_picks(self.rng, self.sizes, self.windows, B, self.one_class_size)
            d_picks = torch.from_numpy(picks).to(self._base.device)
            d_starts = torch.empty(B, dtype=torch.int64, device=self._base.device)
            self._lib.check(L.dgrp_train_resolve_starts(d_picks.data_ptr(), B, self._set_ptr.data_ptr(), self._set_size.data_ptr(),
                                                        len(self.sets), self._base.data_ptr(), self._wprefix.data_ptr(),
                                                        len(self.data.lengths), d_starts.data_ptr(), self._stream()),
                            "dgrp_train_resolve_starts")
            yield d_starts


def _batches(options: Options, data, rng: np.random.Generator):
    """The batch iterator of one side: fetch_batch on the host for a preprocessing.Data, the rank sampler for a DeviceData."""
    if isinstance(data, DeviceData):
        return DeviceSampler(options, data, rng).batches()
    return fetch_batch(options, data, rng)()


# ------------------------------------------------------------------------------------------------ loop
class _Run:
    """One model of training_multi: its generator, samplers, trainer, history file and early-stopping state."""

    def __init__(self, data, options: Options, weights: Dict[str, Any], logdir, seed, classes: int):
        import torch
        self.options, self.logdir = options, logdir
        os.makedirs(logdir, exist_ok=True)
        self.rng = np.random.default_rng(seed)
        self.batches = _batches(options, data[0], self.rng)
        self.val_batches = _batches(options, data[1], self.rng)
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


def training_multi(data: Tuple[Any, Any], options_list, weights_list, logdirs, seeds,
                   log: Optional[Callable[[str], None]] = None) -> List[Dict[str, Any]]:
    """Trains ``len(options_list)`` models side by side on the same data: per step ONE dgrp_train_step_multi over the models still
    running (slices of DGRP_TRAIN_MAX_JOBS), then their optimizer steps; per epoch one loss-only multi step over their validation
    batches.  A model has its own units, vecsize, attention, batch_size, optimizer and hyper-parameters, its own generator
    ``default_rng(seeds[k])``, sampler, dropout masks, early stopping, ``history.tsv`` and model files in ``logdirs[k]``; only
    `n_batches` and `n_epochs` must agree.  A model that stops early leaves the step and the others go on.  Each side of `data` is a
    preprocessing.Data (uploaded once, sampled by fetch_batch on the host) or a DeviceData (resident; every model builds the index
    sets of its own vecsize on the device).  Element k of the result, and the files in logdirs[k], are byte for byte those of
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
            rows = d.classes if isinstance(d, DeviceData) else d.truelbl.shape[0]
            if rows != classes:
                raise ValueError(f"truth of {rows} rows, {classes} expected from repeats_to_search")
    say = log or _LOG.info
    records = [d if isinstance(d, DeviceData) else DeviceRecord.from_data(d) for d in data]
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


def training(data: Tuple[Any, Any], options: Options, model_weights: Dict[str, Any], logdir,
             seed: Optional[int] = None, log: Optional[Callable[[str], None]] = None) -> Dict[str, Any]:
    """Runs training (deepgrp/training.py:15-73): `n_epochs` epochs of `n_batches` steps on data[0]; after each epoch the loss of
    one batch of data[1] without dropout.  An epoch whose validation loss improves writes ``<logdir>/<epoch:02d>.hdf5``
    (ModelCheckpoint, save_best_only); `early_stopping_th` epochs without improvement end the run; the best weights are
    returned (restore_best_weights).  ``<logdir>/history.tsv`` gets one line per epoch: epoch, loss (mean of the epoch's steps),
    val_loss.  Returns the best weights as Keras tensors, with ``history`` (list of (epoch, loss, val_loss)).  The one-model call
    of training_multi's loop."""
    return training_multi(data, [options], [model_weights], [logdir], [seed], log)[0]
