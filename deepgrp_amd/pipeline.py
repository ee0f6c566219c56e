"""Device pipeline for one FASTA record: everything between the sequence bytes and
the segment records stays in HBM.

    bytes --encode--> class idx --GRU/attention + softmax + max-merge--> probs [N,C]
          --scores--> (score f64, class i8) --MSS + vote--> labels i8 --RLE--> records

This is what ``deepgrp predict`` (deepgrp/__main__.py:46-83, :280-292 of the
reference) computes per record; `deepgrp_amd.prediction` / `.sequence` / `.mss`
expose the individual reference functions on top of the same kernels.
PyTorch is used only to own device memory and the stream.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._lib import check, lib, name_blob
from .fasta import DeviceRecord

SEGMENT_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
# struct dgrp_row_score (predict --bed_dir): exact integer statistics of a row's label column over its clipped span
ROW_SCORE_DTYPE = np.dtype([("sum", "<u8"), ("bases", "<i8"), ("agree", "<i8"), ("qmin", "<u4"), ("pad", "<u4")])


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("deepgrp_amd needs an AMD MI355X (gfx950) visible to PyTorch-ROCm; "
                           "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


# DGRP_KERNEL_* (include/deepgrp_hip.h) by value
KERNEL_NAMES = ("none", "wave", "split2", "stream64", "stream", "split", "lstm", "fused", "fp32")


class KernelPlan(NamedTuple):
    """DeviceModel.plan: kernel name (KERNEL_NAMES), dynamic LDS bytes, rows of the merged-output LDS image (0: none), avg[t] row length."""
    kernel: str
    lds: int
    ospan: int
    avg_up: int


class DeviceModel:
    """The tensors ``tf.keras.models.load_model`` yields, packed into MFMA
    fragments in HBM by ``dgrp_model_create``.  Mirrors the two Keras attributes the
    reference reads: ``input_shape`` (__main__.py:270) and ``output_shape`` (:75)."""

    def __init__(self, kernel, recurrent_kernel, bias, ff_kernel, ff_bias, scale=None, vecsize: int = 200,
                 rnn: str = "GRU"):
        require_gpu()
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.kernel, self.recurrent_kernel, self.bias = f32(kernel), f32(recurrent_kernel), f32(bias)
        self.ff_kernel, self.ff_bias = f32(ff_kernel), f32(ff_bias)
        self.scale = None if scale is None else f32(scale).reshape(-1)
        self.units = int(self.recurrent_kernel.shape[0])
        self.classes = int(self.ff_bias.shape[0])
        self.vecsize = int(vecsize)
        self.attention = self.scale is not None
        self.rnn = rnn
        u, c = self.units, self.classes
        h = C.c_void_p()
        if rnn == "LSTM":
            # deepgrp/model.py:219-223: Keras LSTM, gate columns i|f|c|o, one bias vector, never with attention
            self.bias = self.bias.reshape(-1)
            if self.kernel.shape != (5, 4 * u) or self.recurrent_kernel.shape != (u, 4 * u) or self.bias.shape != (4 * u,):
                raise ValueError(f"LSTM tensors have unexpected shapes {self.kernel.shape} {self.recurrent_kernel.shape} {self.bias.shape}")
            if self.attention or self.ff_kernel.shape != (u, c):
                raise ValueError("the LSTM model has no attention and a [units, classes] FF kernel")
            check(lib().dgrp_model_create_lstm(C.byref(h), self.vecsize, u, c, _np_ptr(self.kernel),
                                               _np_ptr(self.recurrent_kernel), _np_ptr(self.bias), _np_ptr(self.ff_kernel),
                                               _np_ptr(self.ff_bias)), "dgrp_model_create_lstm")
            self.handle = h
            self._warn_fp32_path()
            return
        if rnn != "GRU":
            raise ValueError(f"unknown rnn {rnn!r}")
        if self.kernel.shape != (5, 3 * u) or self.recurrent_kernel.shape != (u, 3 * u) or self.bias.shape != (2, 3 * u):
            raise ValueError(f"GRU tensors have unexpected shapes {self.kernel.shape} {self.recurrent_kernel.shape} "
                             f"{self.bias.shape}; expected reset_after GRU with 5 inputs")
        if self.ff_kernel.shape != ((2 if self.attention else 1) * u, c):
            raise ValueError(f"FF kernel shape {self.ff_kernel.shape} does not match units={u}, attention={self.attention}")
        if self.attention and self.scale.shape != (u,):
            raise ValueError("attention scale must have `units` entries")
        check(lib().dgrp_model_create(C.byref(h), self.vecsize, u, c, int(self.attention), _np_ptr(self.kernel),
                                      _np_ptr(self.recurrent_kernel), _np_ptr(self.bias),
                                      _np_ptr(self.scale) if self.attention else None, _np_ptr(self.ff_kernel),
                                      _np_ptr(self.ff_bias)), "dgrp_model_create")
        self.handle = h
        self._warn_fp32_path()

    def _warn_fp32_path(self) -> None:
        """More units than any fused kernel takes: the model runs, on the plain-fp32 kernels (the reference takes any `units`,
        deepgrp/model.py:117,219-229) -- said once, loudly, because it is 10-20x slower than a model of 256 units."""
        self.fp32_only = bool(lib().dgrp_model_flags(self.handle) & 4)
        if self.fp32_only:
            import warnings
            what = f"{self.units} units" if self.units > 256 else f"{self.classes} classes"
            warnings.warn(f"{self.rnn} with {what} is beyond the fused kernels (256 units, 16 classes): every forward pass runs on the "
                          f"plain-fp32 kernels, tens of Mbp/s", RuntimeWarning, stacklevel=3)

    input_shape = property(lambda self: (None, self.vecsize, 5))
    output_shape = property(lambda self: (None, self.vecsize, self.classes))

    # ---- the Keras model surface the reference touches besides predict_on_batch --------------------------------
    def get_config(self) -> dict:
        """``keras.Model.get_config()`` (tests/test_model.py:254-262 of the reference)."""
        from . import model as dgmodel
        if getattr(self, "config", None) is None:
            self.config = dgmodel.keras_config(self.vecsize, self.units, self.classes, self.attention, rnn=self.rnn)
        return self.config["config"]

    def get_weights(self):
        """Tensors in Keras' order: RNN kernel, recurrent kernel, bias, [attention scale], FF kernel, FF bias."""
        scale = [] if self.scale is None else [self.scale.copy()]
        return [self.kernel.copy(), self.recurrent_kernel.copy(), self.bias.copy()] + scale + [self.ff_kernel.copy(), self.ff_bias.copy()]

    def save(self, path: str) -> None:
        """``model.save("*.hdf5")`` (deepgrp/__main__.py:351): the Keras HDF5 layout ``load_model`` reads back."""
        from . import model as dgmodel
        self.get_config()
        dgmodel.save_keras_hdf5(path, self.kernel, self.recurrent_kernel, self.bias, self.ff_kernel, self.ff_bias, self.scale,
                                vecsize=self.vecsize, rnn=self.rnn, config=self.config)

    @property
    def kernel_flags(self) -> int:
        """dgrp_model_flags: bit 0 = the one-reciprocal GRU blend was provably safe for these weights, bit 1 = the
        split-operand kernel is selected."""
        return int(lib().dgrp_model_flags(self.handle))

    @property
    def supports_split(self) -> bool:
        """A split-operand fused kernel (fp16 hi+lo pairs, fp32-grade pre-activations) covers this model (with attention: its
        recurrent pre-pass) -- every model: GRU up to 128 units has the resident-weight kernels, larger GRUs and the LSTM cell
        the streamed one (rnn_stream.hip)."""
        return True

    def set_precision(self, level: int) -> None:
        """dgrp_model_set_precision: 0 = fp16 operands (`--fast`), 1 = split operands (the default of every model), for every later
        call on THIS handle.  Pipelines do not call it: each holds a view of its own (`view`)."""
        check(lib().dgrp_model_set_precision(self.handle, int(level)), "dgrp_model_set_precision")

    def view(self, level: int) -> C.c_void_p:
        """dgrp_model_view: a second handle on the same device buffers with its own precision level (release: dgrp_model_destroy)."""
        v = C.c_void_p()
        check(lib().dgrp_model_view(self.handle, int(level), C.byref(v)), "dgrp_model_view")
        return v

    def plan(self, mode: int, step: int, handle=None) -> "KernelPlan":
        """dgrp_model_plan: the recurrent kernel a launch of `mode` (0 merged, 1 window probabilities, 2 attention pre-pass) with
        step `step` would run on this handle (or on `handle`, a view) at its current precision level, and its LDS carve."""
        k, lds, ospan, avg_up = C.c_int(), C.c_int64(), C.c_int(), C.c_int()
        check(lib().dgrp_model_plan(handle if handle is not None else self.handle, int(mode), int(step), C.byref(k), C.byref(lds),
                                    C.byref(ospan), C.byref(avg_up)), "dgrp_model_plan")
        return KernelPlan(KERNEL_NAMES[k.value], lds.value, ospan.value, avg_up.value)

    def close(self):
        if getattr(self, "handle", None):
            lib().dgrp_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- model.predict_on_batch (prediction.py:106) ---------------------------------------
    def forward_windows(self, d_idx: torch.Tensor, step: int, w0: int, nw: int, handle=None) -> torch.Tensor:
        """probs [nw, T, C] (device) of windows w0.. of a class-index tensor; `handle`: a view of this model with a precision
        level of its own (ContigPipeline.handle) instead of the model's."""
        h = handle if handle is not None else self.handle
        probs = torch.empty((nw, self.vecsize, self.classes), dtype=torch.float32, device=d_idx.device)
        wb = lib().dgrp_forward_workspace_bytes(h, nw)
        work = torch.empty(max(wb, 256), dtype=torch.uint8, device=d_idx.device)
        check(lib().dgrp_forward_windows(h, _ptr(d_idx), d_idx.numel(), step, w0, nw, _ptr(probs),
                                         _ptr(work), work.numel(), stream_ptr()), "dgrp_forward_windows")
        return probs

    def forward_windows_reference(self, d_idx: torch.Tensor, step: int, w0: int, nw: int) -> torch.Tensor:
        """The same windows through the plain-fp32 evaluation of the model on the device (dgrp_forward_windows_reference):
        the yardstick the fused fp16-operand kernel is measured against.  Slow; hundreds of windows."""
        probs = torch.empty((nw, self.vecsize, self.classes), dtype=torch.float32, device=d_idx.device)
        wb = lib().dgrp_forward_reference_workspace_bytes(self.handle, nw)
        work = torch.empty(max(wb, 256), dtype=torch.uint8, device=d_idx.device)
        check(lib().dgrp_forward_windows_reference(self.handle, _ptr(d_idx), d_idx.numel(), step, w0, nw, _ptr(probs),
                                                   _ptr(work), work.numel(), stream_ptr()), "dgrp_forward_windows_reference")
        return probs

    def check_accuracy(self, d_idx: Optional[torch.Tensor] = None, step: int = 50, windows: int = 256, seed: int = 0,
                       level: Optional[int] = None) -> dict:
        """Largest deviation of the fused kernel's class probabilities from the fp32 yardstick on up to `windows`
        windows spread evenly over the class-index tensor `d_idx` (default: a random ACGT sequence).  The bound the
        path is built to is 1e-3 (BASELINE north star).  `level` picks the fused kernel for the comparison (0 = fp16
        operands, 1 = split operands; default: the model's current setting) and is restored afterwards."""
        if level is not None:
            before = 1 if self.kernel_flags & 2 else 0
            self.set_precision(level)
            try:
                return self.check_accuracy(d_idx, step, windows, seed)
            finally:
                self.set_precision(before)
        dev = require_gpu()
        if d_idx is None:
            rng = np.random.default_rng(seed)
            d_idx = torch.from_numpy(rng.integers(0, 4, size=self.vecsize + step * windows, dtype=np.uint8)).to(dev)
        total = int(lib().dgrp_window_count(d_idx.numel(), self.vecsize, step))
        if total <= 0:
            raise ValueError(f"sequence of {d_idx.numel()} bases holds no window of {self.vecsize}")
        chunk = min(64, total)
        starts = sorted({int(x) for x in np.linspace(0, total - chunk, max(1, min(windows, total) // chunk))})
        worst, worst_window, checked, flips, above = 0.0, -1, 0, 0, 0
        per_window = []
        for w0 in starts:
            fast = self.forward_windows(d_idx, step, w0, chunk)
            ref = self.forward_windows_reference(d_idx, step, w0, chunk)
            dpos = (fast - ref).abs().amax(dim=2)                           # [chunk, T]
            diff = dpos.amax(dim=1)
            per_window.append(diff)
            k = int(diff.argmax())
            if float(diff[k]) > worst:
                worst, worst_window = float(diff[k]), w0 + k
            flips += int((fast.argmax(dim=2) != ref.argmax(dim=2)).sum())
            above += int((dpos > 1e-3).sum())
            checked += chunk
        pw = torch.cat(per_window).double()
        q = torch.quantile(pw, torch.tensor([0.5, 0.99], dtype=torch.float64, device=pw.device)).cpu().numpy()
        return {"max_abs_diff": worst, "window": worst_window, "windows_checked": checked, "argmax_flips": flips,
                "positions_checked": checked * self.vecsize, "positions_above_1e-3": above,
                "median_window_max": float(q[0]), "q99_window_max": float(q[1]),
                "windows_above_1e-3": int((pw > 1e-3).sum()), "within_1e-3": worst <= 1e-3}

    def predict_on_batch(self, batch) -> np.ndarray:
        """Keras-style call on a one-hot batch [b, T, 5]; returns numpy float32 [b, T, C]."""
        dev = require_gpu()
        x = torch.as_tensor(np.asarray(batch) if not isinstance(batch, torch.Tensor) else batch)
        if x.ndim != 3 or x.shape[1] != self.vecsize or x.shape[2] != 5:
            raise ValueError(f"expected a batch of shape [b, {self.vecsize}, 5], got {tuple(x.shape)}")
        x = x.to(dev)
        # the device path looks the input projection up by base (one-hot input): anything else -- soft labels, random
        # floats, an all-zero row -- would silently be read as the argmax base, where Keras computes the real projection
        if x.numel() and not bool((((x == 0) | (x == 1)).all(dim=2) & (x.sum(dim=2) == 1)).all()):
            raise ValueError("predict_on_batch takes one-hot batches (every [b, t, :] row holds a single 1): the device path looks "
                             "the input projection up by base")
        idx = x.argmax(dim=2).to(torch.uint8).reshape(-1).contiguous()
        b = x.shape[0]
        if b == 0:
            return np.zeros((0, self.vecsize, self.classes), np.float32)
        return self.forward_windows(idx, self.vecsize, 0, b).cpu().numpy()


def kept_length(n: int) -> int:
    """The all-N rule: such a record's kept length is negative, and the reference's np.zeros raises on it (sequence.pyx:32)."""
    if n < 0:
        raise ValueError("negative dimensions are not allowed")
    return n


def upload_sequence(raw: bytes) -> Tuple[int, torch.Tensor]:
    """A2 on the device: (startpos, class-index uint8 [N]).  Mirrors
    one_hot_encode_dna_sequence's stripping of leading/trailing 'N' (sequence.pyx:27-30),
    including the ValueError for an all-N record."""
    dev = require_gpu()
    st, kept = C.c_int64(0), C.c_int64(0)
    host = np.frombuffer(raw, dtype=np.uint8)
    check(lib().dgrp_strip_n(_np_ptr(host) if len(raw) else None, len(raw), C.byref(st), C.byref(kept)), "dgrp_strip_n")
    n = kept_length(kept.value)
    d_idx = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        d_seq = torch.from_numpy(host[st.value:st.value + n].copy()).to(dev, non_blocking=False)
        check(lib().dgrp_encode(_ptr(d_seq), n, _ptr(d_idx), stream_ptr()), "dgrp_encode")
    return st.value, d_idx


def record_indices(rec) -> Tuple[int, torch.Tensor]:
    """(startpos, class-index uint8 [N]) of a record in either form: a fasta.DeviceRecord, parsed and encoded on the GPU, or the
    sequence as text (str or bytes), uploaded here.  An all-N record raises in both."""
    if isinstance(rec, DeviceRecord):
        kept_length(rec.length)
        return rec.startpos, rec.d_idx
    return upload_sequence(rec.encode("utf-8") if isinstance(rec, str) else bytes(rec))


def _segment_rows(dev, cap: int, launch) -> np.ndarray:
    """The segment rows of a launch that learns their number only by running: launch(d_rec, cap) writes up to `cap` rows and
    returns how many there are; where the guess was short (rare) it runs again with room for all of them."""
    while True:
        rec = torch.empty(cap * SEGMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        total = launch(rec, cap)
        if total <= cap:
            break
        cap = total
    return rec[: total * SEGMENT_DTYPE.itemsize].cpu().numpy().view(SEGMENT_DTYPE).copy()


def _with_room(launch, *caps):
    """What launch(*caps) allocates for an entry that learns how much it writes only by running: launch allocates for the capacities,
    calls the entry and returns (the allocation, what the entry needs of every capacity).  Where a guess was short (rare) it runs
    once more, with room for all the entry reported.  -> the last allocation"""
    out, need = launch(*caps)
    if any(n > c for n, c in zip(need, caps)):
        out, need = launch(*(max(c, n) for c, n in zip(caps, need)))
    return out


class ContigPipeline:
    """Runs records through the device pipeline with the reference's CLI parameters."""

    def __init__(self, model: DeviceModel, step_size: int = 50, batch_size: int = 256, min_mss_len: int = 50,
                 xdrop_len: int = 50, use_mss: bool = True, chunk_windows: int = 1 << 20, precise: bool = False,
                 fast: bool = False, fp32: bool = False):
        self.model = model
        self.step = int(step_size)
        self.batch = int(batch_size)
        self.min_mss_len = int(min_mss_len)
        self.xdrop_len = int(xdrop_len)
        self.use_mss = bool(use_mss)
        self.chunk_windows = int(chunk_windows)
        # Which forward kernels run:
        #   default  split operands -- every model has such a fused kernel (class probabilities within 1e-5 of a float64
        #            evaluation in the tests, attention models included: their avg[t] crosses to the second kernel as float32);
        #   fast     fp16 operands (2-2.5x faster; 1e-3 on all but ill-conditioned windows);
        #   precise  accepted and equal to the default since round 2 made the default fp32-grade for every model (it used to send
        #            attention models through the 30 Mbp/s plain-fp32 kernels);
        #   fp32     the plain-fp32 kernels of ref_kernels.hip with the reference's own batch loop -- the yardstick, for tools.
        if precise and fast:
            raise ValueError("precise and fast exclude each other")
        self.precise, self.fast = bool(precise), bool(fast)
        self.fp32 = bool(fp32)
        self.split = not self.fast and not self.fp32
        self.event_log = None        # bench.py: list collecting (start, end, windows) per GRU launch
        self._view = None            # this pipeline's own handle on the model (dgrp_model_view): its precision level is never
                                     # changed, so pipelines of different levels can share a model on a pool of host threads
        if self.step < 1 or self.batch < 1:
            raise ValueError("step_size and batch_size must be >= 1")

    @property
    def handle(self):
        if self._view is None:
            self._view = self.model.view(1 if self.split else 0)
        return self._view

    def close(self) -> None:
        if self._view is not None:
            lib().dgrp_model_destroy(self._view)
            self._view = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # A3-A6
    def merged(self, d_idx: torch.Tensor) -> torch.Tensor:
        m, L = self.model, lib()
        n = d_idx.numel()
        out = torch.zeros((n, m.classes), dtype=torch.float32, device=d_idx.device)      # np.zeros, prediction.py:103
        nwin = L.dgrp_window_count(n, m.vecsize, self.step)
        if self.fp32:
            # the reference's own loop (prediction.py:104-110): batches of B windows, batch i lands at row i * b * step
            # (b = size of THAT batch); the forward pass runs for several batches at a time
            B = self.batch
            fit = (4 << 30) // (2 * m.vecsize * m.units * 4 + m.vecsize * (m.classes + 1) * 4)      # h_t of both strands, fp32
            per = max(B, min(self.chunk_windows, fit) // B * B)
            w0 = i = 0
            while w0 < nwin:
                nw = min(per, nwin - w0)
                probs = m.forward_windows_reference(d_idx, self.step, w0, nw)
                for off in range(0, nw, B):
                    b = min(B, nw - off)
                    index = i * b * self.step
                    if index < n:
                        check(L.dgrp_get_max(_ptr(out[index:]), n - index, _ptr(probs[off:off + b]), m.vecsize, m.classes,
                                             self.step, b, stream_ptr()), "dgrp_get_max")
                    i += 1
                w0 += nw
            return out
        if self.event_log is None and self.chunk_windows >= (1 << 20):
            # the library's own loop over the record (attention models with small spills: chunks alternating between its lanes)
            wb = L.dgrp_forward_merge_record_workspace_bytes(self.handle, n, self.step)
            work = torch.empty(max(wb, 256), dtype=torch.uint8, device=d_idx.device)
            check(L.dgrp_forward_merge_record(self.handle, _ptr(d_idx), n, self.step, self.batch, _ptr(out), _ptr(work), work.numel(),
                                              stream_ptr()), "dgrp_forward_merge_record")
            return out
        chunk = max(16, min(self.chunk_windows, L.dgrp_forward_window_chunk(self.handle)))     # attention: the avg[t] spill bounds a launch
        work = None
        w0 = 0
        while w0 < nwin:
            nw = min(chunk, nwin - w0)
            wb = L.dgrp_forward_workspace_bytes(self.handle, nw)
            if work is None or work.numel() < wb:
                work = torch.empty(max(wb, 256), dtype=torch.uint8, device=d_idx.device)
            if self.event_log is not None:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            check(L.dgrp_forward_merge(self.handle, _ptr(d_idx), n, self.step, self.batch, w0, nw, _ptr(out),
                                       _ptr(work), work.numel(), stream_ptr()), "dgrp_forward_merge")
            if self.event_log is not None:
                ev1.record()
                self.event_log.append((ev0, ev1, nw))
            w0 += nw
        return out

    # A7-A10 (or A8)
    def labels(self, merged: torch.Tensor) -> torch.Tensor:
        L = lib()
        n, c = merged.shape
        dev = merged.device
        if n == 0:
            return torch.empty(0, dtype=torch.int8, device=dev)
        if self.use_mss:
            scores = torch.empty(n, dtype=torch.float64, device=dev)
            cls = torch.empty(n, dtype=torch.int8, device=dev)
            check(L.dgrp_scores(_ptr(merged), n, c, _ptr(scores), _ptr(cls), stream_ptr()), "dgrp_scores")
            return self.labels_from_scores(scores, cls)
        labels = torch.empty(n, dtype=torch.int8, device=dev)
        work = torch.empty(4096, dtype=torch.uint8, device=dev)
        check(L.dgrp_softmax_labels(_ptr(merged), n, c, None, _ptr(labels), _ptr(work), work.numel(),
                                    stream_ptr()), "dgrp_softmax_labels")
        return labels

    # A9-A10 on scores / classes that are already there (distributed.run_split assembles them from all ranks)
    def labels_from_scores(self, scores: torch.Tensor, cls: torch.Tensor) -> torch.Tensor:
        L = lib()
        n, dev = scores.numel(), scores.device
        labels = torch.empty(n, dtype=torch.int8, device=dev)
        if n == 0:
            return labels
        wb = L.dgrp_mss_workspace_bytes(n)
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        check(L.dgrp_mss_labels(_ptr(scores), _ptr(cls), n, self.model.classes, self.min_mss_len, self.xdrop_len, _ptr(labels),
                                None, _ptr(work), wb, stream_ptr()), "dgrp_mss_labels")
        return labels

    # A11
    def segments(self, labels: torch.Tensor, offset: int, contig: int = 0, cap: Optional[int] = None) -> np.ndarray:
        L = lib()
        n = labels.numel()
        dev = labels.device
        if n == 0:
            return np.zeros(0, SEGMENT_DTYPE)
        wb = L.dgrp_segments_workspace_bytes(n)
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)

        def launch(rec, cap):
            check(L.dgrp_segments(_ptr(labels), n, offset, contig, _ptr(rec), cap, _ptr(count), _ptr(work), wb,
                                  stream_ptr()), "dgrp_segments")
            return int(count.item())
        return _segment_rows(dev, cap if cap is not None else max(1024, n // 64), launch)

    # predict --track_dir
    def track_text(self, merged: torch.Tensor, startpos: int, name, cls: int, digits: int = 2, bin: int = 1) -> bytes:
        """bedGraph lines of class `cls` of one record's merged probabilities (ContigPipeline.merged): `name` (str, surrogateescape, or
        bytes) in the first column, row i at coordinate startpos + i, bins of `bin` bases, values with `digits` decimals."""
        return self.track_text_device(merged, startpos, name, cls, digits, bin).cpu().numpy().tobytes()

    def track_text_device(self, merged: torch.Tensor, startpos: int, name, cls: int, digits: int = 2, bin: int = 1) -> torch.Tensor:
        """track_text's bytes as a uint8 device tensor, where the kernels wrote them (nothing but the size is read back): a
        one-record, one-class call of track_text_batch_device."""
        if merged.ndim == 2 and merged.shape[0] == 0:
            return torch.empty(0, dtype=torch.uint8, device=merged.device)
        return self.track_text_batch_device(merged, [0], [len(merged)], [startpos], [name], [cls], digits, bin)[0]

    def run_idx(self, d_idx: torch.Tensor, startpos: int, contig: int = 0) -> np.ndarray:
        """Segment records of one record whose class indices are on the device: one dgrp_predict_record call
        (the staged merged -> labels -> segments path is kept for callers that time or inspect the stages)."""
        if self.event_log is not None or self.fp32:
            return self.segments(self.labels(self.merged(d_idx)), startpos, contig)
        L = lib()
        n = d_idx.numel()
        if n == 0:
            return np.zeros(0, SEGMENT_DTYPE)
        dev = d_idx.device
        wb = L.dgrp_record_workspace_bytes(self.handle, n, self.step, int(self.use_mss))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        count = C.c_int64(0)

        def launch(rec, cap):
            check(L.dgrp_predict_record(self.handle, _ptr(d_idx), n, self.step, self.batch, self.min_mss_len,
                                        self.xdrop_len, int(self.use_mss), int(startpos), int(contig), _ptr(rec), cap,
                                        C.byref(count), _ptr(work), wb, stream_ptr()), "dgrp_predict_record")
            return int(count.value)
        return _segment_rows(dev, max(1024, n // 64), launch)

    def batchable(self) -> bool:
        """dgrp_predict_batch covers every model on the MSS path (the -m softmax is normalised per record)."""
        return self.use_mss and self.event_log is None and not self.fp32 and not getattr(self.model, "fp32_only", False)

    def run_batch(self, d_base: torch.Tensor, offsets, lengths, startposes, contigs, d_probs: Optional[torch.Tensor] = None) -> np.ndarray:
        """Segment records of MANY short records whose class indices lie in one device buffer (record r: `lengths[r]`
        >= 1 indices at `d_base[offsets[r]:]`): one dgrp_predict_batch call.  Rows come back in record order.  With `d_probs`
        (float32 [dgrp_batch_rows, C]) the call is dgrp_predict_batch_probs and the merged probabilities are left there."""
        L = lib()
        nrec = len(lengths)
        if nrec == 0:
            return np.zeros(0, SEGMENT_DTYPE)
        off = np.ascontiguousarray(offsets, np.int64)
        ln = np.ascontiguousarray(lengths, np.int64)
        sp = np.ascontiguousarray(startposes, np.int64)
        cg = np.ascontiguousarray(contigs, np.int32)
        dev = d_base.device
        wb = L.dgrp_batch_workspace_bytes(self.handle, nrec, ln.ctypes.data, self.step)
        if wb <= 0:
            raise ValueError("run_batch: every record of a batch needs at least one base")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        count = C.c_int64(0)

        def launch(rec, cap):
            args = (self.handle, _ptr(d_base), nrec, off.ctypes.data, ln.ctypes.data, sp.ctypes.data, cg.ctypes.data, self.step,
                    self.batch, self.min_mss_len, self.xdrop_len, _ptr(rec), cap, C.byref(count), _ptr(work), wb, stream_ptr())
            if d_probs is None:
                check(L.dgrp_predict_batch(*args), "dgrp_predict_batch")
            else:
                check(L.dgrp_predict_batch_probs(*args, _ptr(d_probs)), "dgrp_predict_batch_probs")
            return int(count.value)
        return _segment_rows(dev, max(1024, int(ln.sum()) // 64 + 2 * nrec), launch)

    def track_text_batch_device(self, d_probs: torch.Tensor, row0, lengths, startposes, names, classes, digits: int = 2,
                                bin: int = 1) -> Tuple[torch.Tensor, np.ndarray]:
        """The track text of many records and classes in one dgrp_track_text_batch call: record r is rows [row0[r], row0[r] +
        lengths[r]) of `d_probs` (float32 [*, C]), `names[r]` (str, surrogateescape, or bytes) its first column.  -> (uint8 device
        tensor, offsets [len(classes) + 1]): the text is class-major, class classes[k] of all records in order at [off[k], off[k + 1])."""
        L = lib()
        r0, ln, sp, cl = ContigPipeline._track_tables(d_probs, "track_text_batch_device", row0, lengths, startposes, classes)
        c, nrec, ncls, dev = int(d_probs.shape[1]), len(ln), len(cl), d_probs.device
        blob, noff = name_blob(names)[1:]
        wb = L.dgrp_track_batch_workspace_bytes(nrec, ln.ctypes.data, sp.ctypes.data, int(bin), ncls, len(blob))
        if wb <= 0:
            raise ValueError(f"track_text_batch_device: bad record lengths, start positions, bin {bin} or class count {ncls}")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        nb = ln // int(bin) + 2                                               # (a line per bin at most; the guess fits most runs)
        nlen = np.diff(noff)
        cap = ncls * int(min(int((nb * (nlen + 50)).sum()), (1 << 20) + int((nb * (nlen + 12)).sum())))
        off = np.zeros(ncls + 1, np.int64)

        def launch(cap):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            check(L.dgrp_track_text_batch(_ptr(d_probs), c, nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data, blob, noff.ctypes.data,
                                          cl.ctypes.data, ncls, int(digits), int(bin), _ptr(text), cap, off.ctypes.data, _ptr(work), wb,
                                          stream_ptr()), "dgrp_track_text_batch")
            return text, (int(off[ncls]),)
        return _with_room(launch, cap)[:int(off[ncls])], off

    def track_index_batch_device(self, d_probs: torch.Tensor, row0, lengths, startposes, names, classes, digits: int = 2,
                                 bin: int = 1, depth: int = 5) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The tabix index of the text track_text_batch_device gives for the same arguments, in text offsets (one
        dgrp_track_index_batch call, read back once): -> (chunks, chunk_off [len(classes) + 1], linear [len(classes), W], wpref
        [records + 1]).  chunks (tabix.CHUNK_DTYPE) is class-major, class classes[k] at [chunk_off[k], chunk_off[k + 1]), offsets
        inside that class's slice of the text; record r of class k has its windows at linear[k, wpref[r]:wpref[r + 1]], -1 where
        none of its lines ends behind the window.  A record that ends above 2^29 raises tabix.IndexRefused.  depth 6: the bins of
        a CSI index of that depth (one dgrp_track_csi_batch call), records up to 2^32."""
        from .tabix import CHUNK_DTYPE, window_prefix
        L = lib()
        r0, ln, sp, cl = ContigPipeline._track_tables(d_probs, "track_index_batch_device", row0, lengths, startposes, classes)
        c, nrec, ncls, dev = int(d_probs.shape[1]), len(ln), len(cl), d_probs.device
        depth = int(depth)
        wpref = window_prefix(sp + ln, depth)
        blob, noff = name_blob(names)[1:]
        nwin = int(wpref[-1])
        if depth == 5:
            wb = L.dgrp_track_index_workspace_bytes(nrec, ln.ctypes.data, sp.ctypes.data, int(bin), ncls, len(blob))
        else:
            wb = L.dgrp_track_csi_workspace_bytes(nrec, ln.ctypes.data, sp.ctypes.data, int(bin), ncls, len(blob), depth)
        if wb <= 0:
            raise ValueError(f"track_index_batch_device: bad record lengths, start positions, bin {bin} or class count {ncls}")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        linear = torch.empty(max(ncls * nwin, 1), dtype=torch.int64, device=dev)
        cap = ncls * (2 * nwin + 4 * nrec + 16)             # (a leaf chunk per window, one per line across a window edge, a few per
                                                            # record: 1.2 per window on a 250 Mbp record; the guess fits most runs)
        off = np.zeros(ncls + 1, np.int64)

        def launch(cap):
            chunks = torch.empty(max(cap, 1) * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            if depth == 5:
                check(L.dgrp_track_index_batch(_ptr(d_probs), c, nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data, blob,
                                               noff.ctypes.data, cl.ctypes.data, ncls, int(digits), int(bin), _ptr(chunks), cap,
                                               off.ctypes.data, _ptr(linear), ncls * nwin, _ptr(work), wb, stream_ptr()),
                      "dgrp_track_index_batch")
            else:
                check(L.dgrp_track_csi_batch(_ptr(d_probs), c, nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data, blob,
                                             noff.ctypes.data, cl.ctypes.data, ncls, int(digits), int(bin), depth, _ptr(chunks), cap,
                                             off.ctypes.data, _ptr(linear), ncls * nwin, _ptr(work), wb, stream_ptr()),
                      "dgrp_track_csi_batch")
            return chunks, (int(off[ncls]),)
        host = _with_room(launch, cap)[:int(off[ncls]) * CHUNK_DTYPE.itemsize].cpu().numpy().view(CHUNK_DTYPE)
        return host, off, linear[:ncls * nwin].cpu().numpy().reshape(ncls, nwin), wpref

    @staticmethod
    def _track_tables(d_probs: torch.Tensor, who: str, row0, lengths, startposes, classes=()):
        """The check every method that takes `d_probs` makes, and its record tables as the library reads them."""
        if d_probs.dtype != torch.float32 or d_probs.ndim != 2 or not d_probs.is_contiguous():
            raise ValueError(f"{who} takes a contiguous float32 [rows, C] array")
        return (np.ascontiguousarray(row0, np.int64), np.ascontiguousarray(lengths, np.int64), np.ascontiguousarray(startposes, np.int64),
                np.ascontiguousarray(classes, np.int32))

    def track_sections_batch_device(self, d_probs: torch.Tensor, row0, lengths, startposes, classes, digits: int = 2, bin: int = 1,
                                    chrom0: int = 0):
        """The bigWig sections of many records and classes in one dgrp_track_sections_batch call (arguments as
        track_text_batch_device, no names): -> (uint8 device tensor of the uncompressed sections, class-major; byte offsets
        [len(classes) + 1]; uint8 device tensor of the section table, rows of bigwig.SECTION_DTYPE; section offsets [len(classes) + 1]).
        `rec` counts the records of this call, chromId is chrom0 + rec."""
        from .bigwig import SECTION_DTYPE
        L = lib()
        r0, ln, sp, cl = ContigPipeline._track_tables(d_probs, "track_sections_batch_device", row0, lengths, startposes, classes)
        c, nrec, ncls, dev = int(d_probs.shape[1]), len(ln), len(cl), d_probs.device
        wb = L.dgrp_track_sections_workspace_bytes(nrec, ln.ctypes.data, sp.ctypes.data, int(bin), ncls)
        if wb <= 0:
            raise ValueError(f"track_sections_batch_device: bad record lengths, start positions (ends above 2^32 - 1?), bin {bin} or class count {ncls}")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        nb = int((ln // int(bin) + 2).sum())
        cap = ncls * min(12 * nb + 24 * (nb // 1024 + nrec), (1 << 20) + 3 * nb)        # (the guess fits most runs)
        tcap = ncls * (cap // (ncls * 12 * 1024) + nrec + 1)
        off, soff = np.zeros(ncls + 1, np.int64), np.zeros(ncls + 1, np.int64)

        def launch(cap, tcap):
            out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
            table = torch.empty(max(tcap, 1) * SECTION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            check(L.dgrp_track_sections_batch(_ptr(d_probs), c, nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data, cl.ctypes.data, ncls,
                                              int(digits), int(bin), int(chrom0), _ptr(out), cap, off.ctypes.data, _ptr(table), tcap, soff.ctypes.data,
                                              _ptr(work), wb, stream_ptr()), "dgrp_track_sections_batch")
            return (out, table), (int(off[ncls]), int(soff[ncls]))
        out, table = _with_room(launch, cap, tcap)
        return out[:int(off[ncls])], off, table[:int(soff[ncls]) * SECTION_DTYPE.itemsize], soff

    def track_zoom_batch_device(self, d_probs: torch.Tensor, row0, lengths, startposes, classes, digits: int = 2, bin: int = 1,
                                chrom0: int = 0):
        """The zoom records of the same arguments in one dgrp_track_zoom_batch call: -> (uint8 device tensor of the 32-byte records;
        record offsets [len(classes) * bigwig.ZOOM_LEVELS + 1], segment k * ZOOM_LEVELS + level; uint8 device tensor of the block
        table, rows of bigwig.ZOOM_BLOCK_DTYPE; block offsets, as the record offsets; totals, bigwig.TOTALS_DTYPE [len(classes)])."""
        from .bigwig import TOTALS_DTYPE, ZOOM_BLOCK_DTYPE, ZOOM_LEVELS
        L = lib()
        r0, ln, sp, cl = ContigPipeline._track_tables(d_probs, "track_zoom_batch_device", row0, lengths, startposes, classes)
        c, nrec, ncls, dev = int(d_probs.shape[1]), len(ln), len(cl), d_probs.device
        wb = L.dgrp_track_zoom_workspace_bytes(nrec, ln.ctypes.data, sp.ctypes.data, int(bin), ncls)
        if wb <= 0:
            raise ValueError(f"track_zoom_batch_device: bad record lengths, start positions (ends above 2^32 - 1?), bin {bin} or class count {ncls}")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        nseg = ncls * ZOOM_LEVELS
        nwin = int((ln // (16 * int(bin)) + 2).sum())
        cap = 32 * ncls * (nwin // 4 + ZOOM_LEVELS * nrec + 64)                     # (the guess fits sparse tracks)
        tcap = cap // (32 * 1024) + nseg
        roff, boff = np.zeros(nseg + 1, np.int64), np.zeros(nseg + 1, np.int64)
        totals = np.zeros(ncls, TOTALS_DTYPE)

        def launch(cap, tcap):
            out = torch.empty(max(cap, 32), dtype=torch.uint8, device=dev)
            table = torch.empty(max(tcap, 1) * ZOOM_BLOCK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            check(L.dgrp_track_zoom_batch(_ptr(d_probs), c, nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data, cl.ctypes.data, ncls,
                                          int(digits), int(bin), int(chrom0), _ptr(out), cap, roff.ctypes.data, _ptr(table), tcap, boff.ctypes.data,
                                          totals.ctypes.data, _ptr(work), wb, stream_ptr()), "dgrp_track_zoom_batch")
            return (out, table), (32 * int(roff[nseg]), int(boff[nseg]))
        out, table = _with_room(launch, cap, tcap)
        return out[:32 * int(roff[nseg])], roff, table[:int(boff[nseg]) * ZOOM_BLOCK_DTYPE.itemsize], boff, totals

    @staticmethod
    def zlib_compress_device(d_in: torch.Tensor, d_rows: torch.Tensor, stride: int, level: int = 1):
        """The blocks of the uint8 device tensor `d_in` that the rows of `d_rows` name (uint8 device tensor, `stride` bytes a row,
        each beginning with int64 offset and int64 length: a section or zoom block table as it comes) as zlib streams back to back
        (dgrp_zlib_compress_batch): -> (uint8 device tensor, int64 device tensor of the streams' sizes).  One read-back: the total."""
        L = lib()
        nblk = int(d_rows.numel()) // stride
        dev = d_in.device
        if nblk == 0:
            return torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
        n = int(d_in.numel())
        cap = int(L.dgrp_zlib_bound(nblk, n))
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        sizes = torch.empty(nblk, dtype=torch.int64, device=dev)
        wb = int(L.dgrp_zlib_workspace_bytes(nblk, int(level)))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        got = C.c_int64(0)
        check(L.dgrp_zlib_compress_batch(_ptr(d_in), n, _ptr(d_rows), stride, nblk, int(level), _ptr(out), cap, _ptr(sizes), C.byref(got),
                                         _ptr(work), wb, stream_ptr()), "dgrp_zlib_compress_batch")
        return out[:got.value], sizes

    def batch_track_texts(self, d_probs: torch.Tensor, row0, ln, startposes, names, spec, chrom0: int = 0):
        """The track texts of a batch from its merged probabilities (run_batch_probs: record r at rows [row0[r], row0[r] + ln[r])),
        one dgrp_track_text_batch call: texts[k] = the bytes of class spec.classes[k] for the whole batch (what the records' texts
        give one after the other); with spec.gzip_level the BGZF members of that slice instead (no EOF member), deflated on the
        device in gz.GZIP_PIECE pieces: members span records and a batch ends in a short member; with spec.index the batch's
        tracks.WriteIndex comes with them (texts.index); with spec.bigwig tracks.bigwig_write's result instead (chrom0: the
        ordinal of the batch's first record in its input)."""
        if spec.bigwig:                                      # --track_bigwig: sections and zoom blocks instead of text
            from .tracks import bigwig_write
            return bigwig_write(self, d_probs, row0, ln, startposes, names, spec, chrom0)
        d_text, off = self.track_text_batch_device(d_probs, row0, ln, startposes, names, spec.classes, spec.digits, spec.bin)
        index = None
        if spec.gzip_level is not None and spec.index:
            from .tracks import write_index
            index = write_index(self, d_probs, row0, ln, startposes, names, spec)
        del d_probs
        if spec.gzip_level is None:
            host = d_text.cpu().numpy()
            return [host[off[k]:off[k + 1]].tobytes() for k in range(len(spec.classes))]
        from .gz import bgzf_members_device
        from .tracks import TrackTexts
        texts = TrackTexts(bgzf_members_device(d_text[int(off[k]):int(off[k + 1])], spec.gzip_level) for k in range(len(spec.classes)))
        texts.index = index
        return texts

    # predict --bed_dir
    def row_scores_batch(self, d_probs: torch.Tensor, row0, lengths, startposes, rows: np.ndarray, row_off) -> np.ndarray:
        """The scores (ROW_SCORE_DTYPE, one per row) of the segment rows of many records in one dgrp_row_scores_batch call: record r
        is rows [row0[r], row0[r] + lengths[r]) of `d_probs` (float32 [*, C]), its first row has coordinate startposes[r], and its
        segment rows are rows[row_off[r]:row_off[r + 1]] (SEGMENT_DTYPE, original coordinates, clipped to the record)."""
        L = lib()
        r0, ln, sp, _cl = ContigPipeline._track_tables(d_probs, "row_scores_batch", row0, lengths, startposes)
        rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
        ro = np.ascontiguousarray(row_off, np.int64)
        nrec = len(ln)
        if len(ro) != nrec + 1 or len(r0) != nrec or len(sp) != nrec or (nrec and int(ro[-1]) > len(rows)):
            raise ValueError("row_scores_batch: tables of different lengths, or row offsets beyond the rows")
        if nrec and int((r0 + ln).max()) > d_probs.shape[0]:
            raise ValueError("row_scores_batch: a record lies beyond the probability array")
        out = np.zeros(len(rows), ROW_SCORE_DTYPE)
        if nrec == 0 or len(rows) == 0:
            return out
        return self._row_scores_device(d_probs, r0, ln, sp, rows, ro)[1].cpu().numpy().view(ROW_SCORE_DTYPE).copy()

    @staticmethod
    def _row_scores_device(d_probs: torch.Tensor, r0, ln, sp, rows: np.ndarray, ro):
        """row_scores_batch on its checked tables (at least one record and one row): -> (the rows, the scores) as uint8 device
        tensors, complete behind the call on the current stream."""
        L = lib()
        nrec, dev = len(ln), d_probs.device
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        d_scores = torch.zeros(len(rows) * ROW_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        wb = int(L.dgrp_row_scores_workspace_bytes(nrec, int(ro[-1] - ro[0])))
        work = torch.empty(max(wb, 256), dtype=torch.uint8, device=dev)
        check(L.dgrp_row_scores_batch(_ptr(d_probs), int(d_probs.shape[1]), nrec, r0.ctypes.data, ln.ctypes.data, sp.ctypes.data,
                                      _ptr(d_rows), ro.ctypes.data, _ptr(d_scores), _ptr(work), work.numel(), stream_ptr()),
              "dgrp_row_scores_batch")
        return d_rows, d_scores

    # predict --bed_gzip, --bed_index: rows and scores stay on the device
    @staticmethod
    def bed_text_batch(names, by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int = 0) -> torch.Tensor:
        """The BED lines of `d_rows` (uint8 device tensor of SEGMENT_DTYPE rows) with `d_scores` (the same of ROW_SCORE_DTYPE) as a
        uint8 device tensor: one dgrp_bed_text_batch call, the bytes bed.format_rows gives for the same arrays on the host.  The
        text is complete behind the call on the current stream."""
        L = lib()
        nrows, dev = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize, d_rows.device
        if int(d_scores.numel()) != nrows * ROW_SCORE_DTYPE.itemsize:
            raise ValueError(f"bed_text_batch: {nrows} rows but {int(d_scores.numel())} bytes of scores")
        raw, blob, off = name_blob(names)
        wb = int(L.dgrp_bed_text_workspace_bytes(nrows, len(raw), len(blob)))
        if wb <= 0:
            raise ValueError(f"bed_text_batch: bad row count {nrows} or names")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        longest = max(len(x) for x in raw)
        cap = min(int(L.dgrp_format_bed_bound(nrows, longest)), nrows * (longest + 72))       # (the guess fits most runs)
        got = C.c_int64(0)

        def launch(cap):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            check(L.dgrp_bed_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), _ptr(d_rows), _ptr(d_scores), nrows, int(min_score),
                                        _ptr(text), cap, C.byref(got), _ptr(work), wb, stream_ptr()), "dgrp_bed_text_batch")
            return text, (int(got.value),)
        return _with_room(launch, cap)[:got.value]

    @staticmethod
    def bed_index_batch(names, by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int, rec_end, depth: int = 5):
        """The tabix pieces of the text bed_text_batch gives for the same arguments, in text offsets (one dgrp_bed_index_batch call,
        read back once): -> (chunks tabix.CHUNK_DTYPE, linear int64 [windows], wpref int64 [records + 1], last_end int64 [records]);
        record r (a row's contig with by_contig, else 0) ends at rec_end[r] and has its windows at linear[wpref[r]:wpref[r + 1]].
        What bed.reference_index_parts states.  A record that ends above 2^29 raises tabix.IndexRefused.  depth 6: the bins of a
        CSI index of that depth (one dgrp_bed_csi_batch call), records up to 2^32."""
        from .tabix import CHUNK_DTYPE, window_prefix
        L = lib()
        nrows, dev = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize, d_rows.device
        ends = np.ascontiguousarray(rec_end, np.int64)
        nrec = len(ends)
        depth = int(depth)
        wpref = window_prefix(ends, depth)
        raw, blob, off = name_blob(names)
        nwin = int(wpref[-1])
        wb = int(L.dgrp_bed_index_workspace_bytes(nrows, len(raw), len(blob), nrec))
        if wb <= 0:
            raise ValueError(f"bed_index_batch: bad row count {nrows}, record count {nrec} or names")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        linear = torch.full((max(nwin, 1),), -1, dtype=torch.int64, device=dev)
        last = torch.zeros(max(nrec, 1), dtype=torch.int64, device=dev)
        cap = min(nrows, 2 * nwin + 4 * nrec + 16)          # (a chunk per line at most; on long records about one per window)
        got = C.c_int64(0)

        def launch(cap):
            chunks = torch.empty(max(cap, 1) * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            if depth == 5:
                check(L.dgrp_bed_index_batch(blob, off.ctypes.data, len(raw), int(by_contig), _ptr(d_rows), _ptr(d_scores), nrows,
                                             int(min_score), nrec, ends.ctypes.data, _ptr(chunks), cap, C.byref(got), _ptr(linear), nwin,
                                             _ptr(last), _ptr(work), wb, stream_ptr()), "dgrp_bed_index_batch")
            else:
                check(L.dgrp_bed_csi_batch(blob, off.ctypes.data, len(raw), int(by_contig), _ptr(d_rows), _ptr(d_scores), nrows,
                                           int(min_score), nrec, ends.ctypes.data, depth, _ptr(chunks), cap, C.byref(got), _ptr(linear),
                                           nwin, _ptr(last), _ptr(work), wb, stream_ptr()), "dgrp_bed_csi_batch")
            return chunks, (int(got.value),)
        host = _with_room(launch, cap)[:got.value * CHUNK_DTYPE.itemsize].cpu().numpy().view(CHUNK_DTYPE)
        return host, linear[:nwin].cpu().numpy(), wpref, last[:nrec].cpu().numpy()

    def bed_write(self, d_probs: torch.Tensor, row0, lengths, startposes, rows: np.ndarray, row_off, names, by_contig: bool, plan,
                  chrom0: int = 0):
        """One write of a BGZF BED (bed.BedWrite) for the arguments of row_scores_batch, `names` as bed.format_rows takes them and
        `plan` the bed.BedPlan: scores, text and, with plan.index, the index's pieces are made on the device from the uploaded rows;
        the text is deflated there in gz.GZIP_PIECE pieces (members span records, a write ends in a short member) and only the
        members come back.  row_off must cover all rows (row_off[0] = 0, row_off[-1] = len(rows)).  With plan.bigbed the write is
        `bigbed_write`'s (chrom0: the ordinal of the first record in its input)."""
        if plan.bigbed:                                     # --bed_bigbed: item blocks and zoom blocks instead of text
            return self.bigbed_write(d_probs, row0, lengths, startposes, rows, row_off, names, by_contig, plan, chrom0)
        if getattr(plan, "gff3", False):                    # --bed_gff3: GFF3 lines instead of BED lines
            return self.gff_write(d_probs, row0, lengths, startposes, rows, row_off, names, by_contig, plan)
        if getattr(plan, "rmout", False):                   # --bed_rmout: the lines of a RepeatMasker listing instead
            return self.rmout_write(d_probs, row0, lengths, startposes, rows, row_off, names, by_contig, plan)
        from .bed import BedWrite
        from .gz import bgzf_members_device
        from .tabix import end_refusal
        from .tracks import index_depth
        raw = name_blob(names)[0]
        r0, ln, sp, _cl = ContigPipeline._track_tables(d_probs, "bed_write", row0, lengths, startposes)
        ends = sp + ln
        depth = index_depth(getattr(plan, "index_format", "tbi"))
        refused = end_refusal(ends, raw, depth) if plan.index else None
        rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
        ro = np.ascontiguousarray(row_off, np.int64)
        if len(rows) == 0:
            return BedWrite(b"", raw, refused)
        if len(ro) != len(ln) + 1 or int(ro[0]) != 0 or int(ro[-1]) != len(rows):
            raise ValueError("bed_write: the row offsets must cover all rows")
        d_rows, d_scores = self._row_scores_device(d_probs, r0, ln, sp, rows, ro)
        d_text = self.bed_text_batch(raw, by_contig, d_rows, d_scores, plan.min_score)
        parts = (None,) * 4
        if plan.index and refused is None and int(d_text.numel()):
            parts = self.bed_index_batch(raw, by_contig, d_rows, d_scores, plan.min_score, ends, depth)
        del d_probs, d_rows, d_scores
        return BedWrite(bgzf_members_device(d_text, plan.gzip_level), raw, refused, *parts)

    # predict --bed_gff3: the rows as GFF3 feature lines (gff.py)
    @staticmethod
    def _gff_tables(names, class_names):
        """(escaped record names, their blob and offsets, class-name blob or None, its offsets' address or None, class-name count,
        the offsets array to keep alive)."""
        from .gff import escape_seqid, escape_value
        raw, blob, off = name_blob([escape_seqid(nm) for nm in names])
        if not class_names:
            return raw, blob, off, None, None, 0, None
        _c, cblob, coff = name_blob([escape_value(nm) for nm in class_names])
        return raw, blob, off, cblob, coff.ctypes.data, len(class_names), coff

    @staticmethod
    def gff_text_batch(names, by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int = 0, class_names=None,
                       id0: int = 0):
        """The GFF3 feature lines (no header) of `d_rows` with `d_scores` (as bed_text_batch takes them) -> (uint8 device tensor,
        lines): one dgrp_gff_text_batch call, the bytes gff.reference_lines gives for the same arguments.  names and class_names as
        they come: escaped here, once.  The text is complete behind the call on the current stream."""
        L = lib()
        nrows, dev = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize, d_rows.device
        if int(d_scores.numel()) != nrows * ROW_SCORE_DTYPE.itemsize:
            raise ValueError(f"gff_text_batch: {nrows} rows but {int(d_scores.numel())} bytes of scores")
        raw, blob, off, cblob, coff, nc, _keep = ContigPipeline._gff_tables(names, class_names)
        wb = int(L.dgrp_gff_text_workspace_bytes(nrows, len(raw), len(blob), nc, len(cblob or b"")))
        if wb <= 0:
            raise ValueError(f"gff_text_batch: bad row count {nrows} or names")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        cap = nrows * (max(len(x) for x in raw) + 120)      # (a guess that fits most runs; a longer text takes the retry)
        got, lines = C.c_int64(0), C.c_int64(0)

        def launch(cap):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            check(L.dgrp_gff_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, coff, nc, _ptr(d_rows), _ptr(d_scores),
                                        nrows, int(min_score), int(id0), _ptr(text), cap, C.byref(got), C.byref(lines), _ptr(work), wb,
                                        stream_ptr()), "dgrp_gff_text_batch")
            return text, (int(got.value),)
        return _with_room(launch, cap)[:got.value], int(lines.value)

    @staticmethod
    def gff_index_batch(names, by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int, rec_end, class_names=None,
                        id0: int = 0, depth: int = 5):
        """bed_index_batch for the text gff_text_batch gives for the same arguments (one dgrp_gff_index_batch call, at depth 6 one
        dgrp_gff_csi_batch call): what gff.reference_index_parts states."""
        from .tabix import CHUNK_DTYPE, window_prefix
        L = lib()
        nrows, dev = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize, d_rows.device
        ends = np.ascontiguousarray(rec_end, np.int64)
        nrec = len(ends)
        depth = int(depth)
        wpref = window_prefix(ends, depth)
        raw, blob, off, cblob, coff, nc, _keep = ContigPipeline._gff_tables(names, class_names)
        nwin = int(wpref[-1])
        wb = int(L.dgrp_gff_index_workspace_bytes(nrows, len(raw), len(blob), nc, len(cblob or b""), nrec))
        if wb <= 0:
            raise ValueError(f"gff_index_batch: bad row count {nrows}, record count {nrec} or names")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        linear = torch.full((max(nwin, 1),), -1, dtype=torch.int64, device=dev)
        last = torch.zeros(max(nrec, 1), dtype=torch.int64, device=dev)
        cap = min(nrows, 2 * nwin + 4 * nrec + 16)
        got = C.c_int64(0)

        def launch(cap):
            chunks = torch.empty(max(cap, 1) * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            if depth == 5:
                check(L.dgrp_gff_index_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, coff, nc, _ptr(d_rows), _ptr(d_scores),
                                             nrows, int(min_score), int(id0), nrec, ends.ctypes.data, _ptr(chunks), cap, C.byref(got),
                                             _ptr(linear), nwin, _ptr(last), _ptr(work), wb, stream_ptr()), "dgrp_gff_index_batch")
            else:
                check(L.dgrp_gff_csi_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, coff, nc, _ptr(d_rows), _ptr(d_scores),
                                           nrows, int(min_score), int(id0), nrec, ends.ctypes.data, depth, _ptr(chunks), cap,
                                           C.byref(got), _ptr(linear), nwin, _ptr(last), _ptr(work), wb, stream_ptr()),
                      "dgrp_gff_csi_batch")
            return chunks, (int(got.value),)
        host = _with_room(launch, cap)[:got.value * CHUNK_DTYPE.itemsize].cpu().numpy().view(CHUNK_DTYPE)
        return host, linear[:nwin].cpu().numpy(), wpref, last[:nrec].cpu().numpy()

    def gff_write(self, d_probs: torch.Tensor, row0, lengths, startposes, rows: np.ndarray, row_off, names, by_contig: bool, plan):
        """One write of a GFF3 file (gff.GffWrite) for the arguments of bed_write: the scores are summed now and stay on the device
        with the rows; the text, its index pieces and, with plan.gzip_level, its BGZF members are made when bed.BedFiles renders the
        write with the lines in front of it (the ID ordinals run through the file), on the stream that is current then."""
        from .gff import GffText, GffWrite
        from .tabix import end_refusal
        from .tracks import index_depth
        raw = name_blob(names)[0]
        r0, ln, sp, _cl = ContigPipeline._track_tables(d_probs, "gff_write", row0, lengths, startposes)
        ends = sp + ln
        depth = index_depth(getattr(plan, "index_format", "tbi"))
        refused = end_refusal(ends, raw, depth) if plan.index else None
        rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
        ro = np.ascontiguousarray(row_off, np.int64)
        if len(rows) == 0:
            return GffWrite(raw, refused)
        if len(ro) != len(ln) + 1 or int(ro[0]) != 0 or int(ro[-1]) != len(rows):
            raise ValueError("gff_write: the row offsets must cover all rows")
        d_rows, d_scores = self._row_scores_device(d_probs, r0, ln, sp, rows, ro)
        made = torch.cuda.Event()
        made.record()

        def render(id0: int) -> GffText:
            from .gz import bgzf_members_device
            made.wait()                                     # (the renderer's stream may be another one than the scores')
            d_text, lines = self.gff_text_batch(raw, by_contig, d_rows, d_scores, plan.min_score, plan.class_names, id0)
            parts = (None,) * 4
            if plan.index and refused is None and int(d_text.numel()):
                parts = self.gff_index_batch(raw, by_contig, d_rows, d_scores, plan.min_score, ends, plan.class_names, id0, depth)
            if plan.gzip_level is None:
                return GffText(d_text.cpu().numpy().tobytes(), lines)
            return GffText(bgzf_members_device(d_text, plan.gzip_level), lines, *parts)
        return GffWrite(raw, refused, render)

    # predict --bed_rmout: the rows as the lines of a RepeatMasker listing (rmout.py)
    @staticmethod
    def rmout_text_batch(names, by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int, rec_end, pairs,
                         join_gap: int = -1, id0: int = 0):
        """The lines (no title lines) of `d_rows` with `d_scores` (as bed_text_batch takes them) -> (uint8 device tensor, lines, IDs
        used): one dgrp_rmout_text_batch call, what rmout.reference_lines gives for the same arguments.  pairs[L - 1] = (repeat,
        class/family) of label L; record r (a row's contig with by_contig, else 0) ends at rec_end[r].  The text is complete behind
        the call on the current stream."""
        L = lib()
        nrows, dev = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize, d_rows.device
        if int(d_scores.numel()) != nrows * ROW_SCORE_DTYPE.itemsize:
            raise ValueError(f"rmout_text_batch: {nrows} rows but {int(d_scores.numel())} bytes of scores")
        ends = np.ascontiguousarray(rec_end, np.int64)
        raw, blob, off = name_blob(names)
        craw, cblob, coff = name_blob([x for pair in pairs for x in pair])
        wb = int(L.dgrp_rmout_text_workspace_bytes(nrows, len(raw), len(blob), len(pairs), len(cblob), len(ends)))
        if wb <= 0:
            raise ValueError(f"rmout_text_batch: bad row count {nrows}, record count {len(ends)} or names")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        cap = nrows * (max(max(len(x) for x in raw), 16) + 120)             # (a guess that fits most runs; a longer text takes the retry)
        got, lines, ids = C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def launch(cap):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            check(L.dgrp_rmout_text_batch(blob, off.ctypes.data, len(raw), int(by_contig), cblob, coff.ctypes.data, len(pairs), _ptr(d_rows),
                                          _ptr(d_scores), nrows, int(min_score), len(ends), ends.ctypes.data, int(join_gap), int(id0),
                                          _ptr(text), cap, C.byref(got), C.byref(lines), C.byref(ids), _ptr(work), wb, stream_ptr()),
                  "dgrp_rmout_text_batch")
            return text, (int(got.value),)
        return _with_room(launch, cap)[:got.value], int(lines.value), int(ids.value)

    def rmout_write(self, d_probs: torch.Tensor, row0, lengths, startposes, rows: np.ndarray, row_off, names, by_contig: bool, plan):
        """One write of a RepeatMasker listing (rmout.RmoutWrite) for the arguments of bed_write: the scores are summed now and stay
        on the device with the rows; the text and, with plan.gzip_level, its BGZF members are made when bed.BedFiles renders the write
        with the IDs used in front of it (they run through the file), on the stream that is current then."""
        from .rmout import RmoutText, RmoutWrite
        raw = name_blob(names)[0]
        r0, ln, sp, _cl = ContigPipeline._track_tables(d_probs, "rmout_write", row0, lengths, startposes)
        ends = sp + ln
        rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
        ro = np.ascontiguousarray(row_off, np.int64)
        if len(rows) == 0:
            return RmoutWrite(raw)
        if len(ro) != len(ln) + 1 or int(ro[0]) != 0 or int(ro[-1]) != len(rows):
            raise ValueError("rmout_write: the row offsets must cover all rows")
        if plan.rmout_pairs is None:
            raise ValueError("rmout_write: the plan has no names for the labels (bed.from_plan settles them)")
        d_rows, d_scores = self._row_scores_device(d_probs, r0, ln, sp, rows, ro)
        made = torch.cuda.Event()
        made.record()

        def render(id0: int) -> RmoutText:
            from .gz import bgzf_members_device
            made.wait()                                     # (the renderer's stream may be another one than the scores')
            d_text, lines, ids = self.rmout_text_batch(raw, by_contig, d_rows, d_scores, plan.min_score, ends, plan.rmout_pairs,
                                                       plan.rmout_join, id0)
            if plan.gzip_level is None:
                return RmoutText(d_text.cpu().numpy().tobytes(), lines, ids)
            return RmoutText(bgzf_members_device(d_text, plan.gzip_level), lines, ids)
        return RmoutWrite(raw, render)

    # predict --bed_bigbed: the rows as bigBed item blocks and coverage zoom records
    @staticmethod
    def _bed_rows(who: str, d_rows: torch.Tensor, d_scores: torch.Tensor, rec_end):
        nrows = int(d_rows.numel()) // SEGMENT_DTYPE.itemsize
        if int(d_scores.numel()) != nrows * ROW_SCORE_DTYPE.itemsize:
            raise ValueError(f"{who}: {nrows} rows but {int(d_scores.numel())} bytes of scores")
        return nrows, np.ascontiguousarray(rec_end, np.int64)

    @staticmethod
    def bed_blocks_batch(by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int, rec_end, chrom0: int = 0):
        """The emitted rows of `d_rows` / `d_scores` (as bed_text_batch takes them) as uncompressed bigBed item blocks, one
        dgrp_bed_blocks_batch call: -> (uint8 device tensor of the blocks back to back, uint8 device tensor of the block table, rows
        of bigbed.BLOCK_DTYPE, the number of items).  Record r (a row's contig with by_contig, else 0) ends at rec_end[r] and has
        chromId chrom0 + r.  What bigbed.reference_blocks states; complete behind the call on the current stream."""
        from .bigbed import BLOCK_DTYPE, BLOCK_ITEMS
        L = lib()
        nrows, ends = ContigPipeline._bed_rows("bed_blocks_batch", d_rows, d_scores, rec_end)
        nrec, dev = len(ends), d_rows.device
        wb = int(L.dgrp_bed_blocks_workspace_bytes(nrows, nrec, ends.ctypes.data))
        if wb <= 0:
            raise ValueError(f"bed_blocks_batch: bad row count {nrows}, record count {nrec} or record ends (above 2^32 - 1?)")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        got, nblk, items = C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def launch(cap, tcap):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            table = torch.empty(max(tcap, 1) * BLOCK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            check(L.dgrp_bed_blocks_batch(int(by_contig), _ptr(d_rows), _ptr(d_scores), nrows, int(min_score), nrec, ends.ctypes.data,
                                          int(chrom0), _ptr(out), cap, C.byref(got), _ptr(table), tcap, C.byref(nblk), C.byref(items),
                                          _ptr(work), wb, stream_ptr()), "dgrp_bed_blocks_batch")
            return (out, table), (int(got.value), int(nblk.value))
        out, table = _with_room(launch, 48 * nrows, nrows // BLOCK_ITEMS + nrec)     # (an item of predict is 42..46 bytes: the guess fits)
        return out[:got.value], table[:nblk.value * BLOCK_DTYPE.itemsize], int(items.value)

    @staticmethod
    def bed_zoom_batch(by_contig: bool, d_rows: torch.Tensor, d_scores: torch.Tensor, min_score: int, rec_end, chrom0: int = 0):
        """The coverage zoom records of the same arguments, one dgrp_bed_zoom_batch call: -> (uint8 device tensor of the 32-byte
        records; record offsets [bigwig.ZOOM_LEVELS + 1]; uint8 device tensor of the block table, rows of bigwig.ZOOM_BLOCK_DTYPE;
        block offsets; totals, bigwig.TOTALS_DTYPE [1]).  What bigbed.reference_zoom and reference_totals state."""
        from .bigwig import TOTALS_DTYPE, ZOOM_BLOCK_DTYPE, ZOOM_LEVELS
        L = lib()
        nrows, ends = ContigPipeline._bed_rows("bed_zoom_batch", d_rows, d_scores, rec_end)
        nrec, dev = len(ends), d_rows.device
        wb = int(L.dgrp_bed_zoom_workspace_bytes(nrows, nrec, ends.ctypes.data))
        if wb <= 0:
            raise ValueError(f"bed_zoom_batch: bad row count {nrows}, record count {nrec} or record ends (above 2^32 - 1?)")
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        roff, boff = np.zeros(ZOOM_LEVELS + 1, np.int64), np.zeros(ZOOM_LEVELS + 1, np.int64)
        totals = np.zeros(1, TOTALS_DTYPE)
        nwin = int(((ends - 1) // 1024 + 1).sum())
        cap = 32 * (min(2 * nrows, 2 * nwin) + ZOOM_LEVELS * nrec + 64)               # (a short row covers one window a level)

        def launch(cap, tcap):
            out = torch.empty(max(cap, 32), dtype=torch.uint8, device=dev)
            table = torch.empty(max(tcap, 1) * ZOOM_BLOCK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            check(L.dgrp_bed_zoom_batch(int(by_contig), _ptr(d_rows), _ptr(d_scores), nrows, int(min_score), nrec, ends.ctypes.data,
                                        int(chrom0), _ptr(out), cap, roff.ctypes.data, _ptr(table), tcap, boff.ctypes.data,
                                        totals.ctypes.data, _ptr(work), wb, stream_ptr()), "dgrp_bed_zoom_batch")
            return (out, table), (32 * int(roff[ZOOM_LEVELS]), int(boff[ZOOM_LEVELS]))
        out, table = _with_room(launch, cap, cap // (32 * 1024) + ZOOM_LEVELS)
        return out[:32 * int(roff[ZOOM_LEVELS])], roff, table[:int(boff[ZOOM_LEVELS]) * ZOOM_BLOCK_DTYPE.itemsize], boff, totals

    def bigbed_write(self, d_probs: torch.Tensor, row0, lengths, startposes, rows: np.ndarray, row_off, names, by_contig: bool, plan,
                     chrom0: int = 0):
        """One write of a bigBed (bigbed.BigBedWrite) for the arguments of bed_write: scores -> item blocks -> zoom records on the
        device from the uploaded rows, both deflated there (zlib_compress_device, plan.gzip_level); only compressed bytes, tables
        and totals come back.  chrom0 is the ordinal of the first record in its input: chromIds count from there."""
        from . import bigbed as bb
        from .bigwig import ZOOM_BLOCK_DTYPE
        from .tracks import _zlib_pieces
        raw = name_blob(names)[0]
        r0, ln, sp, _cl = ContigPipeline._track_tables(d_probs, "bigbed_write", row0, lengths, startposes)
        ends = sp + ln
        sizes = [int(e) for e in ends]
        refused = bb.end_refusal(raw, sizes)
        rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
        ro = np.ascontiguousarray(row_off, np.int64)
        if refused is not None or len(rows) == 0:
            return bb.BigBedWrite(raw, sizes, refused, chrom0=chrom0)
        if len(ro) != len(ln) + 1 or int(ro[0]) != 0 or int(ro[-1]) != len(rows):
            raise ValueError("bigbed_write: the row offsets must cover all rows")
        level = 1 if plan.gzip_level is None else plan.gzip_level
        d_rows, d_scores = self._row_scores_device(d_probs, r0, ln, sp, rows, ro)
        del d_probs
        d_out, d_tab, _items = self.bed_blocks_batch(by_contig, d_rows, d_scores, plan.min_score, ends, chrom0)
        blob, bsizes = _zlib_pieces(self, d_out, d_tab, bb.BLOCK_DTYPE.itemsize, level)
        table = d_tab.cpu().numpy().view(bb.BLOCK_DTYPE)
        del d_out, d_tab
        d_zoom, _roff, d_ztab, _boff, totals = self.bed_zoom_batch(by_contig, d_rows, d_scores, plan.min_score, ends, chrom0)
        zblob, zsizes = _zlib_pieces(self, d_zoom, d_ztab, ZOOM_BLOCK_DTYPE.itemsize, level)
        ztable = d_ztab.cpu().numpy().view(ZOOM_BLOCK_DTYPE)
        return bb.BigBedWrite(raw, sizes, None, blob, bsizes, table, zblob, zsizes, ztable, tuple(int(x) for x in totals[0]), chrom0)

    @staticmethod
    def batch_row_offsets(rows: np.ndarray, contigs) -> np.ndarray:
        """row_scores_batch's row_off for the rows of a run_batch call: they come back in record order, so record r's rows are the
        running count of rows["contig"] -- for which `contigs` must ascend with the records."""
        cg = np.ascontiguousarray(contigs, np.int64)
        if not (np.diff(cg) > 0).all():
            raise ValueError("batch_row_offsets: contigs must ascend with the records")
        return np.searchsorted(rows["contig"], np.r_[cg, cg[-1] + 1], side="left").astype(np.int64)

    def row_scores(self, merged: torch.Tensor, startpos: int, rows: np.ndarray) -> np.ndarray:
        """The scores of one record's segment rows against its merged probabilities (ContigPipeline.merged): row i of `merged` has
        coordinate startpos + i."""
        if len(rows) == 0 or len(merged) == 0:
            return np.zeros(len(rows), ROW_SCORE_DTYPE)
        return self.row_scores_batch(merged, [0], [len(merged)], [startpos], rows, [0, len(rows)])

    def run_batch_probs(self, d_base: torch.Tensor, offsets, lengths, startposes, contigs):
        """run_batch that keeps the merged probabilities: one dgrp_predict_batch_probs call.  -> (rows, d_probs, row0): the
        probabilities [dgrp_batch_rows, C] stay on the device for batch_track_texts and row_scores_batch (its row_off:
        batch_row_offsets); record r starts at row row0[r]."""
        ln = np.ascontiguousarray(lengths, np.int64)
        nrec = len(ln)
        row0 = np.zeros(nrec, np.int64)
        if nrec == 0:
            return np.zeros(0, SEGMENT_DTYPE), None, row0
        np.cumsum((ln[:-1] + 63) // 64 * 64, out=row0[1:])
        total = int(lib().dgrp_batch_rows(nrec, ln.ctypes.data))
        d_probs = torch.empty((total, self.model.classes), dtype=torch.float32, device=d_base.device)
        return self.run_batch(d_base, offsets, lengths, startposes, contigs, d_probs=d_probs), d_probs, row0

    def run(self, sequence, contig: int = 0) -> np.ndarray:
        startpos, d_idx = record_indices(sequence)
        return self.run_idx(d_idx, startpos, contig)
