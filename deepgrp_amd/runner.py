"""How the command line pushes records through the device pipeline: independent records (deepgrp/__main__.py:280-292)
run on a small pool of host threads, one HIP stream each, with ordered results; consecutive short records of one
ingest buffer go to the GPU as one batch.  `RecordRunner.outputs` yields what the reference's loop would have produced
record after record -- the rows and, where asked for, the track texts (predict --track_dir) and the rows' scores (--bed_dir)
from the same forward pass -- and raises where that loop would raise; `results` is its rows alone.  Every mode takes the
same path: `work_items` groups, `run_item` runs a record or a batch, `in_order` keeps the order."""
from __future__ import annotations

import collections
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, Iterator, List, NamedTuple, Tuple

import numpy as np
import torch

from .fasta import DeviceRecord
from .pipeline import ContigPipeline, record_indices


class _One(NamedTuple):
    """A work item: one record, the name of its track and BED lines (None where neither is made), its ordinal in its input (the
    chromId of --track_bigwig and --bed_bigbed)."""
    name: object
    rec: object
    chrom: int
    key: object = None            # the record's key, for a runner with a probe


class _Batch(list):
    """A batch work item: [(key, record), ...]; chrom0: the ordinal of its first record in its input."""

    def __init__(self, pairs, chrom0: int):
        super().__init__(pairs)
        self.chrom0 = chrom0


_BATCH = object()             # key slot of a work item that is a batch of records (never equal to a user's key, e.g. a header "batch")
SMALL_RECORD = 1 << 18        # bases: up to here a record may join a batch
BATCH_RECORDS = 4096
BATCH_BYTES = 4 << 30         # workspace a batch may ask for


_STREAMS: dict = {}
_STREAMS_LOCK = threading.Lock()


def _worker_stream(dev: int, i: int):
    """Stream of worker i on device dev, the same object for every runner of the process: torch's allocator caches blocks per
    stream, so a fresh stream per run would leave the previous run's workspaces (14 GB for a 250 Mbp record) reserved for good."""
    with _STREAMS_LOCK:
        pool = _STREAMS.setdefault(dev, [])
        while len(pool) <= i:
            pool.append(torch.cuda.Stream(device=dev))
        return pool[i]


def _no_stage(*_a) -> None:
    """run_record's stage callback where none was given: nothing is timed, nothing waits for the device."""


def _format(prefixes: List[bytes], by_contig: bool, rows) -> str:
    """dgrp_format_rows (host code of the library): one pass over the row records, no per-row Python objects."""
    import ctypes as C

    from ._lib import check, lib, name_blob
    from .pipeline import SEGMENT_DTYPE
    L = lib()
    rows = np.ascontiguousarray(rows, dtype=SEGMENT_DTYPE)
    blob, off = name_blob(prefixes)[1:]
    cap = L.dgrp_format_rows_bound(len(rows), max(len(p) for p in prefixes))
    out = np.empty(cap, np.uint8)
    written = C.c_int64()
    check(L.dgrp_format_rows(blob, off.ctypes.data, len(prefixes), int(by_contig), rows.ctypes.data, len(rows), out.ctypes.data, cap,
                             C.byref(written)), "dgrp_format_rows")
    return out[:written.value].tobytes().decode("utf-8", "surrogateescape")


def rows_text(filename: str, header: str, rows) -> str:
    """The TSV rows of one record (__main__.py:291-292)."""
    if len(rows) == 0:
        return ""
    return _format(["{}\t{}\t".format(filename, header).encode("utf-8", "surrogateescape")], False, rows)


def rows_text_batch(filename: str, headers, rows) -> str:
    """The rows of a batch of records (rows["contig"] = index into `headers`), record order = row order."""
    if len(rows) == 0:
        return ""
    return _format(["{}\t{}\t".format(filename, h).encode("utf-8", "surrogateescape") for h in headers], True, rows)


class RecordRunner:
    """Runs (key, record) pairs -- record = DeviceRecord or sequence text -- and yields results in input order (`outputs`,
    `results`).  tracks (a tracks.TrackSpec): every record's track texts come with its rows; scores: the rows' scores
    (pipeline.ROW_SCORE_DTYPE, predict --bed_dir) do -- with bed (a bed.BedPlan with a gzip_level, --bed_gzip) the write's
    bed.BedWrite instead, made on the device where rows and scores then stay, and with a bigBed plan (--bed_bigbed) its
    bigbed.BigBedWrite, chromIds counted by the record's ordinal in its input, and with a GFF3 plan (--bed_gff3, gzip or not) its
    gff.GffWrite, which bed.BedFiles renders in file order.  With either, every key is (header, name), name
    the first column of the record's track and BED lines (evaluation.record_name), and rows, scores and texts come from one merged
    array; with neither, keys are arbitrary and a record is one fused call (dgrp_predict_record, dgrp_predict_batch).
    probe (a callable): called on the worker's stream while the merged array of a work item is alive, probe(d_probs, row0, lengths,
    startposes, keys) -- record r is rows [row0[r], row0[r] + lengths[r]) of d_probs (None for a record without a base) -- and what it
    returns travels with the item's result as one more field; it forces the merged path, as tracks and scores do."""

    def __init__(self, pipe: ContigPipeline, workers: int = 0, max_bases: int = 1 << 29, tracks=None, scores: bool = False, bed=None,
                 probe=None):
        self.pipe = pipe
        self.tracks, self.scores, self.probe = tracks, bool(scores), probe
        # --bed_gzip, --bed_gff3: a bed.BedWrite or gff.GffWrite in the scores' place
        self.bed = bed if bed is not None and bed.on_device else None
        self.workers = workers or int(os.environ.get("DGRP_CLI_WORKERS", "16"))
        self.max_bases = max_bases
        m = pipe.model
        self._T, self._UP = m.vecsize, (m.units + 31) // 32 * 32

    # ---- one work item -> (rows, scores or None, texts or None), with a probe also what it returned
    def _fused(self) -> bool:
        return self.tracks is None and not self.scores and self.probe is None

    def run_record(self, rec, name=None, chrom: int = 0, key=None, stage=None):
        """One record: the fused call, or merged -> [the texts of self.tracks] -> [the probe] -> labels -> segments -> [the rows'
        scores], because the fused call keeps its merged array inside its workspace.  stage (a callable, predict -vv): the record
        takes the second form whatever was asked for, and stage(what, done) is called in front of (done False) and behind (done
        True) "encode", "forward", "tracks", "labels", "segments" and "scores" -- "tracks" and "scores" only where the runner makes
        them, and behind "encode" with the record's bases as a third argument; a record without a base ends there."""
        if stage is None and self._fused():
            if isinstance(rec, DeviceRecord):             # parsed and encoded on the GPU
                startpos, d_idx = record_indices(rec)
                return self.pipe.run_idx(d_idx, startpos), None, None
            return self.pipe.run(rec), None, None
        from .pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE
        from .tracks import empty_texts, record_texts
        stage = stage or _no_stage
        stage("encode", False)
        startpos, d_idx = record_indices(rec)
        stage("encode", True, int(d_idx.numel()))
        if d_idx.numel() == 0:                            # no base: no rows; with --track_bigwig still a chromosome (empty_texts)
            scores = np.zeros(0, ROW_SCORE_DTYPE) if self.scores else None
            if self.scores and self.bed is not None:
                from .bed import empty_write
                scores = empty_write(self.bed, name, startpos, chrom)
            out = (np.zeros(0, SEGMENT_DTYPE), scores, empty_texts(self.tracks, name, startpos) if self.tracks is not None else None)
            return out if self.probe is None else out + (self.probe(None, [0], [0], [startpos], [key]),)
        stage("forward", False)
        merged = self.pipe.merged(d_idx)
        stage("forward", True)
        texts = None
        if self.tracks is not None:
            stage("tracks", False)
            texts = record_texts(self.pipe, merged, startpos, name, self.tracks, chrom)
            stage("tracks", True)
        probed = self.probe(merged, [0], [len(merged)], [startpos], [key]) if self.probe is not None else None
        stage("labels", False)
        labels = self.pipe.labels(merged)
        stage("labels", True)
        stage("segments", False)
        rows = self.pipe.segments(labels, startpos)
        del labels
        stage("segments", True)
        scores = None
        if self.scores:
            stage("scores", False)
            if self.bed is not None:
                scores = self.pipe.bed_write(merged, [0], [len(merged)], [startpos], rows, [0, len(rows)], [name], False, self.bed, chrom)
            else:
                scores = self.pipe.row_scores(merged, startpos, rows)
            stage("scores", True)
        return (rows, scores, texts) if self.probe is None else (rows, scores, texts, probed)

    def run_batch(self, batch: _Batch):
        """A batch: rows of all its records, contig = position in the batch; scores go row by row with them, texts[k] is the text of
        class self.tracks.classes[k] of all its records in order."""
        recs = [r for _k, r in batch]
        args = (recs[0].base, [r.offset for r in recs], [r.length for r in recs], [r.startpos for r in recs], list(range(len(recs))))
        if self._fused():
            return self.pipe.run_batch(*args), None, None
        rows, d_probs, row0 = self.pipe.run_batch_probs(*args)
        ln = np.ascontiguousarray(args[2], np.int64)
        probed = self.probe(d_probs, row0, ln, args[3], [k for k, _r in batch]) if self.probe is not None else None
        scores = texts = None
        if self.scores and self.bed is not None:
            scores = self.pipe.bed_write(d_probs, row0, ln, args[3], rows, self.pipe.batch_row_offsets(rows, args[4]),
                                         [k[1] for k, _r in batch], True, self.bed, batch.chrom0)
        elif self.scores:
            scores = self.pipe.row_scores_batch(d_probs, row0, ln, args[3], rows, self.pipe.batch_row_offsets(rows, args[4]))
        if self.tracks is not None:
            texts = self.pipe.batch_track_texts(d_probs, row0, ln, args[3], [k[1] for k, _r in batch], self.tracks,
                                                batch.chrom0 if self.tracks.bigwig else 0)
        return (rows, scores, texts) if self.probe is None else (rows, scores, texts, probed)

    def run_item(self, item):
        if isinstance(item, _Batch):
            return self.run_batch(item)
        if self.probe is None:
            return self.run_record(item.rec, item.name, item.chrom)
        return self.run_record(item.rec, item.name, item.chrom, item.key)

    # ---- batching
    def _batch_cost(self, n: int) -> int:
        """Workspace bytes a record of n bases adds to a batch (attention: the avg[t] spill of its windows dominates).  With
        tracks: the merged copy, 4 bytes per bin and class, and the text guess (a line of 12 bytes and a short name per bin)."""
        cost = 80 * n
        m = self.pipe.model
        if self.tracks is not None:
            cost += 4 * m.classes * (n + 64) + len(self.tracks.classes) * (n // self.tracks.bin + 2) * (4 + 12 + 32)
        if m.attention:
            cost += len(range(0, n - self._T, self.pipe.step)) * self._T * (self._UP * 4 + m.classes * 4)
        return cost

    def work_items(self, records: Iterable[Tuple[object, object]]) -> Iterator[Tuple[object, object]]:
        """Consecutive short records of one ingest buffer become one (_BATCH, [(key, record), ...]) item, everything
        else stays (key, record)."""
        group: List[Tuple[object, DeviceRecord]] = []
        cost = 0
        batchable = self.pipe.batchable()
        for key, rec in records:
            small = batchable and isinstance(rec, DeviceRecord) and rec.base is not None and 1 <= rec.length <= SMALL_RECORD
            if small:
                c = self._batch_cost(rec.length)
                if group and (group[0][1].base is not rec.base or len(group) >= BATCH_RECORDS or cost + c > BATCH_BYTES):
                    yield _BATCH, group
                    group, cost = [], 0
                group.append((key, rec))
                cost += c
            else:
                if group:
                    yield _BATCH, group
                    group, cost = [], 0
                yield key, rec
        if group:
            yield _BATCH, group

    # ---- ordered execution
    @staticmethod
    def _size(item) -> int:
        if isinstance(item, _Batch):
            return sum(r.length for _k, r in item)
        return item.rec.d_idx.numel() if isinstance(item.rec, DeviceRecord) else len(item.rec)

    def in_order(self, items: Iterable[Tuple[object, object]]) -> Iterator[Tuple[object, object]]:
        """`run_item` for every (key, item) on the pool; yields (key, result) in input order.  While one record is in
        its post-processing (whose fixed-point loop waits on its stream) the next ones are already on the GPU.  The
        bases in flight are bounded; an exception surfaces where the sequential loop would raise it."""
        dev = torch.cuda.current_device() if torch.cuda.is_available() else None
        local = threading.local()
        taken = iter(range(self.workers))

        def task(item):
            if dev is None:
                return self.run_item(item)
            if not hasattr(local, "stream"):
                torch.cuda.set_device(dev)
                local.stream = _worker_stream(dev, next(taken))
            with torch.cuda.stream(local.stream):
                out = self.run_item(item)
                local.stream.synchronize()
            return out

        pending: "collections.deque" = collections.deque()
        inflight = 0
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            for key, item in items:
                w = self._size(item)
                while pending and (inflight + w > self.max_bases or len(pending) >= 4 * self.workers):
                    k0, f0, w0 = pending.popleft()
                    yield k0, f0.result()
                    inflight -= w0
                pending.append((key, pool.submit(task, item), w))
                inflight += w
                del item
            while pending:
                k0, f0, _w0 = pending.popleft()
                yield k0, f0.result()

    def outputs(self, records: Iterable[Tuple[object, object]]):
        """("one", key, rows, scores, texts) for a record on its own, ("batch", [keys], rows, scores, texts) for a batch of short
        records (rows["contig"] indexes the keys); scores and texts are None where the runner was not asked for them; with a probe a
        sixth field holds what it returned for the item.  Records batch the same way whatever is asked for."""
        def items():
            chrom = 0                                     # records of this input so far
            for key, item in self.work_items(records):
                if key is _BATCH:
                    yield ("batch", [k for k, _r in item]), _Batch(item, chrom)
                    chrom += len(item)
                else:
                    yield ("one", key), _One(key[1] if self.tracks is not None or self.scores else None, item, chrom, key)
                    chrom += 1
        for head, result in self.in_order(items()):
            yield head + result

    def results(self, records: Iterable[Tuple[object, object]]):
        """`outputs` without scores and texts: ("one", key, rows) and ("batch", [keys], rows)."""
        for out in self.outputs(records):
            yield out[:3]
