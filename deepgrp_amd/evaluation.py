"""`evaluate`: how well a model finds the repeats of an annotation -- per-class precision, recall, F1 and MCC on the bases `predict`
labels, the measure of the DeepGRP paper and of the reference's model selection (deepgrp/optimization.py:52-69 scores the MSS labels
of a held-out chromosome with calculate_metrics against the truth of preprocess_y), plus element-level counts.

Per record, the evaluated bases are those `predict` labels: from the first to the last non-N base (DeviceRecord's startpos and
kept length).  The prediction of a base is the label of the TSV row `predict` writes over it (0 where none does); its truth is
the smallest kept repeat number among the annotation rows that cover it (0 where none does), which is
preprocess_y(...).argmax(axis=0).  Two deliberate differences from the reference's objective: its drop_start_end_n also drops the
last non-N base, and it runs filter_segments over the labels once more; here the TSV users get is measured as it is.

Both label tracks are painted on the GPU from their rows (dgrp_paint_rows_batch) into flat buffers of the work item's records,
scored by dgrp_confusion_matrix, and every row is counted against the other track (dgrp_row_hits_batch).

REPORTS.  Everything further that `evaluate` can count (--curves, --strata, --offtarget, --boundaries) is a report: an object of a
module of its own that this one never imports.  `Accumulator.add` fills one `WorkItem` per work item -- the tables, both sides' rows
on the host and on the device, their clipped lengths, hits and masks, the two label tracks -- and hands it to every report.  A
report has
    key                      its key in the JSON content
    bind(annotation, classes)  the checks against the model's classes and the annotation, made before the first record runs; it
                             keeps what it needs of the annotation and looks its per-record inputs up by the item's record names
    probe(probe_item)        optional: its share of `Accumulator.probe`, which the runner calls on the worker's stream while the
                             merged probabilities of a work item are alive (`ProbeItem`) -> what `add` gets as `probed`
    add(item, probed)        its share of a work item with at least one base, on the current stream
    summary()                the value under `key`
    write(plan, log)         its files
The helpers the reports share with the core stand beside the two item classes: `tables`, `upload`, `paint`, `count`, `naming`."""
from __future__ import annotations

import logging
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .pipeline import SEGMENT_DTYPE

_LOG = logging.getLogger(__name__)

TSV_COLUMNS = ("class", "true_bases", "predicted_bases", "TP", "FP", "FN", "TPR", "PPV", "F1", "elements", "found", "segments",
               "supported")


class AnnotationError(ValueError):
    """A row of the annotation table that cannot be read."""


class NoMatchError(ValueError):
    """Not one annotation row names a record of the inputs (the usual cause: `chr1` against `1`)."""


def _bad(path, lineno: int, line: str, why: str):
    return AnnotationError(f"{path}:{lineno}: {why}: {line.rstrip()!r}")


def read_annotation(path, repeats: Optional[Iterable[int]] = None) -> Dict[str, np.ndarray]:
    """The rows of a `parse_rm` table (whitespace separated: contig, 0-based begin, exclusive end, repeat number, further columns
    ignored; blank lines and lines starting with '#' skipped) as {contig: SEGMENT_DTYPE rows} with label = repeat number, in file
    order.  Rows whose number is not in `repeats` are dropped (None keeps every row).  A negative begin or end, an end below its
    begin or a column 2-4 that is not an integer raises AnnotationError naming the file and the line."""
    with open(path, "r", errors="surrogateescape") as fh:
        lines = fh.read().splitlines()
    recs: List[List[str]] = []
    linenos: List[int] = []
    for k, line in enumerate(lines):
        f = line.split(None, 4)
        if not f or f[0][0] == "#":
            continue
        if len(f) < 4:
            raise _bad(path, k + 1, line, "expected contig, begin, end and repeat number")
        recs.append(f)
        linenos.append(k + 1)
    n = len(recs)
    names = [f[0] for f in recs]
    tokens = [t for f in recs for t in f[1:4]]
    try:
        vals = np.fromiter(map(int, tokens), np.int64, count=3 * n).reshape(n, 3).T
    except (ValueError, OverflowError):
        for k, t in enumerate(tokens):                           # the first line at fault
            try:
                np.int64(int(t))
            except (ValueError, OverflowError):
                ln = linenos[k // 3]
                raise _bad(path, ln, lines[ln - 1], f"{('begin', 'end', 'repeat number')[k % 3]} {t!r} is not an integer") from None
        raise
    begin, end, number = vals
    bad = np.flatnonzero((begin < 0) | (end < begin))
    if bad.size:
        k = int(bad[0])
        raise _bad(path, linenos[k], lines[linenos[k] - 1], "negative begin" if begin[k] < 0 else "end below begin")
    keep = np.ones(n, bool) if repeats is None else np.isin(number, np.array(sorted(set(int(r) for r in repeats)), np.int64))
    out: Dict[str, np.ndarray] = {}
    idx = np.flatnonzero(keep)
    if idx.size == 0:
        return out
    uniq, inv = np.unique(np.array(names)[idx], return_inverse=True)
    order = np.argsort(inv, kind="stable")
    for u, part in zip(uniq, np.split(order, np.cumsum(np.bincount(inv, minlength=len(uniq)))[:-1])):
        sel = idx[part]
        rows = np.zeros(sel.size, SEGMENT_DTYPE)
        rows["start"], rows["end"], rows["label"] = begin[sel], end[sel], number[sel]
        out[str(u)] = rows
    return out


def clipped_lengths(rows: np.ndarray, origin: int, length: int) -> np.ndarray:
    """Bases of each row inside the evaluated span [origin, origin + length)."""
    a = np.clip(rows["start"].astype(np.int64), origin, origin + length)
    e = np.clip(rows["end"].astype(np.int64), origin, origin + length)
    return np.maximum(e - a, 0)


def tables(origins: Sequence[int], lengths: Sequence[int]):
    """Records back to back in one flat buffer: -> (lengths, origins, offsets [nrec + 1]) as the library reads them."""
    ln = np.ascontiguousarray(lengths, np.int64)
    org = np.ascontiguousarray(origins, np.int64)
    off = np.zeros(len(ln) + 1, np.int64)
    np.cumsum(ln, out=off[1:])
    return ln, org, off


def upload(rows: Sequence[np.ndarray], dev):
    """The rows of the records as one device array: -> (row offsets [nrec + 1], the rows on the host, on the device or None)."""
    import torch
    ro = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=ro[1:])
    flat = np.concatenate(rows) if ro[-1] else np.zeros(0, SEGMENT_DTYPE)
    d = torch.from_numpy(flat.view(np.uint8)).to(dev) if flat.size else None
    return ro, flat, d


def paint(ln: np.ndarray, org: np.ndarray, off: np.ndarray, ro: np.ndarray, d_rows, work, dev):
    """A zeroed label track of the records with the rows painted on it, on the current stream (dgrp_paint_rows_batch)."""
    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    d_labels = torch.zeros(int(off[-1]), dtype=torch.int8, device=dev)
    check(lib().dgrp_paint_rows_batch(d_labels.data_ptr(), len(ln), off.ctypes.data, ln.ctypes.data, org.ctypes.data,
                                      None if d_rows is None else d_rows.data_ptr(), ro.ctypes.data, work.data_ptr(), work.numel(),
                                      stream_ptr()), "dgrp_paint_rows_batch")
    return d_labels


def count(theta: float, labels: np.ndarray, clen: np.ndarray, hits: np.ndarray, total: np.ndarray, good: np.ndarray):
    """total[label] += 1 per row with a base inside its record, good[label] += 1 per such row with hits >= theta * its clipped
    length; -> the two masks."""
    ok = clen > 0
    np.add.at(total, labels[ok], 1)
    hit = ok & (hits.astype(np.float64) >= theta * clen.astype(np.float64))
    np.add.at(good, labels[hit], 1)
    return ok, hit


def naming(names: Sequence[str]) -> str:
    """`record 'a'` or `records 'a', 'b', ...` (the first five) for an error that names a work item."""
    return "record{} {}".format("s" if len(names) > 1 else "", ", ".join(repr(x) for x in list(names)[:5]) + (", ..." if len(names) > 5 else ""))


class WorkItem:
    """What `Accumulator.add` knows of one work item with at least one base, for the reports to read.
    C, theta: the classes and --min_overlap.  names: the records' names.  ln, org, off: `tables`; n = off[-1] bases in nrec records.
    Annotation side: tr the rows record by record, t_off, t_flat, d_trows: `upload` of them; t_clen their clipped lengths, ht their
    hits against the predicted labels, ok, hit: the masks of `count` (a base inside the record; found).
    Predicted side: pr, p_off, p_flat, d_prows, p_clen, hp (hits against the truth), kept, good likewise; scores: the rows' scores
    (pipeline.ROW_SCORE_DTYPE) or None.
    d_true, d_pred: the two int8 label tracks.  dev, stream: the device and the pointer of the stream everything was queued on."""
    __slots__ = ("C", "theta", "names", "ln", "org", "off", "n", "nrec", "tr", "t_off", "t_flat", "d_trows", "t_clen", "ht", "ok", "hit",
                 "pr", "p_off", "p_flat", "d_prows", "p_clen", "hp", "kept", "good", "scores", "d_true", "d_pred", "dev", "stream")


class ProbeItem:
    """What `Accumulator.probe` knows of one work item with at least one base.  d_probs: the merged probabilities, float32
    [rows, C]; record r is its rows [row0[r], row0[r] + ln[r]).  ln, org, off, nrec, names as in WorkItem.  tr, t_off, d_trows: the
    item's annotation rows record by record and `upload` of them.  dev: the device."""
    __slots__ = ("C", "d_probs", "row0", "ln", "org", "off", "nrec", "names", "tr", "t_off", "d_trows", "dev")


class Accumulator:
    """Integer sums over work items: the C x C confusion matrix (cnf[truth][pred]) and the element counts; `reports` (see the
    module's REPORTS) take their share of every item."""

    def __init__(self, classes: int, min_overlap: float, reports=()):
        if not 0.0 < min_overlap <= 1.0:
            raise ValueError(f"min_overlap must lie in (0, 1], not {min_overlap}")
        self.C, self.theta = int(classes), float(min_overlap)
        self.reports = list(reports)
        self.cnf = np.zeros((self.C, self.C), np.int64)
        self.elements = np.zeros(self.C, np.int64)
        self.found = np.zeros(self.C, np.int64)
        self.segments = np.zeros(self.C, np.int64)
        self.supported = np.zeros(self.C, np.int64)
        self.bases = self.records = self.records_annotated = self.rows_used = self.outside = 0

    def probe(self, annotation: Dict[str, np.ndarray]):
        """RecordRunner's probe, or None when no report has one: called on the worker's stream with the merged probabilities of a
        work item (record r: rows [row0[r], row0[r] + lengths[r]) of d_probs; keys[r][1] its annotation contig), it uploads the
        item's truth rows and returns {key: what the report's probe returned} as host arrays -- None for an item without a base;
        `add` hands every report its own."""
        asked = [r for r in self.reports if hasattr(r, "probe")][::-1]       # (the last report's device calls are queued first)
        if not asked:
            return None
        empty = np.zeros(0, SEGMENT_DTYPE)

        def run(d_probs, row0, lengths, startposes, keys):
            import torch

            from .pipeline import require_gpu
            it = ProbeItem()
            it.ln, it.org, it.off = tables(startposes, lengths)
            it.nrec = len(it.ln)
            if it.nrec == 0 or int(it.off[-1]) == 0 or d_probs is None:
                return {r.key: None for r in asked}
            if d_probs.dtype != torch.float32 or d_probs.ndim != 2 or not d_probs.is_contiguous() or d_probs.shape[1] != self.C:
                raise ValueError(f"the {asked[0].key} take a contiguous float32 [rows, {self.C}] array")
            it.C, it.d_probs, it.row0, it.dev = self.C, d_probs, np.ascontiguousarray(row0, np.int64), require_gpu()
            it.names = [k[1] for k in keys]
            it.tr = [np.ascontiguousarray(annotation.get(nm, empty), SEGMENT_DTYPE) for nm in it.names]
            it.t_off, _flat, it.d_trows = upload(it.tr, it.dev)
            return {r.key: r.probe(it) for r in asked}
        return run

    def add(self, origins: Sequence[int], lengths: Sequence[int], pred_rows: Sequence[np.ndarray],
            true_rows: Sequence[np.ndarray], scores: Optional[np.ndarray] = None, probed=None, names: Sequence[str] = ()) -> None:
        """One work item: records r = 0.. with startpos origins[r], kept length lengths[r], the TSV rows `predict` wrote for it
        (original coordinates) and its kept annotation rows.  For the reports also the scores of the predicted rows, record after
        record (pipeline.ROW_SCORE_DTYPE), what `probe` returned for the item, and the records' names."""
        import torch

        from ._lib import check, lib
        from .pipeline import require_gpu, stream_ptr
        L = lib()
        it = WorkItem()
        it.C, it.theta, it.names, it.scores = self.C, self.theta, list(names), scores
        it.nrec = nrec = len(lengths)
        if nrec == 0:
            return
        if self.reports and len(it.names) != nrec:
            raise ValueError(f"{nrec} records but {len(it.names)} names: the reports look their inputs up by record name")
        it.ln, it.org, it.off = ln, org, off = tables(origins, lengths)
        it.n = n = int(off[-1])
        self.records += nrec
        self.bases += n
        self.records_annotated += sum(1 for t in true_rows if len(t))
        it.tr = [np.ascontiguousarray(t, SEGMENT_DTYPE) for t in true_rows]
        it.pr = [np.ascontiguousarray(p, SEGMENT_DTYPE) for p in pred_rows]
        it.t_clen = np.concatenate([clipped_lengths(t, int(org[r]), int(ln[r])) for r, t in enumerate(it.tr)])
        it.p_clen = np.concatenate([clipped_lengths(p, int(org[r]), int(ln[r])) for r, p in enumerate(it.pr)])
        self.rows_used += len(it.t_clen)
        self.outside += int((it.t_clen == 0).sum())
        if n == 0:
            return
        it.dev = dev = require_gpu()
        it.t_off, it.t_flat, it.d_trows = upload(it.tr, dev)
        it.p_off, it.p_flat, it.d_prows = upload(it.pr, dev)
        wb = L.dgrp_eval_workspace_bytes(nrec, max(int(it.t_off[-1]), int(it.p_off[-1])))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        it.stream = s = stream_ptr()

        def hits(d_labels, ro, d_rows):
            d_hits = torch.zeros(max(int(ro[-1]), 1), dtype=torch.int64, device=dev)
            check(L.dgrp_row_hits_batch(d_labels.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data,
                                        None if d_rows is None else d_rows.data_ptr(), ro.ctypes.data, d_hits.data_ptr(), work.data_ptr(),
                                        wb, s), "dgrp_row_hits_batch")
            return d_hits

        it.d_true = paint(ln, org, off, it.t_off, it.d_trows, work, dev)
        it.d_pred = paint(ln, org, off, it.p_off, it.d_prows, work, dev)
        d_ht = hits(it.d_pred, it.t_off, it.d_trows)   # annotation rows against the predicted labels
        d_hp = hits(it.d_true, it.p_off, it.d_prows)   # predicted rows against the truth
        d_cnf = torch.empty((self.C, self.C), dtype=torch.int64, device=dev)
        d_bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(L.dgrp_confusion_matrix(it.d_true.data_ptr(), it.d_pred.data_ptr(), n, self.C, d_cnf.data_ptr(), d_bad.data_ptr(), s),
              "dgrp_confusion_matrix")
        cnf, bad = d_cnf.cpu().numpy(), int(d_bad.item())
        it.ht, it.hp = d_ht.cpu().numpy()[:int(it.t_off[-1])], d_hp.cpu().numpy()[:int(it.p_off[-1])]
        if bad:
            raise ValueError(f"a label outside 0..{self.C - 1} reached the confusion matrix")
        self.cnf += cnf
        it.ok, it.hit = count(self.theta, it.t_flat["label"].astype(np.int64), it.t_clen, it.ht, self.elements, self.found)
        it.kept, it.good = count(self.theta, it.p_flat["label"].astype(np.int64), it.p_clen, it.hp, self.segments, self.supported)
        for r in self.reports:
            r.add(it, None if probed is None else probed.get(r.key))


def metrics_of(cnf: np.ndarray, bases: int) -> Dict[str, object]:
    """prediction._calculate_metrics of the matrix (numpy's NaN where a formula divides by zero), TotalACC = trace / bases."""
    from .prediction import _calculate_metrics
    with np.errstate(divide="ignore", invalid="ignore"):
        m = _calculate_metrics(np.asarray(cnf, np.int64))
        m["TotalACC"] = float(np.trace(cnf)) / bases if bases else float("nan")
    return m


def _num(x) -> Optional[float]:
    x = float(x)
    return None if math.isnan(x) else x


def report(acc: Accumulator, info: Dict[str, object]) -> Dict[str, object]:
    """The JSON content: `info` (paths, options) plus counts, the confusion matrix, every metric (NaN as None) and the element
    counts; then every report's summary under its key."""
    m = metrics_of(acc.cnf, acc.bases)
    metrics = {}
    for k, v in m.items():
        metrics[k] = [_num(x) for x in np.asarray(v).ravel()] if np.ndim(v) else _num(v)
    out = dict(info)
    out.update(classes=acc.C, bases=int(acc.bases), records=int(acc.records), records_annotated=int(acc.records_annotated),
               rows_used=int(acc.rows_used), outside=int(acc.outside), confusion_matrix=acc.cnf.astype(int).tolist(),
               metrics=metrics, min_overlap=acc.theta, elements=acc.elements.tolist(), found=acc.found.tolist(),
               segments=acc.segments.tolist(), supported=acc.supported.tolist())
    for r in acc.reports:
        out[r.key] = r.summary()
    return out


def tsv_report(rep: Dict[str, object]) -> str:
    """The report table: a header line, one line per class, then #TotalACC and #MCC; floats as repr(float) ('nan' for NaN)."""
    f = lambda x: repr(float("nan") if x is None else float(x))
    cnf = np.asarray(rep["confusion_matrix"], np.int64)
    m = rep["metrics"]
    lines = ["#" + "\t".join(TSV_COLUMNS)]
    for c in range(int(rep["classes"])):
        tp = int(cnf[c, c])
        lines.append("\t".join([str(c), str(int(cnf[c].sum())), str(int(cnf[:, c].sum())), str(tp), str(int(cnf[:, c].sum()) - tp),
                                str(int(cnf[c].sum()) - tp), f(m["TPR"][c]), f(m["PPV"][c]), f(m["F1"][c]),
                                str(rep["elements"][c]), str(rep["found"][c]), str(rep["segments"][c]), str(rep["supported"][c])]))
    lines.append(f"#TotalACC\t{f(m['TotalACC'])}")
    lines.append(f"#MCC\t{f(m['MCC'])}")
    return "\n".join(lines) + "\n"


def strip_n(raw: bytes) -> Tuple[int, int]:
    """(startpos, kept length) of a record's sequence bytes, as upload_sequence strips them (kept < 0: all N)."""
    import ctypes as C

    from ._lib import check, lib
    st, kept = C.c_int64(0), C.c_int64(0)
    host = np.frombuffer(raw, dtype=np.uint8)
    check(lib().dgrp_strip_n(host.ctypes.data if len(raw) else None, len(raw), C.byref(st), C.byref(kept)), "dgrp_strip_n")
    return int(st.value), int(kept.value)


def record_name(filename: str, header: str) -> str:
    """The annotation contig a record is matched to: a `.npz` input's basename up to the first '.' (the reference's `train` rule,
    deepgrp/__main__.py:315-316), else the first whitespace-delimited word of the FASTA header."""
    if filename.endswith(".npz") and os.path.isfile(filename):
        return os.path.basename(filename).split(".")[0]
    words = header.split()
    return words[0] if words else ""


def evaluate(model, annotation: Dict[str, np.ndarray], inputs: Iterable[Tuple[str, Iterable[Tuple[str, object]]]], pipe,
             repeats: Sequence[int], min_overlap: float = 0.5, info: Optional[Dict[str, object]] = None, reports=()) -> Dict[str, object]:
    """Run `pipe` (a ContigPipeline of `model`) over the records of `inputs` -- (filename, (header, record) pairs) as
    `predict` reads them -- and score the rows it produces against `annotation` (read_annotation's dict).  Returns the JSON
    content; raises NoMatchError when no annotation row belongs to any record (and logs a warning as soon as the first
    record read has none).  reports (see the module's REPORTS): each is bound to the annotation and the model's classes, its counts
    are summed into it and the JSON content gains its key.  Where one of them has a probe the runner takes the merged path with
    scores and `Accumulator.probe`; else a record is the fused call."""
    from .runner import RecordRunner

    classes = int(model.output_shape[2])
    for r in reports:
        r.bind(annotation, classes)
    acc = Accumulator(classes, min_overlap, reports)
    probe = acc.probe(annotation)
    runner = RecordRunner(pipe, scores=True, probe=probe) if probe is not None else RecordRunner(pipe)
    empty = np.zeros(0, SEGMENT_DTYPE)
    seen_names: List[str] = []
    state = {"matched": False, "warned": False}

    def keyed():
        for filename, records in inputs:
            for header, rec in records:
                if isinstance(rec, str):
                    # text records stay text: the runner's worker uploads them on its own stream, as `predict` does; their
                    # startpos and kept length come from the same host scan (dgrp_strip_n; kept < 0: the worker raises)
                    rec = rec.encode("utf-8")
                    startpos, length = strip_n(rec)
                else:
                    startpos, length = int(rec.startpos), int(rec.length)
                name = record_name(filename, header)
                if len(seen_names) < 5 and name not in seen_names:
                    seen_names.append(name)
                if name in annotation:
                    state["matched"] = True
                elif not state["matched"] and not state["warned"]:
                    # the usual cause of an empty evaluation (`chr1` against `1`) shows before the first forward pass ends
                    state["warned"] = True
                    _LOG.warning("record %r of %s has no annotation rows; annotation contigs: %s", name, filename,
                                 ", ".join(repr(x) for x in sorted(annotation)[:5]) or "none with kept rows")
                # the key carries what the evaluation needs past the runner: header, name (where a runner with scores reads a
                # record's name), startpos, kept length
                yield (header, name, startpos, length), rec

    for out in runner.outputs(keyed()):
        kind, key, rows, scores = out[:4]
        probed = out[5] if probe is not None else None
        keys = key if kind == "batch" else [key]
        rows = np.asarray(rows)
        if kind == "batch":
            contig = rows["contig"] if rows.size else np.zeros(0, np.int32)
            cut = np.searchsorted(contig, np.arange(len(keys) + 1))
            pred = [rows[cut[r]:cut[r + 1]] for r in range(len(keys))]
        else:
            pred = [rows]
        true = [annotation.get(k[1], empty) for k in keys]
        acc.add([k[2] for k in keys], [k[3] for k in keys], pred, true, scores, probed, [k[1] for k in keys])
    if acc.rows_used == 0:
        raise NoMatchError("no annotation row names a record of the inputs (records: {}; annotation: {})".format(
            ", ".join(repr(x) for x in seen_names) or "none",
            ", ".join(repr(x) for x in sorted(annotation)[:5]) or "no kept rows"))
    info = dict(info or {})
    info.setdefault("repeats", [int(r) for r in repeats])
    return report(acc, info)
