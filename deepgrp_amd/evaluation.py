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

With curves (`evaluate --curves`, deepgrp_amd/curves.py) the runner keeps the merged probabilities of every work item long enough
for `Accumulator.probe`: it paints the item's truth on the worker's stream and counts every probability into per-class
histograms split by truth (dgrp_prob_hist_batch); the rows' BED scores come with the rows (dgrp_row_scores_batch).  With element
curves (`--curve_elements`) `Accumulator.add` also paints the predicted rows as (label, score) keys and takes every annotation row's
detection score against them (dgrp_paint_row_keys_batch, dgrp_row_detect_batch).

With strata (`evaluate --strata`, deepgrp_amd/strata.py) the probe also paints the truth as (label, stratum) keys and counts the true
class's probability by them (dgrp_paint_strata_batch, dgrp_prob_hist_strata_batch), and `Accumulator.add` groups the element counts
it already has by label and stratum.

With off-target counts (`evaluate --offtarget`, deepgrp_amd/offtarget.py) `Accumulator.add` also paints what the listing says lies
under every base as keys (dgrp_paint_keys_batch), cross-tabulates the predicted labels against them -- every base, and the bases
of the unsupported predicted rows alone (dgrp_key_crosstab_batch) -- and takes four counts per predicted row
(dgrp_row_key_classes_batch).  The runner and the probe are not touched.

With boundaries (`evaluate --boundaries`, deepgrp_amd/boundaries.py) `Accumulator.add` also takes, for the annotation rows against
the predicted labels and for the predicted rows against the truth, the runs, the first and last matching base and the two flanks of
every row (dgrp_row_bounds_batch) and counts them into the edge-offset and fragment tables (dgrp_bound_hist_batch); only the tables
come back.  The runner and the probe are not touched."""
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


class Accumulator:
    """Integer sums over work items: the C x C confusion matrix (cnf[truth][pred]) and the element counts."""

    def __init__(self, classes: int, min_overlap: float, curves=None, strata=None, offtarget=None, boundaries=None):
        if not 0.0 < min_overlap <= 1.0:
            raise ValueError(f"min_overlap must lie in (0, 1], not {min_overlap}")
        self.C, self.theta = int(classes), float(min_overlap)
        self.curves = curves                           # a curves.Curves: probability histograms and rows by score are summed into it
        self.strata = strata                           # a strata.Strata: element counts and histograms by (label, stratum)
        self.offtarget = offtarget                     # an offtarget.Offtarget: predicted labels by what the listing says is there
        self.boundaries = boundaries                   # a boundaries.Boundaries: edge offsets and runs of both views
        self.cnf = np.zeros((self.C, self.C), np.int64)
        self.elements = np.zeros(self.C, np.int64)
        self.found = np.zeros(self.C, np.int64)
        self.segments = np.zeros(self.C, np.int64)
        self.supported = np.zeros(self.C, np.int64)
        self.bases = self.records = self.records_annotated = self.rows_used = self.outside = 0

    def _count(self, labels: np.ndarray, clen: np.ndarray, hits: np.ndarray, total: np.ndarray, good: np.ndarray):
        """total[label] += 1 per row with a base inside its record, good[label] += 1 per such row with hits >= theta * its clipped
        length; -> the two masks."""
        ok = clen > 0
        np.add.at(total, labels[ok], 1)
        hit = ok & (hits.astype(np.float64) >= self.theta * clen.astype(np.float64))
        np.add.at(good, labels[hit], 1)
        return ok, hit

    @staticmethod
    def _tables(origins: Sequence[int], lengths: Sequence[int]):
        """Records back to back in one flat buffer: -> (lengths, origins, offsets [nrec + 1]) as the library reads them."""
        ln = np.ascontiguousarray(lengths, np.int64)
        org = np.ascontiguousarray(origins, np.int64)
        off = np.zeros(len(ln) + 1, np.int64)
        np.cumsum(ln, out=off[1:])
        return ln, org, off

    @staticmethod
    def _upload(rows: Sequence[np.ndarray], dev):
        """The rows of the records as one device array: -> (row offsets [nrec + 1], the rows on the host, on the device or None)."""
        import torch
        ro = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(x) for x in rows], out=ro[1:])
        flat = np.concatenate(rows) if ro[-1] else np.zeros(0, SEGMENT_DTYPE)
        d = torch.from_numpy(flat.view(np.uint8)).to(dev) if flat.size else None
        return ro, flat, d

    @staticmethod
    def _paint(ln: np.ndarray, org: np.ndarray, off: np.ndarray, ro: np.ndarray, d_rows, work, dev):
        """A zeroed label track of the records with the rows painted on it, on the current stream (dgrp_paint_rows_batch)."""
        import torch

        from ._lib import check, lib
        from .pipeline import stream_ptr
        d_labels = torch.zeros(int(off[-1]), dtype=torch.int8, device=dev)
        check(lib().dgrp_paint_rows_batch(d_labels.data_ptr(), len(ln), off.ctypes.data, ln.ctypes.data, org.ctypes.data,
                                          None if d_rows is None else d_rows.data_ptr(), ro.ctypes.data, work.data_ptr(), work.numel(),
                                          stream_ptr()), "dgrp_paint_rows_batch")
        return d_labels

    def _row_strata(self, annotation, name: str, rows: np.ndarray) -> np.ndarray:
        """The stratum of every annotation row of contig `name`: its millidiv travels beside the rows (annotation.Rows.millidiv;
        a table has none: -1 everywhere)."""
        div_of = getattr(annotation, "millidiv", None)
        md = None if div_of is None or name not in div_of else div_of[name]
        return self.strata.strata_of(rows, md)

    def _probe_strata(self, annotation):
        """The strata's share of the probe: the item's truth painted as keys (dgrp_paint_strata_batch), the true class's
        probability counted by them (dgrp_prob_hist_strata_batch) -> (hist [C, S, bins], flag) as host arrays."""
        st, empty = self.strata, np.zeros(0, SEGMENT_DTYPE)

        def run(d_probs, row0, lengths, startposes, keys):
            import torch

            from ._lib import check, lib
            from .pipeline import require_gpu, stream_ptr
            L = lib()
            ln, org, off = self._tables(startposes, lengths)
            nrec = len(ln)
            hist = np.zeros((self.C, st.S, st.bins), np.int64)
            if nrec == 0 or int(off[-1]) == 0 or d_probs is None:
                return hist, 0
            if d_probs.dtype != torch.float32 or d_probs.ndim != 2 or not d_probs.is_contiguous() or d_probs.shape[1] != self.C:
                raise ValueError(f"the strata take a contiguous float32 [rows, {self.C}] array")
            dev = require_gpu()
            tr = [np.ascontiguousarray(annotation.get(k[1], empty), SEGMENT_DTYPE) for k in keys]
            t_off, _flat, d_trows = self._upload(tr, dev)
            sof = [self._row_strata(annotation, k[1], t) for k, t in zip(keys, tr)]
            d_st = torch.from_numpy(np.concatenate(sof)).to(dev) if int(t_off[-1]) else None
            work = torch.empty(max(int(L.dgrp_eval_workspace_bytes(nrec, int(t_off[-1]))), int(L.dgrp_prob_hist_strata_workspace_bytes(nrec)), 1),
                               dtype=torch.uint8, device=dev)
            d_keys = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)      # (32-bit keys; the sign of the type is not read)
            ptr = lambda t: None if t is None else t.data_ptr()
            check(L.dgrp_paint_strata_batch(d_keys.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, ptr(d_trows),
                                            t_off.ctypes.data, ptr(d_st), work.data_ptr(), work.numel(), stream_ptr()),
                  "dgrp_paint_strata_batch")
            r0 = np.ascontiguousarray(row0, np.int64)
            d_hist = torch.empty((self.C, st.S, st.bins), dtype=torch.int64, device=dev)
            d_bad = torch.empty(1, dtype=torch.int32, device=dev)
            check(L.dgrp_prob_hist_strata_batch(d_probs.data_ptr(), self.C, nrec, r0.ctypes.data, ln.ctypes.data, d_keys.data_ptr(),
                                                off.ctypes.data, st.S, st.bins, d_hist.data_ptr(), d_bad.data_ptr(), work.data_ptr(),
                                                work.numel(), stream_ptr()), "dgrp_prob_hist_strata_batch")
            return d_hist.cpu().numpy(), int(d_bad.item())
        return run

    def probe(self, annotation: Dict[str, np.ndarray]):
        """RecordRunner's probe for the curves: called on the worker's stream with the merged probabilities of a work item (record r:
        rows [row0[r], row0[r] + lengths[r]) of d_probs; keys[r][1] its annotation contig), it paints the item's truth, counts the
        histograms (dgrp_prob_hist_batch) and returns them with the flag as host arrays; `add` sums them.  With strata what it
        returns is a dict: "curves" that pair (where there are curves), "strata" the pair of `_probe_strata`."""
        if self.strata is not None:
            curve_run = self._probe_curves(annotation) if self.curves is not None else None
            strata_run = self._probe_strata(annotation)

            def both(*a):
                out = {"strata": strata_run(*a)}
                if curve_run is not None:
                    out["curves"] = curve_run(*a)
                return out
            return both
        return self._probe_curves(annotation)

    def _probe_curves(self, annotation: Dict[str, np.ndarray]):
        bins, empty = self.curves.bins, np.zeros(0, SEGMENT_DTYPE)

        def run(d_probs, row0, lengths, startposes, keys):
            import torch

            from ._lib import check, lib
            from .pipeline import require_gpu, stream_ptr
            L = lib()
            ln, org, off = self._tables(startposes, lengths)
            nrec = len(ln)
            hist = np.zeros((self.C, 2, bins), np.int64)
            if nrec == 0 or int(off[-1]) == 0 or d_probs is None:
                return hist, 0
            if d_probs.dtype != torch.float32 or d_probs.ndim != 2 or not d_probs.is_contiguous() or d_probs.shape[1] != self.C:
                raise ValueError(f"the curves take a contiguous float32 [rows, {self.C}] array")
            dev = require_gpu()
            tr = [np.ascontiguousarray(annotation.get(k[1], empty), SEGMENT_DTYPE) for k in keys]
            t_off, _flat, d_trows = self._upload(tr, dev)
            work = torch.empty(max(int(L.dgrp_eval_workspace_bytes(nrec, int(t_off[-1]))), int(L.dgrp_prob_hist_workspace_bytes(nrec, self.C, bins))),
                               dtype=torch.uint8, device=dev)
            d_true = self._paint(ln, org, off, t_off, d_trows, work, dev)
            r0 = np.ascontiguousarray(row0, np.int64)
            d_hist = torch.empty((self.C, 2, bins), dtype=torch.int64, device=dev)
            d_bad = torch.empty(1, dtype=torch.int32, device=dev)
            check(L.dgrp_prob_hist_batch(d_probs.data_ptr(), self.C, nrec, r0.ctypes.data, ln.ctypes.data, d_true.data_ptr(), off.ctypes.data,
                                         bins, d_hist.data_ptr(), d_bad.data_ptr(), work.data_ptr(), work.numel(), stream_ptr()),
                  "dgrp_prob_hist_batch")
            return d_hist.cpu().numpy(), int(d_bad.item())
        return run

    def add(self, origins: Sequence[int], lengths: Sequence[int], pred_rows: Sequence[np.ndarray],
            true_rows: Sequence[np.ndarray], scores: Optional[np.ndarray] = None, probed=None, names: Sequence[str] = (),
            true_strata: Optional[Sequence[np.ndarray]] = None, off_rows: Optional[Sequence[np.ndarray]] = None,
            off_keys: Optional[Sequence[np.ndarray]] = None) -> None:
        """One work item: records r = 0.. with startpos origins[r], kept length lengths[r], the TSV rows `predict` wrote for it
        (original coordinates) and its kept annotation rows.  With curves also the scores of the predicted rows, record after record
        (pipeline.ROW_SCORE_DTYPE), what `probe` returned for the item, and the records' names for its error.  With strata also the
        stratum of every annotation row, record after record as true_rows.  With off-target counts also the un-modelled rows of
        every record and their keys (annotation.Rows.offtarget_rows / offtarget_keys)."""
        import torch

        from ._lib import check, lib
        from .pipeline import require_gpu, stream_ptr
        L = lib()
        nrec = len(lengths)
        if nrec == 0:
            return
        ln, org, off = self._tables(origins, lengths)
        n = int(off[-1])
        if self.strata is not None and probed is not None:
            shist, sflag = probed["strata"]
            if sflag:
                raise ValueError("a probability outside [0, 1] or a key outside {} classes and {} strata reached the strata histogram "
                                 "(record{} {})".format(self.C, self.strata.S, "s" if len(names) > 1 else "",
                                                        ", ".join(repr(x) for x in list(names)[:5]) + (", ..." if len(names) > 5 else "")))
            self.strata.hist += shist
            probed = probed.get("curves")
        if self.curves is not None and probed is not None:
            hist, flag = probed
            if flag:
                raise ValueError("a probability outside [0, 1] or a label outside 0..{} reached the probability histogram (record{} {})".format(
                    self.C - 1, "s" if len(names) > 1 else "", ", ".join(repr(x) for x in list(names)[:5]) + (", ..." if len(names) > 5 else "")))
            self.curves.hist += hist
        self.records += nrec
        self.bases += n
        self.records_annotated += sum(1 for t in true_rows if len(t))
        tr = [np.ascontiguousarray(t, SEGMENT_DTYPE) for t in true_rows]
        pr = [np.ascontiguousarray(p, SEGMENT_DTYPE) for p in pred_rows]
        t_clen = [clipped_lengths(t, int(org[r]), int(ln[r])) for r, t in enumerate(tr)]
        self.rows_used += sum(len(t) for t in tr)
        self.outside += int(sum(int((c == 0).sum()) for c in t_clen))
        if n == 0:
            return
        dev = require_gpu()
        t_off, t_flat, d_trows = self._upload(tr, dev)
        p_off, p_flat, d_prows = self._upload(pr, dev)
        wb = L.dgrp_eval_workspace_bytes(nrec, max(int(t_off[-1]), int(p_off[-1])))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        s = stream_ptr()
        ptr = lambda t: None if t is None else t.data_ptr()

        def hits(d_labels, ro, d_rows):
            d_hits = torch.zeros(max(int(ro[-1]), 1), dtype=torch.int64, device=dev)
            check(L.dgrp_row_hits_batch(d_labels.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, ptr(d_rows),
                                        ro.ctypes.data, d_hits.data_ptr(), work.data_ptr(), wb, s), "dgrp_row_hits_batch")
            return d_hits

        d_true = self._paint(ln, org, off, t_off, d_trows, work, dev)
        d_pred = self._paint(ln, org, off, p_off, d_prows, work, dev)
        d_ht = hits(d_pred, t_off, d_trows)            # annotation rows against the predicted labels
        d_hp = hits(d_true, p_off, d_prows)            # predicted rows against the truth
        d_cnf = torch.empty((self.C, self.C), dtype=torch.int64, device=dev)
        d_bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(L.dgrp_confusion_matrix(d_true.data_ptr(), d_pred.data_ptr(), n, self.C, d_cnf.data_ptr(), d_bad.data_ptr(), s),
              "dgrp_confusion_matrix")
        cnf, bad = d_cnf.cpu().numpy(), int(d_bad.item())
        ht, hp = d_ht.cpu().numpy()[:int(t_off[-1])], d_hp.cpu().numpy()[:int(p_off[-1])]
        if bad:
            raise ValueError(f"a label outside 0..{self.C - 1} reached the confusion matrix")
        self.cnf += cnf
        if t_flat.size:
            ok, hit = self._count(t_flat["label"].astype(np.int64), np.concatenate(t_clen), ht, self.elements, self.found)
            if self.strata is not None:
                if true_strata is None or sum(len(x) for x in true_strata) != len(t_flat):
                    raise ValueError(f"{len(t_flat)} annotation rows but {0 if true_strata is None else sum(len(x) for x in true_strata)} strata")
                self.strata.count(t_flat["label"], np.concatenate(true_strata), np.concatenate(t_clen), ht, ok, hit)
        kept = good = np.zeros(0, bool)
        if p_flat.size:
            p_clen = np.concatenate([clipped_lengths(p, int(org[r]), int(ln[r])) for r, p in enumerate(pr)])
            kept, good = self._count(p_flat["label"].astype(np.int64), p_clen, hp, self.segments, self.supported)
            if self.curves is not None:
                from .curves import row_counts, row_scores_of
                if scores is None or len(scores) != len(p_flat):
                    raise ValueError(f"{len(p_flat)} predicted rows but {0 if scores is None else len(scores)} scores")
                sc = np.zeros(len(p_flat), np.int64)
                sc[kept] = row_scores_of(scores[kept])
                seg, sup = row_counts(p_flat["label"].astype(np.int64), sc, kept, good, self.C)
                self.curves.seg += seg
                self.curves.sup += sup
        if self.curves is not None and self.curves.elements and t_flat.size:
            self._detect(ln, org, off, t_off, t_flat, d_trows, np.concatenate(t_clen), p_off, d_prows, scores, names)
        if self.offtarget is not None:
            self._offtarget(ln, org, off, tr, off_rows, off_keys, d_pred, pr, p_off, p_flat, d_prows, kept, good)
        if self.boundaries is not None:
            self._boundaries(ln, org, off, tr, t_off, d_trows, pr, p_off, d_prows, d_true, d_pred)

    def _boundaries(self, ln, org, off, tr, t_off, d_trows, pr, p_off, d_prows, d_true, d_pred) -> None:
        """The boundaries' share of a work item, once per view: the element view takes the annotation rows (joined into units with
        --boundary_join, uploaded anew then) against the predicted labels, the row view the predicted rows against the truth.
        Per view dgrp_row_bounds_batch, then dgrp_bound_hist_batch with need = ceil(theta * clipped length); the three tables and
        the flag are all that is copied back."""
        import torch

        from ._lib import check, lib
        from .boundaries import FRAG
        from .curves import need_of
        from .pipeline import require_gpu, stream_ptr
        bd, L, dev, s, nrec = self.boundaries, lib(), require_gpu(), stream_ptr(), len(ln)
        W, C = bd.W, self.C
        if bd.join is not None:
            tr = [bd.units(t) for t in tr]
            t_off, _t_flat, d_trows = self._upload(tr, dev)
        for view, (rows, ro, d_rows, d_labels) in enumerate(((tr, t_off, d_trows, d_pred), (pr, p_off, d_prows, d_true))):
            nrows = int(ro[-1])
            if nrows == 0:
                continue
            clen = np.concatenate([clipped_lengths(q, int(org[r]), int(ln[r])) for r, q in enumerate(rows)])
            d_need = torch.from_numpy(need_of(self.theta, clen)).to(dev)
            wb = int(L.dgrp_row_bounds_workspace_bytes(nrec, nrows))
            work = torch.empty(max(wb, int(L.dgrp_bound_hist_workspace_bytes(nrec)), 1), dtype=torch.uint8, device=dev)
            d_bounds = torch.empty((nrows, 5), dtype=torch.int64, device=dev)          # (dgrp_row_bound: 40 bytes a row)
            check(L.dgrp_row_bounds_batch(d_labels.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, d_rows.data_ptr(),
                                          ro.ctypes.data, W, d_bounds.data_ptr(), work.data_ptr(), work.numel(), s), "dgrp_row_bounds_batch")
            d_frag = torch.empty((C, FRAG), dtype=torch.int64, device=dev)
            d_edge = torch.empty((C, 2, 2 * W + 1), dtype=torch.int64, device=dev)
            d_tally = torch.empty((C, 2), dtype=torch.int64, device=dev)
            d_bad = torch.empty(1, dtype=torch.int32, device=dev)
            check(L.dgrp_bound_hist_batch(nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, d_rows.data_ptr(), ro.ctypes.data,
                                          d_bounds.data_ptr(), d_need.data_ptr(), C, W, d_frag.data_ptr(), d_edge.data_ptr(),
                                          d_tally.data_ptr(), d_bad.data_ptr(), work.data_ptr(), work.numel(), s), "dgrp_bound_hist_batch")
            frag, edge, tally, bad = d_frag.cpu().numpy(), d_edge.cpu().numpy(), d_tally.cpu().numpy(), int(d_bad.item())
            if bad:
                raise ValueError(f"a row label outside 0..{C - 1} reached the boundary counts")
            bd.count(view, frag, edge, tally)

    def _offtarget(self, ln, org, off, tr, off_rows, off_keys, d_pred, pr, p_off, p_flat, d_prows, kept, good) -> None:
        """The off-target share of a work item.  The key track: the item's modelled rows with their labels as keys and its
        un-modelled rows with 64 + family id (dgrp_paint_keys_batch).  Two cross-tabulations against it (dgrp_key_crosstab_batch):
        the predicted labels, and a second track painted from only the predicted rows `_count` found unsupported -- of which the
        label 0, everything outside those rows, is dropped.  Four counts per predicted row (dgrp_row_key_classes_batch)."""
        import torch

        from ._lib import check, lib
        from .pipeline import require_gpu, stream_ptr
        ot, L, dev, s, nrec = self.offtarget, lib(), require_gpu(), stream_ptr(), len(ln)
        n = int(off[-1])
        if off_rows is None or off_keys is None or len(off_rows) != nrec or len(off_keys) != nrec:
            raise ValueError("the off-target counts need the un-modelled rows and keys of every record")
        k_rows, k_keys = [], []
        for r in range(nrec):
            o = np.ascontiguousarray(off_rows[r], SEGMENT_DTYPE)
            ok = np.ascontiguousarray(off_keys[r], np.uint32)
            if len(o) != len(ok):
                raise ValueError(f"{len(o)} un-modelled rows but {len(ok)} keys")
            k_rows.append(np.concatenate([tr[r], o]))
            k_keys.append(np.concatenate([tr[r]["label"].astype(np.uint32), ok]))
        k_off, _k_flat, d_krows = self._upload(k_rows, dev)
        uns = kept & ~good
        ur = [p[uns[int(p_off[r]):int(p_off[r + 1])]] for r, p in enumerate(pr)]
        u_off, _u_flat, d_urows = self._upload(ur, dev)
        wb = int(L.dgrp_eval_workspace_bytes(nrec, max(int(k_off[-1]), int(p_off[-1]), int(u_off[-1]))))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        d_rk = torch.from_numpy(np.concatenate(k_keys).view(np.int32)).to(dev) if int(k_off[-1]) else None   # (the sign of the type is not read)
        d_keys = torch.empty(n, dtype=torch.int32, device=dev)                    # (32-bit keys; the sign of the type is not read)
        check(L.dgrp_paint_keys_batch(d_keys.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, ptr(d_krows),
                                      k_off.ctypes.data, ptr(d_rk), work.data_ptr(), wb, s), "dgrp_paint_keys_batch")
        d_uns = self._paint(ln, org, off, u_off, d_urows, work, dev)
        d_hist = torch.empty((2, self.C, ot.K), dtype=torch.int64, device=dev)
        d_bad = torch.empty(2, dtype=torch.int32, device=dev)
        for k, d_lab in enumerate((d_pred, d_uns)):
            check(L.dgrp_key_crosstab_batch(d_lab.data_ptr(), d_keys.data_ptr(), n, self.C, ot.K, d_hist[k].data_ptr(), d_bad[k:].data_ptr(), s),
                  "dgrp_key_crosstab_batch")
        d_cls = torch.zeros((max(int(p_off[-1]), 1), 4), dtype=torch.int64, device=dev)
        check(L.dgrp_row_key_classes_batch(d_keys.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, ptr(d_prows),
                                           p_off.ctypes.data, d_cls.data_ptr(), work.data_ptr(), wb, s), "dgrp_row_key_classes_batch")
        hist, bad, cls = d_hist.cpu().numpy(), d_bad.cpu().numpy(), d_cls.cpu().numpy()[:int(p_off[-1])]
        if bad.any():
            raise ValueError(f"a predicted label outside 0..{self.C - 1} or a key outside the {ot.F} families of the listing reached the "
                             "off-target counts")
        hist[1, 0] = 0
        ot.hist += hist
        if p_flat.size:
            ot.count_rows(p_flat["label"].astype(np.int64), kept, good, cls)

    def _detect(self, ln, org, off, t_off, t_flat, d_trows, t_clen, p_off, d_prows, scores, names) -> None:
        """The element curves' share of a work item: the predicted rows painted as keys (label << 10 | BED score) on a zeroed
        uint16 track (dgrp_paint_row_keys_batch), the detection score of every annotation row against it (dgrp_row_detect_batch),
        counted into curves.det by label and score + 1 for the rows with a base inside their record."""
        import torch

        from ._lib import check, lib
        from .curves import need_of
        from .pipeline import ROW_SCORE_DTYPE, require_gpu, stream_ptr
        L, dev, s, nrec = lib(), require_gpu(), stream_ptr(), len(ln)
        wb = int(L.dgrp_row_detect_workspace_bytes(nrec, max(int(t_off[-1]), int(p_off[-1]))))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        d_keys = torch.zeros(int(off[-1]), dtype=torch.int16, device=dev)          # (16-bit keys; the sign of the type is not read)
        if d_prows is not None:
            sc = np.ascontiguousarray(scores, ROW_SCORE_DTYPE)
            d_sc = torch.from_numpy(sc.view(np.uint8)).to(dev)
            rc = L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, d_prows.data_ptr(),
                                             p_off.ctypes.data, d_sc.data_ptr(), work.data_ptr(), wb, s)
            if rc != 0:
                raise ValueError("the predicted rows of record{} {} cannot be painted by score: {}".format(
                    "s" if len(names) > 1 else "", ", ".join(repr(x) for x in list(names)[:5]) + (", ..." if len(names) > 5 else ""),
                    L.dgrp_last_error().decode("utf-8", "replace")))
        d_need = torch.from_numpy(need_of(self.theta, t_clen)).to(dev)
        d_det = torch.empty(len(t_flat), dtype=torch.int32, device=dev)
        check(L.dgrp_row_detect_batch(d_keys.data_ptr(), nrec, off.ctypes.data, ln.ctypes.data, org.ctypes.data, d_trows.data_ptr(),
                                      t_off.ctypes.data, d_need.data_ptr(), d_det.data_ptr(), work.data_ptr(), wb, s), "dgrp_row_detect_batch")
        det = d_det.cpu().numpy().astype(np.int64)
        ok = t_clen > 0
        np.add.at(self.curves.det, (t_flat["label"].astype(np.int64)[ok], det[ok] + 1), 1)


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
    counts; with curves also their summaries under `curves`."""
    m = metrics_of(acc.cnf, acc.bases)
    metrics = {}
    for k, v in m.items():
        metrics[k] = [_num(x) for x in np.asarray(v).ravel()] if np.ndim(v) else _num(v)
    out = dict(info)
    out.update(classes=acc.C, bases=int(acc.bases), records=int(acc.records), records_annotated=int(acc.records_annotated),
               rows_used=int(acc.rows_used), outside=int(acc.outside), confusion_matrix=acc.cnf.astype(int).tolist(),
               metrics=metrics, min_overlap=acc.theta, elements=acc.elements.tolist(), found=acc.found.tolist(),
               segments=acc.segments.tolist(), supported=acc.supported.tolist())
    if acc.curves is not None:
        out["curves"] = acc.curves.summary()
    if acc.strata is not None:
        out["strata"] = acc.strata.summary()
    if acc.offtarget is not None:
        out["offtarget"] = acc.offtarget.summary()
    if acc.boundaries is not None:
        out["boundaries"] = acc.boundaries.summary()
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
             repeats: Sequence[int], min_overlap: float = 0.5, info: Optional[Dict[str, object]] = None, curves=None,
             strata=None, offtarget=None, boundaries=None) -> Dict[str, object]:
    """Run `pipe` (a ContigPipeline of `model`) over the records of `inputs` -- (filename, (header, record) pairs) as
    `predict` reads them -- and score the rows it produces against `annotation` (read_annotation's dict).  Returns the JSON
    content; raises NoMatchError when no annotation row belongs to any record (and logs a warning as soon as the first
    record read has none).  curves (a curves.Curves of the model's classes): the runner takes the merged path with scores and
    `Accumulator.probe`, the counts of the curves are summed into it and the JSON content gains the key `curves`; without it a
    record is the fused call, as before.  strata (a strata.Strata of the model's classes): the same runner and probe, the counts by
    (label, stratum) are summed into it and the JSON content gains the key `strata`; the divergence of the rows is
    `annotation.millidiv` (annotation.Rows), -1 everywhere without it.  offtarget (an offtarget.Offtarget of the model's classes
    and the listing's families): `annotation` is what annotation.evaluation_rows(offtarget=True) returns, the counts are summed
    into it and the JSON content gains the key `offtarget`; the runner is the one the other arguments choose.  boundaries (a
    boundaries.Boundaries of the model's classes): the edge offsets and runs of both views are summed into it and the JSON content
    gains the key `boundaries`; the runner is the one the other arguments choose."""
    from .runner import RecordRunner

    classes = int(model.output_shape[2])
    if curves is not None and curves.C != classes:
        raise ValueError(f"curves of {curves.C} classes for a model of {classes}")
    if strata is not None and strata.C != classes:
        raise ValueError(f"strata of {strata.C} classes for a model of {classes}")
    if offtarget is not None:
        if offtarget.C != classes:
            raise ValueError(f"off-target counts of {offtarget.C} classes for a model of {classes}")
        if getattr(annotation, "offtarget_rows", None) is None:
            raise ValueError("off-target counts need the un-modelled rows of a RepeatMasker listing (annotation.evaluation_rows(offtarget=True))")
    if boundaries is not None and boundaries.C != classes:
        raise ValueError(f"boundaries of {boundaries.C} classes for a model of {classes}")
    acc = Accumulator(classes, min_overlap, curves, strata, offtarget, boundaries)
    no_keys = np.zeros(0, np.uint32)
    probing = curves is not None or strata is not None
    runner = RecordRunner(pipe, scores=True, probe=acc.probe(annotation)) if probing else RecordRunner(pipe)
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
        probed = out[5] if probing else None
        keys = key if kind == "batch" else [key]
        rows = np.asarray(rows)
        if kind == "batch":
            contig = rows["contig"] if rows.size else np.zeros(0, np.int32)
            cut = np.searchsorted(contig, np.arange(len(keys) + 1))
            pred = [rows[cut[r]:cut[r + 1]] for r in range(len(keys))]
        else:
            pred = [rows]
        true = [annotation.get(k[1], empty) for k in keys]
        true_strata = [acc._row_strata(annotation, k[1], t) for k, t in zip(keys, true)] if strata is not None else None
        off_rows = [annotation.offtarget_rows.get(k[1], empty) for k in keys] if offtarget is not None else None
        off_keys = [annotation.offtarget_keys.get(k[1], no_keys) for k in keys] if offtarget is not None else None
        acc.add([k[2] for k in keys], [k[3] for k in keys], pred, true, scores, probed, [k[1] for k in keys], true_strata, off_rows, off_keys)
    if acc.rows_used == 0:
        raise NoMatchError("no annotation row names a record of the inputs (records: {}; annotation: {})".format(
            ", ".join(repr(x) for x in seen_names) or "none",
            ", ".join(repr(x) for x in sorted(annotation)[:5]) or "no kept rows"))
    info = dict(info or {})
    info.setdefault("repeats", [int(r) for r in repeats])
    return report(acc, info)
