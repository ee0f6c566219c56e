"""`evaluate --curves`: what a threshold does to precision and recall, from integer counts alone.

Base curves.  Per class c the device counts the merged probability P[b, c] of every evaluated base into `bins` bins, split by whether
the base's truth is c (dgrp_prob_hist_batch; `reference_hist` is its numpy statement): bin k = min(bins - 1, int(float32(p) *
float32(bins))).  Threshold k / bins means "call the base class c if its bin is >= k"; TP, FP, FN, TN of every threshold are suffix
sums of the two histograms, every rate a ratio of those integers (float64 only there, NaN where a denominator is 0).

Row curves answer "what does `predict --bed_min_score m` keep": per class and m = 0..1000 the predicted rows whose BED score is at
least m (`segments`), those of them the annotation supports by `evaluate`'s --min_overlap rule (`supported`), and their ratio.

Element curves (`--curve_elements`) are the other half: how many annotated elements are still found once the rows below m are gone.
Predict's rows of one record never overlap, so the bases of an element that rows of its class with score >= m cover cannot rise
with m: an element has one detection score d, the largest m at which the --min_overlap rule still finds it (-1: not even at 0), and
`found` at every m is a suffix sum of the histogram of d (dgrp_paint_row_keys_batch and dgrp_row_detect_batch; `reference_detect`
is their numpy statement).

ON THE DEVICE (`Curves`, a report of deepgrp_amd/evaluation.py).  The runner keeps the merged probabilities of every work item long
enough for `Curves.probe`: it paints the item's truth on the worker's stream and counts every probability into the per-class
histograms split by truth; the rows' BED scores come with the rows (dgrp_row_scores_batch).  With element curves `Curves.add` also
paints the predicted rows as (label, score) keys and takes every annotation row's detection score against them.

Everything else here is numpy over int64; the same counts give the same file bytes."""
from __future__ import annotations

import math
import sys
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from .outfiles import plan_prefix, write_texts

MIN_BINS, MAX_BINS, DEFAULT_BINS = 2, 4096, 1000
SCORES = 1001                                       # BED scores 0..1000
BASES_HEADER = ("class", "threshold", "TP", "FP", "FN", "TN", "TPR", "FPR", "PPV", "F1")
ROWS_HEADER = ("class", "min_score", "segments", "supported", "precision")
ELEMENTS_HEADER = ("class", "min_score", "elements", "found", "recall", "segments", "supported", "precision", "F1")


class CurvePlan(NamedTuple):
    prefix: str
    bins: int
    bases_path: str
    rows_path: str
    elements_path: Optional[str] = None                 # PREFIX.elements.tsv with --curve_elements


def plan(args) -> Optional[CurvePlan]:
    """--curves, --curve_bins and --curve_elements, or None without --curves.  Every refusal is made here (sys.exit), before the model is read or the
    GPU is touched."""
    prefix = getattr(args, "curves", None)
    bins = getattr(args, "curve_bins", None)
    elements = bool(getattr(args, "curve_elements", False))
    if prefix is None:
        if elements:
            sys.exit("--curve_elements needs --curves")
        if bins is not None:
            sys.exit("--curve_bins needs --curves")
        return None
    bins = DEFAULT_BINS if bins is None else bins
    if not MIN_BINS <= bins <= MAX_BINS:
        sys.exit(f"--curve_bins must lie in {MIN_BINS}..{MAX_BINS}, not {bins}")
    # (unlike the other reports: a prefix that exists as a directory passes, and only the FASTA inputs are guarded)
    paths = plan_prefix("--curves", prefix, (".bases.tsv", ".rows.tsv") + ((".elements.tsv",) if elements else ()), args,
                        "the histograms are summed on the rank that holds the merged probabilities", refuse_directory=False,
                        other_inputs=())
    return CurvePlan(prefix, int(bins), *paths)


def from_plan(p: CurvePlan, classes: int, annotation) -> "Curves":
    return Curves(classes, p.bins, p.elements_path is not None)


def bin_index(p: np.ndarray, bins: int) -> np.ndarray:
    """The bin of float32 probabilities in [0, 1]: one float32 product, truncated, the last bin closed at 1."""
    k = (np.asarray(p, np.float32) * np.float32(bins)).astype(np.int64)
    return np.minimum(k, bins - 1)


def reference_hist(probs: np.ndarray, truth: np.ndarray, bins: int):
    """dgrp_prob_hist_batch's statement in numpy for the bases of any number of records laid back to back: `probs` float32 [n, C],
    `truth` int8 [n] -> (hist int64 [C, 2, bins], flag).  hist[c, 1] counts the bases whose truth is c, hist[c, 0] the others.  A
    NaN or a probability outside [0, 1] raises the flag and is not counted; a truth outside 0..C-1 raises it and none of the base's
    elements is."""
    probs = np.asarray(probs, np.float32)
    n, C = probs.shape
    truth = np.asarray(truth).astype(np.int64).reshape(n)
    hist = np.zeros((C, 2, bins), np.int64)
    with np.errstate(invalid="ignore"):
        good_t = (truth >= 0) & (truth < C)
        good_p = (probs >= 0) & (probs <= 1)                     # (NaN compares false; -0.0 compares equal to 0)
        good = good_p & good_t[:, None]
        k = bin_index(np.where(good, probs, np.float32(0)), bins)
    for c in range(C):
        for side in (0, 1):
            sel = good[:, c] & ((truth == c) == bool(side))
            hist[c, side] = np.bincount(k[sel, c], minlength=bins)
    return hist, int(not good.all())


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def base_curves(hist: np.ndarray) -> Dict[str, np.ndarray]:
    """TP, FP, FN, TN (int64 [C, bins]) and TPR, FPR, PPV, F1 (float64, NaN where a denominator is 0) of every class and threshold
    index k: the base is called c when its bin is >= k."""
    hist = np.asarray(hist, np.int64)
    tp = hist[:, 1, ::-1].cumsum(axis=1)[:, ::-1]
    fp = hist[:, 0, ::-1].cumsum(axis=1)[:, ::-1]
    fn, tn = tp[:, :1] - tp, fp[:, :1] - fp
    return dict(TP=tp, FP=fp, FN=fn, TN=tn, TPR=_ratio(tp, tp + fn), FPR=_ratio(fp, fp + tn), PPV=_ratio(tp, tp + fp),
                F1=_ratio(2 * tp, 2 * tp + fp + fn))


def summaries(hist: np.ndarray) -> Dict[str, List[float]]:
    """Per class: auroc (trapezoids over the (FPR, TPR) points from (0, 0) at k = bins down to k = 0), average_precision (sum over
    k of (TPR[k] - TPR[k+1]) * PPV[k], TPR[bins] = 0, thresholds that call nothing skipped), best_f1 and best_threshold (the lowest
    k / bins that reaches it).  auroc is NaN where a class has no positive or no negative base, average_precision where it has no
    positive one, best_f1 and best_threshold where F1 is NaN at every threshold (no base at all)."""
    hist = np.asarray(hist, np.int64)
    C, _two, bins = hist.shape
    cv = base_curves(hist)
    out = dict(auroc=[], average_precision=[], best_f1=[], best_threshold=[])
    for c in range(C):
        tp = [int(x) for x in cv["TP"][c]] + [0]
        fp = [int(x) for x in cv["FP"][c]] + [0]
        pos, neg = tp[0], fp[0]
        # twice the area in units of 1 / (pos * neg): an exact integer
        area2 = sum((fp[k] - fp[k + 1]) * (tp[k] + tp[k + 1]) for k in range(bins))
        out["auroc"].append(area2 / (2 * pos * neg) if pos and neg else float("nan"))
        if pos:
            terms = [(tp[k] - tp[k + 1]) * tp[k] / (tp[k] + fp[k]) for k in range(bins) if tp[k] + fp[k]]
            out["average_precision"].append(math.fsum(terms) / pos)
        else:
            out["average_precision"].append(float("nan"))
        f1 = cv["F1"][c]
        if np.isnan(f1).all():
            out["best_f1"].append(float("nan"))
            out["best_threshold"].append(float("nan"))
        else:
            k = int(np.nanargmax(f1))                            # (the first maximum: the lowest k on a tie)
            out["best_f1"].append(float(f1[k]))
            out["best_threshold"].append(k / bins)
    return out


def row_scores_of(scores: np.ndarray) -> np.ndarray:
    """The integer 0..1000 `bed.py` prints for each scored row (pipeline.ROW_SCORE_DTYPE, bases > 0)."""
    from .bed import _half_up
    return np.fromiter((_half_up(int(s), int(b) << 24, 1000) for s, b in zip(scores["sum"], scores["bases"])), np.int64, count=len(scores))


def row_counts(labels: np.ndarray, score: np.ndarray, kept: np.ndarray, supported: np.ndarray, classes: int):
    """Rows by class and score: -> (kept rows, supported rows), int64 [classes, 1001] each, NOT yet cumulated.  `kept`: the row has a
    base inside its record; `supported`: it is kept and passes the --min_overlap rule."""
    seg = np.zeros((classes, SCORES), np.int64)
    sup = np.zeros((classes, SCORES), np.int64)
    np.add.at(seg, (labels[kept], score[kept]), 1)
    np.add.at(sup, (labels[supported], score[supported]), 1)
    return seg, sup


def row_curves(seg: np.ndarray, sup: np.ndarray):
    """segments_at[c, m] and supported_at[c, m]: the rows of `row_counts` with score >= m."""
    at = lambda x: np.asarray(x, np.int64)[:, ::-1].cumsum(axis=1)[:, ::-1]
    return at(seg), at(sup)


def need_of(theta: float, clen: np.ndarray) -> np.ndarray:
    """The bases an element of clipped length clen needs: ceil(theta * float64(clen)), 0 where clen is 0.  For integer hits,
    hits >= need is `evaluation.count`'s float64(hits) >= theta * float64(clen): an integer is at least x exactly when it is at
    least ceil(x), and both sides are exact in float64."""
    clen = np.asarray(clen, np.int64)
    return np.where(clen > 0, np.ceil(float(theta) * clen.astype(np.float64)), 0.0).astype(np.int64)


def reference_detect(origins, lengths, pred_rows, pred_scores, true_rows, need):
    """dgrp_paint_row_keys_batch and dgrp_row_detect_batch in numpy for a list of records (record r: `lengths[r]` bases from the
    coordinate `origins[r]`): pred_rows[r] its predicted rows (SEGMENT_DTYPE fields, ascending, not overlapping), pred_scores[r]
    their BED scores 0..1000, true_rows[r] its annotation rows, need[r] the bases each needs.
    -> ([key track uint16 per record], detection scores int32 of all annotation rows, record after record).
    key = label << 10 | score on every base of a predicted row's clipped span, 0 elsewhere.  The detection score of annotation
    row j with label L and clipped span S is the largest m in 0..1000 with #{b in S: L << 10 | m <= key[b] < (L + 1) << 10} >=
    need[j], -1 where there is none, where need[j] <= 0 or where S is empty -- taken by trying every m."""
    keys, out = [], []
    for r in range(len(lengths)):
        n, o = int(lengths[r]), int(origins[r])
        key = np.zeros(n, np.uint16)
        for row, sc in zip(pred_rows[r], pred_scores[r]):
            a, e = min(max(int(row["start"]) - o, 0), n), min(max(int(row["end"]) - o, 0), n)
            if e > a:
                key[a:e] = int(row["label"]) << 10 | int(sc)
        keys.append(key)
        t = true_rows[r]
        nd = np.asarray(need[r], np.int64).reshape(len(t))
        a = np.clip(np.asarray(t["start"], np.int64) - o, 0, n)
        e = np.maximum(np.clip(np.asarray(t["end"], np.int64) - o, 0, n), a)
        d = np.full(len(t), -1, np.int32)
        labels = np.asarray(t["label"], np.int64)
        live = (e > a) & (nd > 0)
        for lab in np.unique(labels[live]):
            sel = np.flatnonzero(live & (labels == lab))
            k = key.astype(np.int64)
            for m in range(SCORES):
                cs = np.concatenate([[0], np.cumsum((k >= (lab << 10 | m)) & (k < (lab + 1) << 10))])
                ok = cs[e[sel]] - cs[a[sel]] >= nd[sel]
                d[sel[ok]] = m
        out.append(d)
    return keys, (np.concatenate(out) if out else np.zeros(0, np.int32))


def element_curves(det: np.ndarray, seg: np.ndarray, sup: np.ndarray) -> Dict[str, np.ndarray]:
    """Per class and m = 0..1000 from det (int64 [C, 1002]: the elements with a base inside their record by label and detection
    score + 1) and `row_counts`: elements [C], found (detection score >= m), segments, supported (int64 [C, 1001]) and recall =
    found / elements, precision = supported / segments, F1 = 2 P R / (P + R) (float64, NaN where a denominator is 0)."""
    det = np.asarray(det, np.int64)
    elements = det.sum(axis=1)
    found = det[:, :0:-1].cumsum(axis=1)[:, ::-1]
    seg_at, sup_at = row_curves(seg, sup)
    recall, prec = _ratio(found, elements[:, None]), _ratio(sup_at, seg_at)
    with np.errstate(invalid="ignore"):
        f1 = _ratio(2 * prec * recall, prec + recall)
    f1[np.isnan(prec) | np.isnan(recall)] = np.nan
    return dict(elements=elements, found=found, recall=recall, segments=seg_at, supported=sup_at, precision=prec, F1=f1)


def element_summary(det: np.ndarray, seg: np.ndarray, sup: np.ndarray) -> Dict[str, List[float]]:
    """Per class: recall_at_0, best_f1 and best_min_score (the lowest m that reaches it; NaN where F1 is NaN at every m)."""
    cv = element_curves(det, seg, sup)
    out = dict(recall_at_0=[], best_f1=[], best_min_score=[])
    for c in range(cv["F1"].shape[0]):
        f1 = cv["F1"][c]
        out["recall_at_0"].append(float(cv["recall"][c, 0]))
        if np.isnan(f1).all():
            out["best_f1"].append(float("nan"))
            out["best_min_score"].append(float("nan"))
        else:
            m = int(np.nanargmax(f1))                            # (the first maximum: the lowest m on a tie)
            out["best_f1"].append(float(f1[m]))
            out["best_min_score"].append(m)
    return out


_f = lambda x: repr(float(x))                                    # floats as `evaluate` prints them ('nan' for NaN)


def bases_tsv(hist: np.ndarray) -> str:
    hist = np.asarray(hist, np.int64)
    C, _two, bins = hist.shape
    cv = base_curves(hist)
    lines = ["#" + "\t".join(BASES_HEADER)]
    for c in range(C):
        for k in range(bins):
            lines.append("\t".join([str(c), repr(k / bins)] + [str(int(cv[x][c, k])) for x in ("TP", "FP", "FN", "TN")]
                                   + [_f(cv[x][c, k]) for x in ("TPR", "FPR", "PPV", "F1")]))
    return "\n".join(lines) + "\n"


def rows_tsv(seg: np.ndarray, sup: np.ndarray) -> str:
    seg_at, sup_at = row_curves(seg, sup)
    prec = _ratio(sup_at, seg_at)
    lines = ["#" + "\t".join(ROWS_HEADER)]
    for c in range(1, seg_at.shape[0]):
        for m in range(SCORES):
            lines.append("\t".join([str(c), str(m), str(int(seg_at[c, m])), str(int(sup_at[c, m])), _f(prec[c, m])]))
    return "\n".join(lines) + "\n"


def elements_tsv(det: np.ndarray, seg: np.ndarray, sup: np.ndarray) -> str:
    cv = element_curves(det, seg, sup)
    lines = ["#" + "\t".join(ELEMENTS_HEADER)]
    for c in range(1, cv["found"].shape[0]):
        for m in range(SCORES):
            lines.append("\t".join([str(c), str(m), str(int(cv["elements"][c])), str(int(cv["found"][c, m])), _f(cv["recall"][c, m]),
                                    str(int(cv["segments"][c, m])), str(int(cv["supported"][c, m])), _f(cv["precision"][c, m]),
                                    _f(cv["F1"][c, m])]))
    return "\n".join(lines) + "\n"


class Curves:
    """The counts of one `evaluate --curves` run, summed over its work items; with `elements` (--curve_elements) also `det`, the
    elements by label and detection score + 1."""
    key = "curves"

    def __init__(self, classes: int, bins: int = DEFAULT_BINS, elements: bool = False):
        if not MIN_BINS <= int(bins) <= MAX_BINS:
            raise ValueError(f"bins must lie in {MIN_BINS}..{MAX_BINS}, not {bins}")
        self.C, self.bins = int(classes), int(bins)
        self.hist = np.zeros((self.C, 2, self.bins), np.int64)
        self.seg = np.zeros((self.C, SCORES), np.int64)
        self.sup = np.zeros((self.C, SCORES), np.int64)
        self.elements = bool(elements)
        self.det = np.zeros((self.C, SCORES + 1), np.int64)

    def bind(self, annotation, classes: int) -> None:
        if self.C != classes:
            raise ValueError(f"curves of {self.C} classes for a model of {classes}")

    def probe(self, it):
        """The item's truth painted, every probability counted by class and truth (dgrp_prob_hist_batch) -> (hist [C, 2, bins],
        flag) as host arrays."""
        import torch

        from ._lib import check, lib
        from .evaluation import paint
        from .pipeline import stream_ptr
        L, C, bins, dev = lib(), it.C, self.bins, it.dev
        work = torch.empty(max(int(L.dgrp_eval_workspace_bytes(it.nrec, int(it.t_off[-1]))), int(L.dgrp_prob_hist_workspace_bytes(it.nrec, C, bins))),
                           dtype=torch.uint8, device=dev)
        d_true = paint(it.ln, it.org, it.off, it.t_off, it.d_trows, work, dev)
        d_hist = torch.empty((C, 2, bins), dtype=torch.int64, device=dev)
        d_bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(L.dgrp_prob_hist_batch(it.d_probs.data_ptr(), C, it.nrec, it.row0.ctypes.data, it.ln.ctypes.data, d_true.data_ptr(),
                                     it.off.ctypes.data, bins, d_hist.data_ptr(), d_bad.data_ptr(), work.data_ptr(), work.numel(), stream_ptr()),
              "dgrp_prob_hist_batch")
        return d_hist.cpu().numpy(), int(d_bad.item())

    def add(self, it, probed) -> None:
        """A work item: the probe's histogram summed, the predicted rows counted by class and BED score, and with elements `_detect`."""
        from .evaluation import naming
        if probed is not None:
            hist, flag = probed
            if flag:
                raise ValueError(f"a probability outside [0, 1] or a label outside 0..{it.C - 1} reached the probability histogram "
                                 f"({naming(it.names)})")
            self.hist += hist
        if it.p_flat.size:
            if it.scores is None or len(it.scores) != len(it.p_flat):
                raise ValueError(f"{len(it.p_flat)} predicted rows but {0 if it.scores is None else len(it.scores)} scores")
            sc = np.zeros(len(it.p_flat), np.int64)
            sc[it.kept] = row_scores_of(it.scores[it.kept])
            seg, sup = row_counts(it.p_flat["label"].astype(np.int64), sc, it.kept, it.good, it.C)
            self.seg += seg
            self.sup += sup
        if self.elements and it.t_flat.size:
            self._detect(it)

    def _detect(self, it) -> None:
        """The element curves' share of a work item: the predicted rows painted as keys (label << 10 | BED score) on a zeroed
        uint16 track (dgrp_paint_row_keys_batch), the detection score of every annotation row against it (dgrp_row_detect_batch),
        counted into `det` by label and score + 1 for the rows with a base inside their record."""
        import torch

        from ._lib import check, lib
        from .evaluation import naming
        from .pipeline import ROW_SCORE_DTYPE
        L, dev, s, nrec = lib(), it.dev, it.stream, it.nrec
        off, ln, org = it.off.ctypes.data, it.ln.ctypes.data, it.org.ctypes.data
        wb = int(L.dgrp_row_detect_workspace_bytes(nrec, max(int(it.t_off[-1]), int(it.p_off[-1]))))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        d_keys = torch.zeros(it.n, dtype=torch.int16, device=dev)                  # (16-bit keys; the sign of the type is not read)
        if it.d_prows is not None:
            sc = np.ascontiguousarray(it.scores, ROW_SCORE_DTYPE)
            d_sc = torch.from_numpy(sc.view(np.uint8)).to(dev)
            rc = L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), nrec, off, ln, org, it.d_prows.data_ptr(), it.p_off.ctypes.data,
                                             d_sc.data_ptr(), work.data_ptr(), wb, s)
            if rc != 0:
                raise ValueError("the predicted rows of {} cannot be painted by score: {}".format(
                    naming(it.names), L.dgrp_last_error().decode("utf-8", "replace")))
        d_need = torch.from_numpy(need_of(it.theta, it.t_clen)).to(dev)
        d_det = torch.empty(len(it.t_flat), dtype=torch.int32, device=dev)
        check(L.dgrp_row_detect_batch(d_keys.data_ptr(), nrec, off, ln, org, it.d_trows.data_ptr(), it.t_off.ctypes.data,
                                      d_need.data_ptr(), d_det.data_ptr(), work.data_ptr(), wb, s), "dgrp_row_detect_batch")
        det = d_det.cpu().numpy().astype(np.int64)
        np.add.at(self.det, (it.t_flat["label"].astype(np.int64)[it.ok], det[it.ok] + 1), 1)

    def element_curves(self) -> Dict[str, np.ndarray]:
        return element_curves(self.det, self.seg, self.sup)

    def elements_tsv(self) -> str:
        return elements_tsv(self.det, self.seg, self.sup)

    def summary(self) -> Dict[str, object]:
        """The `curves` key of the JSON report (NaN as None)."""
        num = lambda x: None if math.isnan(x) else x
        out: Dict[str, object] = dict(bins=self.bins)
        out.update({k: [num(x) for x in v] for k, v in summaries(self.hist).items()})
        if self.elements:
            out["elements"] = {k: [num(x) for x in v] for k, v in element_summary(self.det, self.seg, self.sup).items()}
        return out

    def write(self, p: CurvePlan, log) -> None:
        """The two files, with elements the three, staged: a failure leaves none of them, nor a temporary file."""
        texts, paths = [bases_tsv(self.hist), rows_tsv(self.seg, self.sup)], [p.bases_path, p.rows_path]
        if self.elements:
            if p.elements_path is None:
                raise ValueError("element curves were counted but the plan names no PREFIX.elements.tsv")
            texts.append(self.elements_tsv())
            paths.append(p.elements_path)
        write_texts(log, p.prefix, "--curves", paths, texts)
