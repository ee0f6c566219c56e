"""`evaluate --strata`: where a model loses elements -- recall split by the divergence of an element from its consensus and by its
length, from integer counts alone.

The stratum of an annotation row is div_bin * n_len + len_bin.  The divergence bins are [0, e1), [e1, e2), ..., [ek, inf) over the
row's millidiv (tenths of a percent, from the RepeatMasker listing: annotation.millidiv_of_line) plus a last bin `NA` for -1, "not
stated" -- every row of a table annotation.  The length bins are taken on the row's own end - start, not on its clipped length.  A
value equal to an edge goes to the upper bin.  The rows are few: the binning is numpy on the host.

Element counts.  `Accumulator.add` already has, per annotation row, the clipped length, the hits against the predicted labels and
the --min_overlap rule; they are grouped here by (label, stratum).  Overlapping annotation rows count twice.

Base counts.  The device paints the truth as keys, label << 8 | stratum, the smallest key winning a base (dgrp_paint_strata_batch;
`reference_keys` is its numpy statement) and counts the probability of the TRUE class of every annotated base into `bins` bins per
(class, stratum) (dgrp_prob_hist_strata_batch; `reference_strata_hist`): every base once, under the element that won it.

ON THE DEVICE (`Strata`, a report of deepgrp_amd/evaluation.py).  `Strata.probe` does the base counts on the worker's stream while
the runner holds the merged probabilities of a work item; `Strata.add` sums them and does the element counts.

Everything else here is numpy over int64; the same counts give the same file bytes."""
from __future__ import annotations

import math
import re
import sys
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from .outfiles import plan_prefix, write_texts

MIN_BINS, MAX_BINS, DEFAULT_BINS = 2, 1000, 100
MAX_EDGES, MAX_STRATA = 15, 256
DEFAULT_DIV, DEFAULT_LEN = "5,10,15,20,25,30", "100,300,1000,3000"
NONE = 0xFFFFFFFF                                   # the key of a base that no row covers
STRATA_HEADER = ("class", "divergence", "length", "elements", "found", "recall", "element_bases", "element_hits", "base_recall")
BASES_HEADER = ("class", "divergence", "length", "threshold", "TP", "FN", "TPR")
STRATA_COMMENT = ("# element_bases and element_hits are sums over elements of the clipped length and of the hits: overlapping "
                  "annotation rows count twice")
_PERCENT = re.compile(r"([0-9]{1,6})(?:\.([0-9]))?")
_BASES = re.compile(r"[0-9]{1,12}")


class StrataPlan(NamedTuple):
    prefix: str
    div_edges: tuple                                # tenths of a percent, ascending
    len_edges: tuple                                # bases, ascending
    bins: int
    strata_path: str
    bases_path: str


def _edges(flag: str, text: str, pattern, value) -> tuple:
    parts = text.split(",")
    if not 1 <= len(parts) <= MAX_EDGES:
        sys.exit(f"{flag} takes 1..{MAX_EDGES} edges, not {len(parts)}")
    out = []
    for part in parts:
        m = pattern.fullmatch(part.strip())
        if m is None:
            sys.exit(f"{flag}: {part!r} is not an edge ({'percent, one decimal at most' if pattern is _PERCENT else 'bases'})")
        out.append(value(m))
    if out[0] <= 0 or any(b <= a for a, b in zip(out, out[1:])):
        sys.exit(f"{flag}: the edges must be positive and ascend, not {text!r}")
    return tuple(out)


def plan(args) -> Optional[StrataPlan]:
    """--strata, --strata_div, --strata_len and --strata_bins, or None without --strata.  Every refusal is made here (sys.exit),
    before the model is read or the GPU is touched."""
    prefix = getattr(args, "strata", None)
    div, length, bins = (getattr(args, k, None) for k in ("strata_div", "strata_len", "strata_bins"))
    if prefix is None:
        for flag, v in (("--strata_div", div), ("--strata_len", length), ("--strata_bins", bins)):
            if v is not None:
                sys.exit(f"{flag} needs --strata")
        return None
    bins = DEFAULT_BINS if bins is None else bins
    if not MIN_BINS <= bins <= MAX_BINS:
        sys.exit(f"--strata_bins must lie in {MIN_BINS}..{MAX_BINS}, not {bins}")
    div_edges = _edges("--strata_div", DEFAULT_DIV if div is None else div, _PERCENT,
                       lambda m: 10 * int(m.group(1)) + int(m.group(2) or 0))
    len_edges = _edges("--strata_len", DEFAULT_LEN if length is None else length, _BASES, lambda m: int(m.group(0)))
    n = (len(div_edges) + 2) * (len(len_edges) + 1)
    if n > MAX_STRATA:
        sys.exit(f"--strata: {len(div_edges) + 2} divergence bins x {len(len_edges) + 1} length bins are {n} strata, more than {MAX_STRATA}")
    paths = plan_prefix("--strata", prefix, (".strata.tsv", ".strata.bases.tsv"), args,
                        "the histograms are summed on the rank that holds the merged probabilities")
    return StrataPlan(prefix, div_edges, len_edges, int(bins), *paths)


def from_plan(p: StrataPlan, classes: int, annotation) -> "Strata":
    return Strata(classes, p.div_edges, p.len_edges, p.bins)


def _percent(e: int) -> str:
    return str(e // 10) if e % 10 == 0 else f"{e // 10}.{e % 10}"


def _labels(edges: Sequence[int], show) -> List[str]:
    lo = ["0"] + [show(e) for e in edges]
    return [f"{a}-{b}" for a, b in zip(lo, lo[1:])] + [lo[-1] + "+"]


def div_labels(div_edges: Sequence[int]) -> List[str]:
    """`0-5`, `5-10`, ..., `30+`, `NA`"""
    return _labels(div_edges, _percent) + ["NA"]


def len_labels(len_edges: Sequence[int]) -> List[str]:
    """`0-100`, ..., `3000+`"""
    return _labels(len_edges, str)


def div_bin(millidiv, div_edges: Sequence[int]) -> np.ndarray:
    """[0, e1) -> 0, ..., [ek, inf) -> k, -1 (not stated) -> k + 1; a value equal to an edge goes to the upper bin."""
    v = np.asarray(millidiv, np.int64)
    return np.where(v < 0, len(div_edges) + 1, np.searchsorted(np.asarray(div_edges, np.int64), v, side="right")).astype(np.int64)


def len_bin(length, len_edges: Sequence[int]) -> np.ndarray:
    return np.searchsorted(np.asarray(len_edges, np.int64), np.asarray(length, np.int64), side="right").astype(np.int64)


def strata_of(rows: np.ndarray, millidiv, div_edges: Sequence[int], len_edges: Sequence[int]) -> np.ndarray:
    """The stratum (uint8) of every row: div_bin * n_len + len_bin, the length being the row's own end - start.  millidiv None:
    -1 everywhere (a table annotation)."""
    n = len(rows)
    md = np.full(n, -1, np.int64) if millidiv is None else np.asarray(millidiv, np.int64).reshape(n)
    length = np.asarray(rows["end"], np.int64) - np.asarray(rows["start"], np.int64)
    return (div_bin(md, div_edges) * (len(len_edges) + 1) + len_bin(length, len_edges)).astype(np.uint8)


def reference_keys(origins, lengths, rows, strata) -> List[np.ndarray]:
    """dgrp_paint_strata_batch in numpy for a list of records (record r: `lengths[r]` bases from the coordinate `origins[r]`, rows[r]
    its rows with SEGMENT_DTYPE fields, strata[r] their strata): -> [key track uint32 per record], 0xFFFFFFFF where no row covers a
    base, else the smallest label << 8 | stratum among the rows that do."""
    out = []
    for r in range(len(lengths)):
        n, o = int(lengths[r]), int(origins[r])
        key = np.full(n, NONE, np.uint32)
        for row, s in zip(rows[r], strata[r]):
            a, e = min(max(int(row["start"]) - o, 0), n), min(max(int(row["end"]) - o, 0), n)
            if e > a:
                key[a:e] = np.minimum(key[a:e], np.uint32(int(row["label"]) << 8 | int(s)))
        out.append(key)
    return out


def reference_strata_hist(probs: np.ndarray, keys: np.ndarray, S: int, bins: int):
    """dgrp_prob_hist_strata_batch in numpy for the bases of any number of records laid back to back: `probs` float32 [n, C], `keys`
    uint32 [n] -> (hist int64 [C, S, bins], flag).  A base whose key is not 0xFFFFFFFF counts P[b, key >> 8] into hist[key >> 8,
    key & 255] by curves.bin_index; a class >= C, a stratum >= S, a NaN or a probability outside [0, 1] raises the flag and the
    base is not counted."""
    from .curves import bin_index
    probs = np.asarray(probs, np.float32)
    n, C = probs.shape
    keys = np.asarray(keys, np.uint32).reshape(n)
    live = keys != np.uint32(NONE)
    t, s = (keys >> np.uint32(8)).astype(np.int64), (keys & np.uint32(255)).astype(np.int64)
    good = live & (t < C) & (s < S)
    p = probs[np.arange(n), np.where(good, t, 0)]
    with np.errstate(invalid="ignore"):
        ok = good & (p >= 0) & (p <= 1)                              # (NaN compares false; -0.0 compares equal to 0)
        k = bin_index(np.where(ok, p, np.float32(0)), bins)
    hist = np.zeros((C, S, bins), np.int64)
    np.add.at(hist, (t[ok], s[ok], k[ok]), 1)
    return hist, int(bool((live & ~ok).any()))


def _ratio(num, den) -> np.ndarray:
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


_f = lambda x: repr(float(x))                                        # floats as `evaluate` prints them ('nan' for NaN)


def strata_tsv(counts: np.ndarray, div_edges: Sequence[int], len_edges: Sequence[int]) -> str:
    """PREFIX.strata.tsv of counts int64 [4, C, S] (elements, found, element_bases, element_hits): the comment, the header, one line
    per class >= 1 and stratum, then per class its margins -- `*` over the divergence for every length bin, `*` over the length
    for every divergence bin, and `*` over both."""
    dl, ll = div_labels(div_edges), len_labels(len_edges)
    counts = np.asarray(counts, np.int64)
    C = counts.shape[1]
    x = counts.reshape(4, C, len(dl), len(ll))

    def line(c, d, l, v):
        el, fo, eb, eh = (int(y) for y in v)
        return "\t".join([str(c), d, l, str(el), str(fo), _f(_ratio(fo, el)), str(eb), str(eh), _f(_ratio(eh, eb))])
    lines = [STRATA_COMMENT, "#" + "\t".join(STRATA_HEADER)]
    for c in range(1, C):
        for i, d in enumerate(dl):
            for j, l in enumerate(ll):
                lines.append(line(c, d, l, x[:, c, i, j]))
    for c in range(1, C):
        for j, l in enumerate(ll):
            lines.append(line(c, "*", l, x[:, c, :, j].sum(axis=1)))
        for i, d in enumerate(dl):
            lines.append(line(c, d, "*", x[:, c, i, :].sum(axis=1)))
        lines.append(line(c, "*", "*", x[:, c].sum(axis=(1, 2))))
    return "\n".join(lines) + "\n"


def bases_tsv(hist: np.ndarray, div_edges: Sequence[int], len_edges: Sequence[int]) -> str:
    """PREFIX.strata.bases.tsv of hist int64 [C, S, bins]: per class >= 1, stratum and threshold k / bins the annotated bases whose
    winning element lies in the stratum (each base once) with their true class's probability in a bin >= k (TP), the others (FN)
    and TPR = TP / (TP + FN) -- the suffix sums curves.base_curves forms."""
    dl, ll = div_labels(div_edges), len_labels(len_edges)
    hist = np.asarray(hist, np.int64)
    C, S, bins = hist.shape
    tp = hist[:, :, ::-1].cumsum(axis=2)[:, :, ::-1]
    fn = tp[:, :, :1] - tp
    tpr = _ratio(tp, tp + fn)
    lines = ["#" + "\t".join(BASES_HEADER)]
    for c in range(1, C):
        for s in range(S):
            d, l = dl[s // len(ll)], ll[s % len(ll)]
            for k in range(bins):
                lines.append("\t".join([str(c), d, l, repr(k / bins), str(int(tp[c, s, k])), str(int(fn[c, s, k])), _f(tpr[c, s, k])]))
    return "\n".join(lines) + "\n"


class Strata:
    """The counts of one `evaluate --strata` run, summed over its work items: `counts` int64 [4, C, S] (elements, found,
    element_bases, element_hits by label and stratum) and `hist` int64 [C, S, bins]."""
    key = "strata"

    def __init__(self, classes: int, div_edges: Sequence[int], len_edges: Sequence[int], bins: int = DEFAULT_BINS):
        if not MIN_BINS <= int(bins) <= MAX_BINS:
            raise ValueError(f"bins must lie in {MIN_BINS}..{MAX_BINS}, not {bins}")
        self.C, self.bins = int(classes), int(bins)
        self.div_edges, self.len_edges = tuple(int(e) for e in div_edges), tuple(int(e) for e in len_edges)
        self.n_div, self.n_len = len(self.div_edges) + 2, len(self.len_edges) + 1
        self.S = self.n_div * self.n_len
        if not 1 <= self.S <= MAX_STRATA:
            raise ValueError(f"{self.S} strata: at most {MAX_STRATA}")
        self.counts = np.zeros((4, self.C, self.S), np.int64)
        self.hist = np.zeros((self.C, self.S, self.bins), np.int64)
        self.millidiv = None                            # {contig: the millidiv of its rows} once bound to a listing

    def bind(self, annotation, classes: int) -> None:
        if self.C != classes:
            raise ValueError(f"strata of {self.C} classes for a model of {classes}")
        self.millidiv = getattr(annotation, "millidiv", None)

    def strata_of(self, rows: np.ndarray, millidiv) -> np.ndarray:
        return strata_of(rows, millidiv, self.div_edges, self.len_edges)

    def row_strata(self, name: str, rows: np.ndarray) -> np.ndarray:
        """The stratum of every annotation row of contig `name`: its millidiv travels beside the rows (annotation.Rows.millidiv;
        a table has none: -1 everywhere)."""
        return self.strata_of(rows, None if self.millidiv is None or name not in self.millidiv else self.millidiv[name])

    def probe(self, it):
        """The item's truth painted as keys (dgrp_paint_strata_batch), the true class's probability counted by them
        (dgrp_prob_hist_strata_batch) -> (hist [C, S, bins], flag) as host arrays."""
        import torch

        from ._lib import check, lib
        from .pipeline import stream_ptr
        L, C, dev, nrec = lib(), it.C, it.dev, it.nrec
        off, ln, org = it.off.ctypes.data, it.ln.ctypes.data, it.org.ctypes.data
        d_st = torch.from_numpy(np.concatenate([self.row_strata(nm, t) for nm, t in zip(it.names, it.tr)])).to(dev) if int(it.t_off[-1]) else None
        work = torch.empty(max(int(L.dgrp_eval_workspace_bytes(nrec, int(it.t_off[-1]))), int(L.dgrp_prob_hist_strata_workspace_bytes(nrec)), 1),
                           dtype=torch.uint8, device=dev)
        d_keys = torch.empty(int(it.off[-1]), dtype=torch.int32, device=dev)      # (32-bit keys; the sign of the type is not read)
        ptr = lambda t: None if t is None else t.data_ptr()
        check(L.dgrp_paint_strata_batch(d_keys.data_ptr(), nrec, off, ln, org, ptr(it.d_trows), it.t_off.ctypes.data, ptr(d_st),
                                        work.data_ptr(), work.numel(), stream_ptr()), "dgrp_paint_strata_batch")
        d_hist = torch.empty((C, self.S, self.bins), dtype=torch.int64, device=dev)
        d_bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(L.dgrp_prob_hist_strata_batch(it.d_probs.data_ptr(), C, nrec, it.row0.ctypes.data, ln, d_keys.data_ptr(), off, self.S,
                                            self.bins, d_hist.data_ptr(), d_bad.data_ptr(), work.data_ptr(), work.numel(), stream_ptr()),
              "dgrp_prob_hist_strata_batch")
        return d_hist.cpu().numpy(), int(d_bad.item())

    def add(self, it, probed) -> None:
        """A work item: the probe's histogram summed, the element counts the item holds grouped by label and stratum."""
        from .evaluation import naming
        if probed is not None:
            hist, flag = probed
            if flag:
                raise ValueError(f"a probability outside [0, 1] or a key outside {it.C} classes and {self.S} strata reached the strata "
                                 f"histogram ({naming(it.names)})")
            self.hist += hist
        if it.t_flat.size:
            strata = np.concatenate([self.row_strata(nm, t) for nm, t in zip(it.names, it.tr)])
            self.count(it.t_flat["label"], strata, it.t_clen, it.ht, it.ok, it.hit)

    def count(self, labels: np.ndarray, strata: np.ndarray, clen: np.ndarray, hits: np.ndarray, ok: np.ndarray, hit: np.ndarray) -> None:
        """The annotation rows of a work item: `ok` has a base inside its record, `hit` passes the --min_overlap rule
        (evaluation.count's masks)."""
        lab, st = np.asarray(labels, np.int64), np.asarray(strata, np.int64)
        np.add.at(self.counts[0], (lab[ok], st[ok]), 1)
        np.add.at(self.counts[1], (lab[hit], st[hit]), 1)
        np.add.at(self.counts[2], (lab[ok], st[ok]), np.asarray(clen, np.int64)[ok])
        np.add.at(self.counts[3], (lab[ok], st[ok]), np.asarray(hits, np.int64)[ok])

    def summary(self) -> Dict[str, object]:
        """The `strata` key of the JSON report: the edges, and per class the recall by divergence bin and by length bin (the
        margins; NaN as None)."""
        num = lambda v: [None if math.isnan(x) else float(x) for x in v]
        x = self.counts.reshape(4, self.C, self.n_div, self.n_len)
        by_div, by_len = x.sum(axis=3), x.sum(axis=2)
        return dict(bins=self.bins, divergence_edges=[e / 10 for e in self.div_edges], length_edges=list(self.len_edges),
                    divergence_bins=div_labels(self.div_edges), length_bins=len_labels(self.len_edges),
                    recall_by_divergence=[num(_ratio(by_div[1, c], by_div[0, c])) for c in range(self.C)],
                    recall_by_length=[num(_ratio(by_len[1, c], by_len[0, c])) for c in range(self.C)])

    def write(self, p: StrataPlan, log) -> None:
        """The two files, staged: a failure leaves neither of them, nor a temporary file."""
        write_texts(log, p.prefix, "--strata", (p.strata_path, p.bases_path),
                    [strata_tsv(self.counts, self.div_edges, self.len_edges), bases_tsv(self.hist, self.div_edges, self.len_edges)])
