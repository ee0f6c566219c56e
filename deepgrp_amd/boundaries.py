"""`evaluate --boundaries`: how well a found element is delimited -- where the other track's run begins and ends against the row's
own ends, and into how many runs it falls -- from integer counts alone.

TWO VIEWS.  `element`: every annotation row against the predicted labels.  `row`: every predicted row against the truth.  In both
a row is FOUND by the --min_overlap rule `evaluate` already applies: hits >= need = ceil(min_overlap * clipped length).

PER ROW (dgrp_row_bounds_batch; `reference_bounds` is its numpy statement).  With L the row's label, [a, e) its span clipped to the
evaluated bases [o, o + n) of its record and in(b) = "the other track has L at b": hits, the runs of L under the row, the first and
last base with in(b), and lead / trail: how far L runs on in front of a and behind e - 1, at most W = --boundary_max bases and never
beyond the record.

THE RULE (dgrp_bound_hist_batch; `reference_bound_hist`).  A found row has a start offset ds and an end offset de:
    ds = first - a (at most W) where the run begins inside the row, else -lead
    de = -(e - 1 - last) (at least -W) where the run ends inside the row, else trail
so 0 is an exact edge, a positive ds a late start, a negative ds a run that begins in front of the row; a negative de an early end,
a positive de a run that goes on behind the row; +-W stands for "W or more".  A side the record clipped is not counted.  Every row
with a base inside its record counts its runs, 16 and more together.

JOINING (`--boundary_join G`, element view only).  RepeatMasker lists one element as several rows where it was interrupted or
aligned in pieces; `join_rows` makes one unit of the rows of one record and label whose gap is at most G bases.

ON THE DEVICE (`Boundaries`, a report of deepgrp_amd/evaluation.py).  `Boundaries.add` makes the two calls once per view of a work
item; only the edge-offset and fragment tables come back.  The runner and the probe are not touched.

Everything else here is numpy over int64; the same counts give the same file bytes."""
from __future__ import annotations

import sys
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from .curves import need_of
from .outfiles import plan_prefix, write_texts

MIN_W, MAX_W, DEFAULT_W = 1, 4096, 200              # --boundary_max (the library takes 0 as well)
FRAG = 17                                           # runs 0..15 and 16+
VIEWS = ("element", "row")
SIDES = ("start", "end")
WITHIN = 10
BOUND_DTYPE = np.dtype([("hits", "<i8"), ("runs", "<i8"), ("first", "<i8"), ("last", "<i8"), ("lead", "<i4"), ("trail", "<i4")])
COMMENT = ("# offset: of a found row (hits >= ceil(min_overlap * clipped length)), where the other track's run of the row's class "
           "begins (side start) and ends (side end) against the row's own first and last base, in bases: 0 exact; start > 0 begins "
           "late, start < 0 begins in front of the row; end < 0 ends early, end > 0 goes on behind the row; +-{W} stands for {W} or "
           "more; a side the record clipped is not counted{join}")
HEADER = ("view", "class", "side", "offset", "count", "share")
FRAG_HEADER = ("view", "class", "runs", "count", "share")


class BoundaryPlan(NamedTuple):
    prefix: str
    W: int
    join: Optional[int]
    edges_path: str
    fragments_path: str


def plan(args) -> Optional[BoundaryPlan]:
    """--boundaries, --boundary_max and --boundary_join, or None without --boundaries.  Every refusal is made here (sys.exit),
    before the model is read or the GPU is touched."""
    prefix = getattr(args, "boundaries", None)
    W, join = getattr(args, "boundary_max", None), getattr(args, "boundary_join", None)
    if prefix is None:
        for flag, v in (("--boundary_max", W), ("--boundary_join", join)):
            if v is not None:
                sys.exit(f"{flag} needs --boundaries")
        return None
    W = DEFAULT_W if W is None else W
    if not MIN_W <= W <= MAX_W:
        sys.exit(f"--boundary_max must lie in {MIN_W}..{MAX_W}, not {W}")
    if join is not None and join < 0:
        sys.exit(f"--boundary_join must be 0 or more, not {join}")
    paths = plan_prefix("--boundaries", prefix, (".boundaries.tsv", ".fragments.tsv"), args,
                        "the counts are summed on the rank that holds the predicted rows")
    return BoundaryPlan(prefix, int(W), None if join is None else int(join), *paths)


def from_plan(p: BoundaryPlan, classes: int, annotation) -> "Boundaries":
    return Boundaries(classes, p.W, p.join)


def join_rows(rows: np.ndarray, gap: int) -> np.ndarray:
    """The rows of ONE record with those of one label whose gap is at most `gap` bases made one unit (overlapping, nested and
    abutting rows included: their gap is 0 or less): sorted by label and start, a row opens a unit when its start lies more than
    `gap` behind the largest end so far of its label.  -> SEGMENT_DTYPE units ordered by label, then start."""
    from .pipeline import SEGMENT_DTYPE
    rows = np.ascontiguousarray(rows, SEGMENT_DTYPE)
    if len(rows) < 2:
        return rows.copy()
    order = np.lexsort((rows["end"], rows["start"], rows["label"]))
    lab, st, en = (rows[k][order].astype(np.int64) for k in ("label", "start", "end"))
    big = int(en.max()) + int(gap) + 2                              # a label's ends stay below the next label's starts
    reach = np.maximum.accumulate(en + lab * big)                   # the largest end so far, restarting with every label
    opens = np.ones(len(rows), bool)
    opens[1:] = (lab[1:] != lab[:-1]) | (st[1:] + lab[1:] * big > reach[:-1] + int(gap))
    first = np.flatnonzero(opens)
    last = np.append(first[1:], len(rows)) - 1
    out = np.zeros(len(first), SEGMENT_DTYPE)
    out["start"], out["end"], out["label"] = st[first], reach[last] - lab[last] * big, lab[first]
    out["contig"] = rows["contig"][order][first]
    return out


def _clip(rows: np.ndarray, o: int, n: int):
    a = np.clip(rows["start"].astype(np.int64), o, o + n) - o
    e = np.clip(rows["end"].astype(np.int64), o, o + n) - o
    return a, np.maximum(e, a)


def reference_bounds(origins, lengths, tracks, rows, W: int) -> np.ndarray:
    """dgrp_row_bounds_batch in numpy for a list of records (record r: `lengths[r]` bases from the coordinate `origins[r]`,
    tracks[r] its int8 label track, rows[r] its rows with SEGMENT_DTYPE fields) -> BOUND_DTYPE of all rows, record after record.
    Per record and label: prefix sums of the matches and of the run starts, and the nearest match / non-match on either side of
    every base."""
    out = []
    for r in range(len(lengths)):
        n, o = int(lengths[r]), int(origins[r])
        q = np.asarray(rows[r])
        res = np.zeros(len(q), BOUND_DTYPE)
        res["first"] = res["last"] = -1
        a, e = _clip(q, o, n)
        track = np.asarray(tracks[r], np.int8)[:n]
        idx = np.arange(n, dtype=np.int64)
        for L in np.unique(q["label"][e > a]) if n else ():
            sel = np.flatnonzero((q["label"] == L) & (e > a))
            sa, se = a[sel], e[sel]
            m = track == L
            hit = np.concatenate([[0], np.cumsum(m)])
            start = m.copy()
            start[1:] &= ~m[:-1]
            starts = np.concatenate([[0], np.cumsum(start)])
            match_at_or_behind = np.minimum.accumulate(np.where(m, idx, n)[::-1])[::-1]           # smallest b' >= b with in(b'), else n
            match_at_or_before = np.maximum.accumulate(np.where(m, idx, -1))                      # largest b' <= b with in(b'), else -1
            miss_at_or_before = np.concatenate([[-1], np.maximum.accumulate(np.where(m, -1, idx))])     # [b + 1]: largest b' <= b with !in(b')
            miss_at_or_behind = np.concatenate([np.minimum.accumulate(np.where(m, n, idx)[::-1])[::-1], [n]])   # [b]: smallest b' >= b with !in(b')
            hits = hit[se] - hit[sa]
            res["hits"][sel] = hits
            res["runs"][sel] = starts[se] - starts[sa] + (m[sa] & ~start[sa])                  # a run that is cut by the row's start begins there
            res["first"][sel] = np.where(hits > 0, o + match_at_or_behind[sa], -1)
            res["last"][sel] = np.where(hits > 0, o + match_at_or_before[se - 1], -1)
            res["lead"][sel] = np.minimum(W, sa - 1 - miss_at_or_before[sa])
            res["trail"][sel] = np.minimum(W, miss_at_or_behind[se] - se)
        out.append(res)
    return np.concatenate(out) if out else np.zeros(0, BOUND_DTYPE)


def offsets_of(bounds: np.ndarray, a: np.ndarray, e: np.ndarray, W: int):
    """The rule: (ds, de) of rows with the clipped spans [a, e) in original coordinates (read for found rows only)."""
    first, last = bounds["first"].astype(np.int64), bounds["last"].astype(np.int64)
    ds = np.where(first > a, np.minimum(first - a, W), -bounds["lead"].astype(np.int64))
    de = np.where(last + 1 < e, -np.minimum(e - 1 - last, W), bounds["trail"].astype(np.int64))
    return ds, de


def reference_bound_hist(origins, lengths, rows, bounds, need, C: int, W: int):
    """dgrp_bound_hist_batch in numpy: rows[r] the rows of record r, `bounds` (BOUND_DTYPE) and `need` (int64) of all rows, record
    after record -> (frag int64 [C, 17], edge int64 [C, 2, 2W + 1], tally int64 [C, 2], flag)."""
    frag, edge, tally = np.zeros((C, FRAG), np.int64), np.zeros((C, 2, 2 * W + 1), np.int64), np.zeros((C, 2), np.int64)
    bounds, need = np.asarray(bounds), np.asarray(need, np.int64)
    flag, at = 0, 0
    for r in range(len(lengths)):
        n, o = int(lengths[r]), int(origins[r])
        q = np.asarray(rows[r])
        b, nd = bounds[at:at + len(q)], need[at:at + len(q)]
        at += len(q)
        a, e = _clip(q, o, n)
        lab = q["label"].astype(np.int64)
        inside = e > a
        ok = inside & (lab >= 0) & (lab < C)
        flag |= int((inside & ~ok).any())
        ds, de = offsets_of(b, a + o, e + o, W)
        fits = (np.abs(ds) <= W) & (np.abs(de) <= W)
        np.add.at(frag, (lab[ok], np.clip(b["runs"][ok], 0, FRAG - 1)), 1)
        found = ok & (nd > 0) & (b["hits"] >= nd)
        flag |= int((found & ~fits).any())
        found &= fits
        np.add.at(tally[:, 0], lab[found], 1)
        s_ok, e_ok = found & (q["start"] >= o), found & (q["end"] <= o + n)
        np.add.at(edge, (lab[s_ok], 0, ds[s_ok] + W), 1)
        np.add.at(edge, (lab[e_ok], 1, de[e_ok] + W), 1)
        both = s_ok & e_ok & (ds == 0) & (de == 0)
        np.add.at(tally[:, 1], lab[both], 1)
    return frag, edge, tally, flag


def _share(count: int, total: int) -> str:
    return f"{count / total:.6f}" if total else "nan"


def boundaries_tsv(edge: np.ndarray, W: int, join: Optional[int] = None) -> str:
    """PREFIX.boundaries.tsv of edge int64 [2, C, 2, 2W + 1] (view, class, side, offset + W): the rule, the header, and per view,
    class >= 1 and side the offsets with a count, ascending, with their share of that (view, class, side) to six decimals."""
    edge = np.asarray(edge, np.int64)
    note = "" if join is None else f"; element view: annotation rows of one record and class at most {join} bases apart are one unit"
    lines = [COMMENT.format(W=W, join=note), "\t".join(HEADER)]
    for v, view in enumerate(VIEWS):
        for c in range(1, edge.shape[1]):
            for s, side in enumerate(SIDES):
                total = int(edge[v, c, s].sum())
                for k in np.flatnonzero(edge[v, c, s]).tolist():
                    lines.append("\t".join([view, str(c), side, str(k - W), str(int(edge[v, c, s, k])), _share(int(edge[v, c, s, k]), total)]))
    return "\n".join(lines) + "\n"


def fragments_tsv(frag: np.ndarray) -> str:
    """PREFIX.fragments.tsv of frag int64 [2, C, 17]: per view and class >= 1 the rows with a base inside their record by the runs of
    their class under them on the other track, 0..15 and `16+`, with their share of that (view, class) (`nan` without rows)."""
    frag = np.asarray(frag, np.int64)
    lines = ["\t".join(FRAG_HEADER)]
    for v, view in enumerate(VIEWS):
        for c in range(1, frag.shape[1]):
            total = int(frag[v, c].sum())
            for k in range(FRAG):
                lines.append("\t".join([view, str(c), str(k) if k < FRAG - 1 else f"{FRAG - 1}+", str(int(frag[v, c, k])),
                                        _share(int(frag[v, c, k]), total)]))
    return "\n".join(lines) + "\n"


def _median_abs(hist: np.ndarray, W: int) -> Optional[float]:
    """The median of |offset| over the rows of hist [2W + 1] (the mean of the two middle ones for an even count), None without rows."""
    by_abs = np.zeros(W + 1, np.int64)
    np.add.at(by_abs, np.abs(np.arange(-W, W + 1)), hist)
    total = int(by_abs.sum())
    if total == 0:
        return None
    cum = np.cumsum(by_abs)
    lo = int(np.searchsorted(cum, (total + 1) // 2))                # the ((total + 1) // 2)-th smallest, counted from 1
    hi = int(np.searchsorted(cum, total // 2 + 1))
    return (lo + hi) / 2.0


class Boundaries:
    """The counts of one `evaluate --boundaries` run, summed over its work items: per view frag int64 [C, 17], edge int64
    [C, 2, 2W + 1] and tally int64 [C, 2] (found, both edges exact)."""
    key = "boundaries"

    def __init__(self, classes: int, W: int = DEFAULT_W, join: Optional[int] = None):
        if not 0 <= W <= MAX_W:
            raise ValueError(f"W must lie in 0..{MAX_W}, not {W}")
        if join is not None and join < 0:
            raise ValueError(f"join must be 0 or more, not {join}")
        self.C, self.W, self.join = int(classes), int(W), join
        self.frag = np.zeros((2, self.C, FRAG), np.int64)
        self.edge = np.zeros((2, self.C, 2, 2 * self.W + 1), np.int64)
        self.tally = np.zeros((2, self.C, 2), np.int64)

    def units(self, rows: np.ndarray) -> np.ndarray:
        """The element view's rows of one record: joined with --boundary_join, else as they are."""
        return rows if self.join is None else join_rows(rows, self.join)

    def bind(self, annotation, classes: int) -> None:
        if self.C != classes:
            raise ValueError(f"boundaries of {self.C} classes for a model of {classes}")

    def add(self, it, probed) -> None:
        """A work item, once per view: the element view takes the annotation rows (joined into units with --boundary_join, uploaded
        anew then) against the predicted labels, the row view the predicted rows against the truth.  Per view
        dgrp_row_bounds_batch, then dgrp_bound_hist_batch with need = ceil(theta * clipped length); the three tables and the flag
        are all that is copied back."""
        import torch

        from ._lib import check, lib
        from .evaluation import clipped_lengths, upload
        L, dev, s, nrec, W, C = lib(), it.dev, it.stream, it.nrec, self.W, it.C
        off, ln, org = it.off.ctypes.data, it.ln.ctypes.data, it.org.ctypes.data
        tr, t_off, d_trows = it.tr, it.t_off, it.d_trows
        if self.join is not None:
            tr = [self.units(t) for t in tr]
            t_off, _t_flat, d_trows = upload(tr, dev)
        for view, (rows, ro, d_rows, d_labels) in enumerate(((tr, t_off, d_trows, it.d_pred), (it.pr, it.p_off, it.d_prows, it.d_true))):
            nrows = int(ro[-1])
            if nrows == 0:
                continue
            clen = np.concatenate([clipped_lengths(q, int(it.org[r]), int(it.ln[r])) for r, q in enumerate(rows)])
            d_need = torch.from_numpy(need_of(it.theta, clen)).to(dev)
            wb = int(L.dgrp_row_bounds_workspace_bytes(nrec, nrows))
            work = torch.empty(max(wb, int(L.dgrp_bound_hist_workspace_bytes(nrec)), 1), dtype=torch.uint8, device=dev)
            d_bounds = torch.empty((nrows, 5), dtype=torch.int64, device=dev)          # (dgrp_row_bound: 40 bytes a row)
            check(L.dgrp_row_bounds_batch(d_labels.data_ptr(), nrec, off, ln, org, d_rows.data_ptr(), ro.ctypes.data, W,
                                          d_bounds.data_ptr(), work.data_ptr(), work.numel(), s), "dgrp_row_bounds_batch")
            d_frag = torch.empty((C, FRAG), dtype=torch.int64, device=dev)
            d_edge = torch.empty((C, 2, 2 * W + 1), dtype=torch.int64, device=dev)
            d_tally = torch.empty((C, 2), dtype=torch.int64, device=dev)
            d_bad = torch.empty(1, dtype=torch.int32, device=dev)
            check(L.dgrp_bound_hist_batch(nrec, off, ln, org, d_rows.data_ptr(), ro.ctypes.data, d_bounds.data_ptr(), d_need.data_ptr(),
                                          C, W, d_frag.data_ptr(), d_edge.data_ptr(), d_tally.data_ptr(), d_bad.data_ptr(),
                                          work.data_ptr(), work.numel(), s), "dgrp_bound_hist_batch")
            frag, edge, tally, bad = d_frag.cpu().numpy(), d_edge.cpu().numpy(), d_tally.cpu().numpy(), int(d_bad.item())
            if bad:
                raise ValueError(f"a row label outside 0..{C - 1} reached the boundary counts")
            self.count(view, frag, edge, tally)

    def count(self, view: int, frag: np.ndarray, edge: np.ndarray, tally: np.ndarray) -> None:
        self.frag[view] += frag
        self.edge[view] += edge
        self.tally[view] += tally

    def summary(self) -> Dict[str, object]:
        """The `boundaries` key of the JSON report.  Per view and class: found rows, those with an exact start / end / both, those
        within 10 bases (None where --boundary_max is 10 or less: +-W stands for more), the median |offset| per side (W stands
        for W or more), the mean runs per row (16+ taken as 16) and the share of rows with two runs or more."""
        W = self.W
        k = np.arange(FRAG, dtype=np.int64)
        near = slice(W - WITHIN, W + WITHIN + 1) if W > WITHIN else None
        views = {}
        for v, view in enumerate(VIEWS):
            out: List[Dict[str, object]] = []
            for c in range(self.C):
                e, f = self.edge[v, c], self.frag[v, c]
                rows = int(f.sum())
                out.append(dict(found=int(self.tally[v, c, 0]), start_rows=int(e[0].sum()), end_rows=int(e[1].sum()),
                                exact_start=int(e[0, W]), exact_end=int(e[1, W]), exact_both=int(self.tally[v, c, 1]),
                                within_10_start=None if near is None else int(e[0, near].sum()),
                                within_10_end=None if near is None else int(e[1, near].sum()),
                                median_abs_start=_median_abs(e[0], W), median_abs_end=_median_abs(e[1], W),
                                rows=rows, mean_runs=None if rows == 0 else float((k * f).sum()) / rows,
                                share_runs_ge_2=None if rows == 0 else int(f[2:].sum()) / rows))
            views[view] = out
        return dict(max=W, join=self.join, views=views)

    def write(self, p: BoundaryPlan, log) -> None:
        """The two files, staged: a failure leaves neither of them, nor a temporary file."""
        write_texts(log, p.prefix, "--boundaries", (p.edges_path, p.fragments_path),
                    [boundaries_tsv(self.edge, self.W, self.join), fragments_tsv(self.frag)])
