"""`evaluate --offtarget`: what the predicted repeats lie on -- the model's false positives split by what the RepeatMasker listing
says is there, from integer counts alone.

ROWS.  Every line of the listing that matches a pattern of parse_rm is a row.  A row is MODELLED when `evaluate` keeps it today (its
number is in --repeats): its key is its label, 1..63.  Every other row is UN-MODELLED: its key is 64 + the id of its class/family
token, the rank of the token among the distinct tokens of the listing in ascending byte order (annotation.read_listing(all_rows=True)).

KEY OF A BASE.  The smallest key among the rows that cover it, 0xFFFFFFFF where none does: a base under any modelled row has the label
`evaluate` paints there, an un-modelled family shows only where no modelled row covers, and among several families the first in byte
order wins (dgrp_paint_keys_batch; `reference_keys` is its numpy statement).

COUNTS.  Per work item `Offtarget.add` (a report of deepgrp_amd/evaluation.py) cross-tabulates the predicted label of every base
against its key, once for all bases and once for a track that holds only the predicted rows found unsupported
(dgrp_key_crosstab_batch; `reference_crosstab`), and takes per predicted row the bases of its clipped span under its own label,
another label, a family, nothing (dgrp_row_key_classes_batch).  The runner and the probe are not touched.

Everything here is numpy over int64; the same counts give the same file bytes."""
from __future__ import annotations

import sys
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from .outfiles import plan_prefix, write_texts

NONE = 0xFFFFFFFF                                   # the key of a base that no row covers
FIRST_FAMILY = 64                                   # keys below it are labels
MAX_FAMILIES = 16384                                # DGRP_TOKEN_MAX
BY = ("family", "class")
SCOPES = ("all", "unsupported")
COMMENT = ("# under: a base counts under the smallest key among the listing's rows that cover it -- class<L> for a row of a modelled "
           "class, which wins over every family; else the class/family token first in byte order; `none` where no row covers it")
HEADER = ("scope", "predicted", "under", "bases", "share")
ROWS_HEADER = ("class", "rows", "supported", "mostly_own", "mostly_other_class", "mostly_offtarget", "mostly_unannotated")


class OfftargetPlan(NamedTuple):
    prefix: str
    by: str
    table_path: str
    rows_path: str


def plan(args) -> Optional[OfftargetPlan]:
    """--offtarget and --offtarget_by, or None without --offtarget.  Every refusal is made here (sys.exit), before the model is read
    or the GPU is touched."""
    prefix, by = getattr(args, "offtarget", None), getattr(args, "offtarget_by", None)
    if prefix is None:
        if by is not None:
            sys.exit("--offtarget_by needs --offtarget")
        return None
    by = BY[0] if by is None else by
    if by not in BY:
        sys.exit(f"--offtarget_by: one of {', '.join(BY)}, not {by!r}")
    paths = plan_prefix("--offtarget", prefix, (".offtarget.tsv", ".offtarget.rows.tsv"), args,
                        "the counts are summed on the rank that holds the predicted rows")
    from . import annotation
    ann = getattr(args, "annotation", None)
    fmt = annotation.resolve_format(ann, getattr(args, "annotation_format", "auto")) if ann is not None else None
    if fmt in ("table", "gff3"):
        how = "a table of parse_rm" if fmt == "table" else "GFF3 numbered by name, like a table of parse_rm"
        sys.exit(f"--offtarget: {ann} is read as {how}, which holds the rows of the modelled classes only; what the other "
                 "predicted bases lie on is in the RepeatMasker listing itself: give `genome.fa.out`, `genome.fa.out.gz` or a UCSC "
                 "`rmsk.txt.gz`")
    return OfftargetPlan(prefix, by, *paths)


def from_plan(p: OfftargetPlan, classes: int, annotation) -> "Offtarget":
    return Offtarget(classes, annotation.families, p.by)


def reference_keys(origins, lengths, rows, keys) -> List[np.ndarray]:
    """dgrp_paint_keys_batch in numpy for a list of records (record r: `lengths[r]` bases from the coordinate `origins[r]`, rows[r]
    its rows with SEGMENT_DTYPE fields -- the label is not read --, keys[r] their keys): -> [key track uint32 per record],
    0xFFFFFFFF where no row covers a base, else the smallest key among the rows that do."""
    out = []
    for r in range(len(lengths)):
        n, o = int(lengths[r]), int(origins[r])
        track = np.full(n, NONE, np.uint32)
        for row, k in zip(rows[r], keys[r]):
            a, e = min(max(int(row["start"]) - o, 0), n), min(max(int(row["end"]) - o, 0), n)
            if e > a:
                track[a:e] = np.minimum(track[a:e], np.uint32(int(k)))
        out.append(track)
    return out


def reference_crosstab(pred, keys, C: int, K: int):
    """dgrp_key_crosstab_batch in numpy: `pred` int8 [n], `keys` uint32 [n] -> (hist int64 [C, K], flag).  hist[p, k] counts the
    bases with predicted label p and key k < K - 1, hist[p, K - 1] those with the key 0xFFFFFFFF; any other key, or a label outside
    0 .. C - 1, raises the flag and the base is not counted."""
    p = np.asarray(pred, np.int8).astype(np.int64).ravel()
    k = np.asarray(keys, np.uint32).astype(np.int64).ravel()
    col = np.where(k == NONE, K - 1, k)
    ok = (p >= 0) & (p < C) & ((k == NONE) | (k < K - 1))
    hist = np.zeros((C, K), np.int64)
    np.add.at(hist, (p[ok], col[ok]), 1)
    return hist, int(bool((~ok).any()))


def reference_row_classes(keys, label: int) -> np.ndarray:
    """dgrp_row_key_classes_batch for one row: the keys of its clipped span -> int64 [4]: key == label; another key below 64; a
    family; 0xFFFFFFFF."""
    k = np.asarray(keys, np.uint32).astype(np.int64)
    return np.array([(k == label).sum(), ((k < FIRST_FAMILY) & (k != label)).sum(), ((k >= FIRST_FAMILY) & (k != NONE)).sum(),
                     (k == NONE).sum()], np.int64)


def fold(names: Sequence[str], by: str) -> List[str]:
    """The name a family token is listed under: itself, or with by == "class" its part in front of the first '/'."""
    return list(names) if by == "family" else [nm.split("/", 1)[0] for nm in names]


def _under(hist: np.ndarray, families: Sequence[str], by: str):
    """hist int64 [..., K] -> (names, int64 [..., len(names)]): class<L> for the keys 1..63, the (folded) family names in byte order,
    `none`; columns of one folded name are summed."""
    hist = np.asarray(hist, np.int64)
    F = len(families)
    if hist.shape[-1] != FIRST_FAMILY + F + 1:
        raise ValueError(f"{hist.shape[-1]} key columns for {F} families")
    folded = fold(families, by)
    uniq = sorted(set(folded), key=lambda s: s.encode("utf-8", "surrogateescape"))
    at = {nm: i for i, nm in enumerate(uniq)}
    fam = np.zeros(hist.shape[:-1] + (len(uniq),), np.int64)
    if F:
        np.add.at(fam, (Ellipsis, np.fromiter((at[nm] for nm in folded), np.int64, count=F)), hist[..., FIRST_FAMILY:FIRST_FAMILY + F])
    names = [f"class{k}" for k in range(FIRST_FAMILY)] + uniq + ["none"]
    return names, np.concatenate([hist[..., :FIRST_FAMILY], fam, hist[..., -1:]], axis=-1)


def offtarget_tsv(hist: np.ndarray, families: Sequence[str], by: str = "family") -> str:
    """PREFIX.offtarget.tsv of hist int64 [2, C, K] (scope all / unsupported): the comment, the header, and per scope and predicted
    label the names with bases > 0 -- bases descending, then the name in byte order -- with their share of that (scope, predicted)
    to six decimals."""
    names, x = _under(hist, families, by)
    raw = [nm.encode("utf-8", "surrogateescape") for nm in names]
    lines = [COMMENT, "\t".join(HEADER)]
    for s, scope in enumerate(SCOPES):
        for p in range(x.shape[1]):
            total = int(x[s, p].sum())
            for k in sorted(np.flatnonzero(x[s, p]).tolist(), key=lambda k: (-int(x[s, p, k]), raw[k])):
                lines.append("\t".join([scope, str(p), names[k], str(int(x[s, p, k])), f"{int(x[s, p, k]) / total:.6f}"]))
    return "\n".join(lines) + "\n"


def rows_tsv(rows: np.ndarray) -> str:
    """PREFIX.offtarget.rows.tsv of rows int64 [C, 6]: per predicted class >= 1 its rows, the supported ones, and the unsupported ones
    by the largest of their four counts."""
    rows = np.asarray(rows, np.int64)
    lines = ["\t".join(ROWS_HEADER)]
    for c in range(1, rows.shape[0]):
        lines.append("\t".join([str(c)] + [str(int(v)) for v in rows[c]]))
    return "\n".join(lines) + "\n"


class Offtarget:
    """The counts of one `evaluate --offtarget` run, summed over its work items: `hist` int64 [2, C, K] (scope all / unsupported:
    predicted label by key column, K = 64 + F + 1) and `rows` int64 [C, 6] (ROWS_HEADER behind the class)."""
    key = "offtarget"

    def __init__(self, classes: int, families: Sequence[str], by: str = "family"):
        if by not in BY:
            raise ValueError(f"by: one of {BY}, not {by!r}")
        if len(families) > MAX_FAMILIES:
            raise ValueError(f"{len(families)} families: at most {MAX_FAMILIES}")
        self.C, self.by, self.families = int(classes), by, list(families)
        self.F = len(self.families)
        self.K = FIRST_FAMILY + self.F + 1
        self.hist = np.zeros((2, self.C, self.K), np.int64)
        self.rows = np.zeros((self.C, 6), np.int64)

    def bind(self, annotation, classes: int) -> None:
        if self.C != classes:
            raise ValueError(f"off-target counts of {self.C} classes for a model of {classes}")
        if getattr(annotation, "offtarget_rows", None) is None:
            raise ValueError("off-target counts need the un-modelled rows of a RepeatMasker listing (annotation.evaluation_rows(offtarget=True))")
        self.offtarget_rows, self.offtarget_keys = annotation.offtarget_rows, annotation.offtarget_keys

    def add(self, it, probed) -> None:
        """A work item.  The key track: the item's modelled rows with their labels as keys and its un-modelled rows with 64 + family
        id (dgrp_paint_keys_batch).  Two cross-tabulations against it (dgrp_key_crosstab_batch): the predicted labels, and a second
        track painted from only the predicted rows the item holds as unsupported -- of which the label 0, everything outside those
        rows, is dropped.  Four counts per predicted row (dgrp_row_key_classes_batch)."""
        import torch

        from ._lib import check, lib
        from .evaluation import paint, upload
        from .pipeline import SEGMENT_DTYPE
        L, dev, s, nrec, n, C = lib(), it.dev, it.stream, it.nrec, it.n, it.C
        no_rows, no_keys = np.zeros(0, SEGMENT_DTYPE), np.zeros(0, np.uint32)
        off, ln, org = it.off.ctypes.data, it.ln.ctypes.data, it.org.ctypes.data
        k_rows, k_keys = [], []
        for nm, t in zip(it.names, it.tr):
            o = np.ascontiguousarray(self.offtarget_rows.get(nm, no_rows), SEGMENT_DTYPE)
            ok = np.ascontiguousarray(self.offtarget_keys.get(nm, no_keys), np.uint32)
            if len(o) != len(ok):
                raise ValueError(f"{len(o)} un-modelled rows but {len(ok)} keys")
            k_rows.append(np.concatenate([t, o]))
            k_keys.append(np.concatenate([t["label"].astype(np.uint32), ok]))
        k_off, _k_flat, d_krows = upload(k_rows, dev)
        uns = it.kept & ~it.good
        ur = [p[uns[int(it.p_off[r]):int(it.p_off[r + 1])]] for r, p in enumerate(it.pr)]
        u_off, _u_flat, d_urows = upload(ur, dev)
        wb = int(L.dgrp_eval_workspace_bytes(nrec, max(int(k_off[-1]), int(it.p_off[-1]), int(u_off[-1]))))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        d_rk = torch.from_numpy(np.concatenate(k_keys).view(np.int32)).to(dev) if int(k_off[-1]) else None   # (the sign of the type is not read)
        d_keys = torch.empty(n, dtype=torch.int32, device=dev)                    # (32-bit keys; the sign of the type is not read)
        check(L.dgrp_paint_keys_batch(d_keys.data_ptr(), nrec, off, ln, org, ptr(d_krows), k_off.ctypes.data, ptr(d_rk), work.data_ptr(),
                                      wb, s), "dgrp_paint_keys_batch")
        d_uns = paint(it.ln, it.org, it.off, u_off, d_urows, work, dev)
        d_hist = torch.empty((2, C, self.K), dtype=torch.int64, device=dev)
        d_bad = torch.empty(2, dtype=torch.int32, device=dev)
        for k, d_lab in enumerate((it.d_pred, d_uns)):
            check(L.dgrp_key_crosstab_batch(d_lab.data_ptr(), d_keys.data_ptr(), n, C, self.K, d_hist[k].data_ptr(), d_bad[k:].data_ptr(), s),
                  "dgrp_key_crosstab_batch")
        d_cls = torch.zeros((max(int(it.p_off[-1]), 1), 4), dtype=torch.int64, device=dev)
        check(L.dgrp_row_key_classes_batch(d_keys.data_ptr(), nrec, off, ln, org, ptr(it.d_prows), it.p_off.ctypes.data, d_cls.data_ptr(),
                                           work.data_ptr(), wb, s), "dgrp_row_key_classes_batch")
        hist, bad, cls = d_hist.cpu().numpy(), d_bad.cpu().numpy(), d_cls.cpu().numpy()[:int(it.p_off[-1])]
        if bad.any():
            raise ValueError(f"a predicted label outside 0..{C - 1} or a key outside the {self.F} families of the listing reached the "
                             "off-target counts")
        hist[1, 0] = 0
        self.hist += hist
        if it.p_flat.size:
            self.count_rows(it.p_flat["label"].astype(np.int64), it.kept, it.good, cls)

    def count_rows(self, labels: np.ndarray, kept: np.ndarray, good: np.ndarray, cls: np.ndarray) -> None:
        """The predicted rows of a work item: `kept` has a base inside its record, `good` is supported (evaluation.count's masks),
        cls int64 [rows, 4] the four counts.  An unsupported row goes to the largest of its counts, ties to the first."""
        lab = np.asarray(labels, np.int64)
        np.add.at(self.rows[:, 0], lab[kept], 1)
        np.add.at(self.rows[:, 1], lab[good], 1)
        uns = kept & ~good
        if uns.any():
            np.add.at(self.rows, (lab[uns], 2 + np.argmax(np.asarray(cls, np.int64)[uns], axis=1)), 1)

    def summary(self) -> Dict[str, object]:
        """The `offtarget` key of the JSON report: per class its unsupported rows' bases split three ways -- under a modelled class,
        under an un-modelled family, under nothing -- as shares (None without such bases), and its three largest families."""
        names, x = _under(self.hist[1], self.families, self.by)
        fam = x[:, FIRST_FAMILY:-1]
        out = []
        for c in range(self.C):
            total = int(x[c].sum())
            share = lambda v: None if total == 0 else int(v) / total
            top = sorted(np.flatnonzero(fam[c]).tolist(), key=lambda k: (-int(fam[c, k]), names[FIRST_FAMILY + k].encode("utf-8", "surrogateescape")))[:3]
            out.append(dict(unsupported_bases=total, modelled=share(x[c, :FIRST_FAMILY].sum()), offtarget=share(fam[c].sum()),
                            unannotated=share(x[c, -1]), top=[[names[FIRST_FAMILY + k], int(fam[c, k])] for k in top]))
        return dict(by=self.by, families=self.F, classes=out)

    def write(self, p: OfftargetPlan, log) -> None:
        """The two files, staged: a failure leaves neither of them, nor a temporary file."""
        write_texts(log, p.prefix, "--offtarget", (p.table_path, p.rows_path),
                    [offtarget_tsv(self.hist, self.families, self.by), rows_tsv(self.rows)])
