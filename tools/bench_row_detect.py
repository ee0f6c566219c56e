"""The two entries of `evaluate --curves --curve_elements` alone (dgrp_paint_row_keys_batch, dgrp_row_detect_batch)
next to dgrp_row_hits_batch, their yardstick: one record of MBP million bases with the rows of synthetic_annotation as its
annotation and the same rows moved by a few bases, with random scores, as its predicted rows.  HIP events around each entry (its
row check and its one synchronisation included), a warm-up, then the median and fastest..slowest of RUNS runs; bytes read per pass
of the detection (2 per clipped base) and by the hits (1 per clipped base).

    python tools/bench_row_detect.py [MBP] [--runs R] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepgrp_amd import synthetic
from deepgrp_amd._lib import check, lib
from deepgrp_amd.curves import need_of
from deepgrp_amd.evaluation import clipped_lengths
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE, require_gpu, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("mbp", nargs="?", type=float, default=250.0)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--json", default=None)
args = ap.parse_args()
assert args.runs >= 5

dev = require_gpu()
L = lib()
n, flank = int(args.mbp * 1e6), 1000
lines = synthetic.synthetic_annotation(n, contig=0, name="chr1", flank=flank)
true = np.zeros(len(lines), SEGMENT_DTYPE)
for i, l in enumerate(lines):
    f = l.split("\t")
    true[i] = (int(f[1]), int(f[2]), int(f[3]), 0)
pred = true.copy()
pred["start"] += 7                                                      # the same runs a little off: ascending, not overlapping
pred["end"] = np.maximum(pred["end"] + 3, pred["start"])
rng = np.random.default_rng(1)
origin, length = flank, n - 2 * flank
p_clen, t_clen = clipped_lengths(pred, origin, length), clipped_lengths(true, origin, length)
scores = np.zeros(len(pred), ROW_SCORE_DTYPE)
scores["bases"] = p_clen
scores["sum"] = (rng.random(len(pred)) * (p_clen.astype(np.float64) * 2.0 ** 24)).astype(np.uint64)
need = need_of(0.5, t_clen)

up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
d_true, d_pred, d_scores, d_need = up(true), up(pred), up(scores), up(need)
off, ln, org = (np.array([v], np.int64) for v in (0, length, origin))
ro = np.array([0, len(true)], np.int64)
wb = int(L.dgrp_row_detect_workspace_bytes(1, len(true)))
work = torch.empty(wb, dtype=torch.uint8, device=dev)
d_keys = torch.zeros(length, dtype=torch.int16, device=dev)
d_labels = torch.zeros(length, dtype=torch.int8, device=dev)
d_det = torch.empty(len(true), dtype=torch.int32, device=dev)
d_hits = torch.empty(len(true), dtype=torch.int64, device=dev)
tabs = (1, off.ctypes.data, ln.ctypes.data, org.ctypes.data)


def paint_keys():
    check(L.dgrp_paint_row_keys_batch(d_keys.data_ptr(), *tabs, d_pred.data_ptr(), ro.ctypes.data, d_scores.data_ptr(), work.data_ptr(), wb,
                                      stream_ptr()), "dgrp_paint_row_keys_batch")


def detect():
    check(L.dgrp_row_detect_batch(d_keys.data_ptr(), *tabs, d_true.data_ptr(), ro.ctypes.data, d_need.data_ptr(), d_det.data_ptr(),
                                  work.data_ptr(), wb, stream_ptr()), "dgrp_row_detect_batch")


def hits():
    check(L.dgrp_row_hits_batch(d_labels.data_ptr(), *tabs, d_true.data_ptr(), ro.ctypes.data, d_hits.data_ptr(), work.data_ptr(), wb,
                                stream_ptr()), "dgrp_row_hits_batch")


def timed(f):
    f()                                                                 # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), fastest=min(ms), slowest=max(ms))


check(L.dgrp_paint_rows_batch(d_labels.data_ptr(), *tabs, d_pred.data_ptr(), ro.ctypes.data, work.data_ptr(), wb, stream_ptr()),
      "dgrp_paint_rows_batch")
out = dict(mbp=args.mbp, runs=args.runs, rows=len(true), clipped_bases=int(t_clen.sum()), predicted_bases=int(p_clen.sum()),
           detect_bytes_per_pass=2 * int(t_clen.sum()), detect_passes=10, hits_bytes=int(t_clen.sum()))
out["paint_keys_ms"] = timed(paint_keys)
out["detect_ms"] = timed(detect)
out["hits_ms"] = timed(hits)
det, h = d_det.cpu().numpy(), d_hits.cpu().numpy()
assert ((det >= 0) == (h >= need))[need > 0].all()                      # at m = 0 the two entries say the same
out["found_at_0"] = int((det >= 0).sum())
out["distinct_scores"] = int(len(np.unique(det)))
print(json.dumps(out), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
