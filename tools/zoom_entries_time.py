"""Time of the two zoom entries alone (the ladder of csrc/bbi_zoom.h under both), one JSON line.

    zoom_entries_time.py [ROOT]     ROOT: a built checkout whose deepgrp_amd is measured (default: this tree)

ContigPipeline.bed_zoom_batch on the rows of tools/bigbed_cost.py (10^6 rows of 30 bases every 48 bases over 24 records) and
ContigPipeline.track_zoom_batch_device on 8 records of 4 Mbp (classes 1-4, bin 1, D = 2, runs of 37 equal values): 9 runs each after
one warm-up, a host clock around each call, which ends with its offsets and totals on the host and a device synchronise.  Median,
fastest and slowest in milliseconds, the records written and a digest of the track's records.  To compare two checkouts, run the
tool for each alternately, every run a process of its own."""
import hashlib
import json
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch

from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE, ContigPipeline

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
nrows, nrec = 1_000_000, 24
per = (nrows + nrec - 1) // nrec
counts = np.minimum(per, nrows - per * np.arange(nrec)).clip(0)
ends = (counts * 48 + 64).astype(np.int64)
rows = np.zeros(nrows, SEGMENT_DTYPE)
row_off = np.r_[0, np.cumsum(counts)]
for r in range(nrec):
    a, b = int(row_off[r]), int(row_off[r + 1])
    rows["start"][a:b] = 5 + 48 * np.arange(b - a)
    rows["contig"][a:b] = r
rows["end"] = rows["start"] + 30
rows["label"] = 1 + np.arange(nrows) % 4
scores = np.zeros(nrows, ROW_SCORE_DTYPE)
scores["bases"], scores["sum"], scores["agree"], scores["qmin"] = 30, 30 << 23, 15, 1 << 22
up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
d_rows, d_scores = up(rows), up(scores)
n = np.full(8, 4_000_000, np.int64)
row0 = np.r_[0, np.cumsum(n[:-1])].astype(np.int64)
torch.manual_seed(3)
probs = (torch.randint(0, 5, (int(n.sum()) // 37 + 1, 5), device=dev).float() / 4).repeat_interleave(37, 0)[:int(n.sum())].contiguous()


def timed(call):
    ms = []
    for it in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        torch.cuda.synchronize()
        if it:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return got, {"median": statistics.median(ms), "fastest": min(ms), "slowest": max(ms)}


bed, bed_ms = timed(lambda: ContigPipeline.bed_zoom_batch(True, d_rows, d_scores, 0, ends, 0))
track, track_ms = timed(lambda: ContigPipeline.track_zoom_batch_device(None, probs, row0, n, np.zeros(8, np.int64), (1, 2, 3, 4), 2, 1, 0))
print(json.dumps({"what": "one zoom call, ms", "this_tree": len(sys.argv) < 2, "bed_zoom": bed_ms, "bed_records": int(bed[1][-1]),
                  "track_zoom": track_ms, "track_records": int(track[1][-1]),
                  "track_sha256_16": hashlib.sha256(track[0].cpu().numpy().tobytes()).hexdigest()[:16]}), flush=True)
