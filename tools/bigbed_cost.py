"""Device time of one bigBed write beside one BGZF BED write of the same rows, one JSON line.

    bigbed_cost.py [rows] [records] [runs] [gzip_level]

Synthetic input without a model: `rows` segment rows (default 10^6) of 30 bases every 48 bases, shared out evenly over `records`
records (default 24), labels 1..4, against random float32 probabilities [bases, 5] made on the device.  ContigPipeline.bigbed_write
(scores, item blocks, zoom records, both deflated, read back) and ContigPipeline.bed_write (--bed_gzip: scores, text, BGZF members,
read back) run alternately, `runs` each (default 5) after one warm-up of both; a host clock around each call, which ends with its
results on the host and a device synchronise.  Median, fastest and slowest in milliseconds, and the bytes each form produced."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepgrp_amd import bed
from deepgrp_amd.pipeline import SEGMENT_DTYPE, ContigPipeline

nrows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
nrec = int(sys.argv[2]) if len(sys.argv) > 2 else 24
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
level = int(sys.argv[4]) if len(sys.argv) > 4 else 1

per = (nrows + nrec - 1) // nrec
counts = np.minimum(per, nrows - per * np.arange(nrec)).clip(0)
lengths = (counts * 48 + 64).astype(np.int64)
row0 = np.r_[0, np.cumsum((lengths[:-1] + 63) // 64 * 64)].astype(np.int64)
rows = np.zeros(nrows, SEGMENT_DTYPE)
row_off = np.r_[0, np.cumsum(counts)].astype(np.int64)
for r in range(nrec):
    a, b = int(row_off[r]), int(row_off[r + 1])
    rows["start"][a:b] = 5 + 48 * np.arange(b - a)
    rows["contig"][a:b] = r
rows["end"] = rows["start"] + 30
rows["label"] = 1 + np.arange(nrows) % 4
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
torch.manual_seed(7)
probs = torch.rand((int(row0[-1] + lengths[-1]), 5), dtype=torch.float32, device=dev)
probs /= probs.sum(1, keepdim=True)
names = [b"chr%d" % (r + 1) for r in range(nrec)]
pipe = ContigPipeline.__new__(ContigPipeline)          # (the two methods use no model)
forms = {"bigbed_write": bed.BedPlan("", 0, {}, level, False, True), "bed_write (--bed_gzip)": bed.BedPlan("", 0, {}, level, False, False)}
ms = {k: [] for k in forms}
size = {}
for it in range(runs + 1):
    for label, plan in forms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = pipe.bed_write(probs, row0, lengths, np.zeros(nrec, np.int64), rows, row_off, names, True, plan)
        torch.cuda.synchronize()
        if it:
            ms[label].append(round((time.perf_counter() - t0) * 1e3, 2))
        size[label] = len(w.blocks) + len(w.zoom) if plan.bigbed else len(w.members)
print(json.dumps({"what": "one write, ms", "rows": nrows, "records": nrec, "runs": runs, "gzip_level": level,
                  **{k: {"median": statistics.median(v), "fastest": min(v), "slowest": max(v), "bytes": size[k]} for k, v in ms.items()}}))
