"""One dgrp_rmout_text_batch call next to one dgrp_gff_text_batch call on the same rows, one JSON line per figure.

    rmout_cost.py [rows] [runs]

`rows` synthetic rows (default 10^6) of three records with consistent random scores are uploaded once; after a warm-up of both
entries each is called `runs` times (default 20), alternating, through ContigPipeline's methods (allocation of text and workspace,
the call with its one synchronisation, no read-back of the text), with a host clock around the call and a device synchronise behind
it.  The listing is timed without join and with --rmout_join 100.  The first call's text is checked against rmout.reference_lines on
the first 2 000 rows."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepgrp_amd import rmout
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE, ContigPipeline

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ONE = 1 << 24
rng = np.random.default_rng(1)
rows = np.zeros(n, SEGMENT_DTYPE)
rows["contig"] = np.sort(rng.integers(0, 3, n))
width = rng.integers(40, 3000, n)
gap = rng.integers(0, 400, n)
for r in range(3):
    sel = rows["contig"] == r
    end = np.cumsum(width[sel] + gap[sel])
    rows["start"][sel], rows["end"][sel] = end - width[sel], end
rows["label"] = rng.integers(1, 5, n)
ends = [int(rows["end"][rows["contig"] == r].max()) + 1000 for r in range(3)]
sc = np.zeros(n, ROW_SCORE_DTYPE)
sc["bases"] = width
sc["qmin"] = rng.integers(0, ONE + 1, n)
sc["sum"] = sc["bases"].astype(np.uint64) * rng.integers(sc["qmin"], ONE + 1, n).astype(np.uint64)
sc["agree"] = (sc["bases"] * rng.random(n)).astype(np.int64)
names = [b"chr1", b"chr2", b"scaffold_300"]
pairs = rmout.pairs_of_repeats(range(1, 5))

torch.cuda.set_device(0)
d_rows = torch.from_numpy(rows.view(np.uint8)).cuda()
d_scores = torch.from_numpy(sc.view(np.uint8)).cuda()
forms = {
    "gff3": lambda: ContigPipeline.gff_text_batch(names, True, d_rows, d_scores, 0, None, 0)[0],
    "rmout": lambda: ContigPipeline.rmout_text_batch(names, True, d_rows, d_scores, 0, ends, pairs, -1, 0)[0],
    "rmout_join100": lambda: ContigPipeline.rmout_text_batch(names, True, d_rows, d_scores, 0, ends, pairs, 100, 0)[0],
}
size = {}
for k, f in forms.items():                                  # warm-up: the kernels' load, the allocator's blocks
    for _ in range(2):
        size[k] = int(f().numel())
torch.cuda.synchronize()
head = 2000
want = rmout.reference_lines(names, True, rows[:head], sc[:head], 0, ends, pairs, 100, 0)[0]
got = forms["rmout_join100"]()[:len(want)].cpu().numpy().tobytes()
ms = {k: [] for k in forms}
for _ in range(runs):
    for k, f in forms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text = f()
        torch.cuda.synchronize()
        ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
        del text
print(json.dumps({"what": "one text call, ms", "rows": n, "runs": runs,
                  **{k: {"median": statistics.median(v), "fastest": min(v), "slowest": max(v)} for k, v in ms.items()}}), flush=True)
print(json.dumps({"what": "text bytes", **size, "first_rows_are_the_statement": got == want}), flush=True)
