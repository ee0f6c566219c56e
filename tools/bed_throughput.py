"""Cost of predict --bed_dir, one JSON line per figure.

    bed_throughput.py [Mbp] [all|kernel] [runs]

all (default): on one synthetic record of Mbp (default 250) with the trained model:
  * in-process, timed around device syncs (three runs each): the fused record call (dgrp_predict_record), the staged form
    merged -> labels -> segments that --bed_dir uses for a record on its own, and the score call on the staged form's rows;
  * the command line (FASTA file -> TSV file) without and with --bed_dir, interleaved, `runs` each (default 4).
kernel: one staged run and one score call, nothing else (for rocprofv3 --kernel-trace --stats)."""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main
from deepgrp_amd.pipeline import ContigPipeline, upload_sequence

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
mode = sys.argv[2] if len(sys.argv) > 2 else "all"
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 4
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(round((time.perf_counter() - t0) * 1e3, 2))
    return r, ts


w = synthetic.trained_weights()
trained = os.path.join(d, "trained.h5")
dgmodel.save_keras_hdf5(trained, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
torch.cuda.set_device(0)
pipe = ContigPipeline(dgmodel.load_model(trained))
st, d_idx = upload_sequence(raw)
if mode == "kernel":
    merged = pipe.merged(d_idx)
    rows = pipe.segments(pipe.labels(merged), st)
    pipe.row_scores(merged, st, rows)
    torch.cuda.synchronize()
    out(what="kernel run done", mbp=mbp, rows=len(rows))
    sys.exit(0)

_, t_fused = timed(lambda: pipe.run_idx(d_idx, st), 3)
staged = lambda: pipe.segments(pipe.labels(pipe.merged(d_idx)), st)
rows, t_staged = timed(staged, 3)
merged = pipe.merged(d_idx)
scores, t_score = timed(lambda: pipe.row_scores(merged, st, rows), 3)
out(what="in-process", mbp=mbp, rows=len(rows), scored_bases=int(scores["bases"].sum()), fused_record_ms=t_fused, staged_record_ms=t_staged,
    row_scores_ms=t_score, note="row_scores: upload of the rows, check, span, scan, init, score kernel, read-back of 32 bytes per row")
del merged, d_idx

fa = os.path.join(d, "chr.fa")
with open(fa, "wb") as fh:
    fh.write(b">chr1\n" + b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
times = {"plain": [], "bed": []}
for it in range(runs):
    for label, extra in (("plain", []), ("bed", ["--bed_dir", os.path.join(d, "beds")])):
        t0 = time.perf_counter()
        main(["predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv")] + extra)
        times[label].append(round(time.perf_counter() - t0, 3))
out(what="e2e", mbp=mbp, plain_s=times["plain"], bed_s=times["bed"], plain_median=statistics.median(times["plain"]),
    bed_median=statistics.median(times["bed"]), bed_bytes=os.path.getsize(os.path.join(d, "beds", "chr.fa.bed")),
    tsv_identical=open(os.path.join(d, "plain.tsv"), "rb").read() == open(os.path.join(d, "bed.tsv"), "rb").read())
