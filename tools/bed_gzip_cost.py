"""Cost of predict --bed_dir as plain text, with --bed_gzip and with --bed_gzip --bed_index, one JSON line per figure.

    bed_gzip_cost.py [Mbp] [runs] [gzip_level]

On one synthetic record of Mbp (default 250, the benchmark chromosome) with the trained model, the command line under -vv (FASTA
file -> TSV file, the staged record path) in the three forms, interleaved, `runs` each (default 5): the milliseconds of the BED
stage (the `row scores` debug line: scores, text, deflate, index pieces and the write to the file, between device syncs) and of the
whole command; then the three file sizes and the size bgzip at level 6 would give the same text (zlib level 6 over the same
0xff00-byte blocks, gz.bgzf_compress)."""
import json
import logging
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import gz
from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
level = sys.argv[3] if len(sys.argv) > 3 else "1"
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def out(**kw):
    print(json.dumps(kw), flush=True)


class Stage(logging.Handler):
    """Keeps the milliseconds of the `row scores` debug lines."""

    def __init__(self):
        super().__init__(logging.DEBUG)
        self.ms = []

    def emit(self, record):
        m = re.search(r": row scores ([0-9.]+) ms", record.getMessage())
        if m:
            self.ms.append(float(m.group(1)))


w = synthetic.trained_weights()
trained = os.path.join(d, "trained.h5")
dgmodel.save_keras_hdf5(trained, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
fa = os.path.join(d, "chr.fa")
with open(fa, "wb") as fh:
    fh.write(b">chr1\n" + b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
torch.cuda.set_device(0)
log = logging.getLogger("deepgrp_amd.__main__")
log.propagate = False                                   # the debug lines of 15 runs stay out of the output
stage = Stage()
log.addHandler(stage)
forms = (("plain", []), ("gzip", ["--bed_gzip", "--gzip_level", level]), ("gzip_index", ["--bed_gzip", "--bed_index", "--gzip_level", level]))
stage_ms = {k: [] for k, _ in forms}
total_s = {k: [] for k, _ in forms}
main(["predict", trained, fa, "--output", os.path.join(d, "warm.tsv")])              # the first run pays for the kernels' load
for it in range(runs):
    for label, extra in forms:
        del stage.ms[:]
        t0 = time.perf_counter()
        main(["-vv", "predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv"), "--bed_dir", os.path.join(d, label)] + extra)
        total_s[label].append(round(time.perf_counter() - t0, 3))
        stage_ms[label].append(round(sum(stage.ms), 2))


def spread(v):
    return {"median": statistics.median(v), "fastest": min(v), "slowest": max(v)}


text = open(os.path.join(d, "plain", "chr.fa.bed"), "rb").read()
packed = open(os.path.join(d, "gzip", "chr.fa.bed.gz"), "rb").read()
indexed = open(os.path.join(d, "gzip_index", "chr.fa.bed.gz"), "rb").read()
out(what="bed stage, ms", mbp=mbp, runs=runs, gzip_level=int(level), rows=text.count(b"\n"), **{k: spread(v) for k, v in stage_ms.items()})
out(what="whole command under -vv, s", **{k: spread(v) for k, v in total_s.items()})
out(what="bytes", bed=len(text), bed_gz=len(packed), bed_gz_with_index=len(indexed),
    tbi=os.path.getsize(os.path.join(d, "gzip_index", "chr.fa.bed.gz.tbi")), zlib_level_6_same_blocks=len(gz.bgzf_compress(text, level=6)),
    same_members=packed == indexed,
    tsv_identical=len({open(os.path.join(d, f"{k}.tsv"), "rb").read() for k, _ in forms}) == 1)
