"""Cost of predict --bed_dir --bed_gff3 --bed_gzip --bed_index against --bed_gzip --bed_index, one JSON line per figure.

    gff_cost.py [Mbp] [runs] [gzip_level]

On one synthetic record of Mbp (default 250, the benchmark chromosome) with the trained model, the command line under -vv (FASTA
file -> TSV file, the staged record path) in the two forms, interleaved as tools/bed_gzip_cost.py does it, `runs` each (default
5): the milliseconds of the BED stage (the `row scores` debug line: scores, text, deflate, index pieces and the write to the file,
between device syncs) and of the whole command; then the file sizes, and whether the `.tbi` is gff.reference_index of the file."""
import json
import logging
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import gff
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
log.propagate = False                                   # the debug lines of the runs stay out of the output
stage = Stage()
log.addHandler(stage)
forms = (("bed", ["--bed_gzip", "--bed_index", "--gzip_level", level]),
         ("gff3", ["--bed_gff3", "--bed_gzip", "--bed_index", "--gzip_level", level]))
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


def inflate(data):
    import zlib
    res, off = [], 0
    while off < len(data):
        z = zlib.decompressobj(31)
        res.append(z.decompress(data[off:]))
        off = len(data) - len(z.unused_data)
    return b"".join(res)


bed_gz = open(os.path.join(d, "bed", "chr.fa.bed.gz"), "rb").read()
gff_gz = open(os.path.join(d, "gff3", "chr.fa.gff3.gz"), "rb").read()
tbi = open(os.path.join(d, "gff3", "chr.fa.gff3.gz.tbi"), "rb").read()
text = inflate(gff_gz)
out(what="bed stage, ms", mbp=mbp, runs=runs, gzip_level=int(level), rows=text.count(b"\n") - 1, **{k: spread(v) for k, v in stage_ms.items()})
out(what="whole command under -vv, s", **{k: spread(v) for k, v in total_s.items()})
out(what="bytes", bed_gz=len(bed_gz), bed_text=len(inflate(bed_gz)), gff3_gz=len(gff_gz), gff3_text=len(text), gff3_tbi=len(tbi),
    bed_tbi=os.path.getsize(os.path.join(d, "bed", "chr.fa.bed.gz.tbi")),
    tbi_is_the_reference_index=inflate(tbi) == gff.reference_index(gff_gz),
    tsv_identical=len({open(os.path.join(d, f"{k}.tsv"), "rb").read() for k, _ in forms}) == 1)
shutil.rmtree(d, ignore_errors=True)
