"""Cost of predict --track_bigwig, one JSON line.

    track_bigwig_throughput.py [Mbp] [PARENT]   the command line with --track_gzip --track_index and with --track_bigwig, two runs each,
                                                every run a process of its own, interleaved; with PARENT (a built checkout of the parent
                                                commit) the --track_gzip --track_index run is the parent's

On one synthetic record of Mbp (default 250) with the trained model, D = 2, B = 1, classes 1-4."""
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
parent = sys.argv[2] if len(sys.argv) > 2 else here
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
w = synthetic.trained_weights()
trained = os.path.join(d, "trained.h5")
dgmodel.save_keras_hdf5(trained, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
fa = os.path.join(d, "chr.fa")
with open(fa, "wb") as fh:
    fh.write(b">chr1\n" + b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
runs = [("index", parent, ["--track_dir", os.path.join(d, "x"), "--track_gzip", "--track_index"]),
        ("bigwig", here, ["--track_dir", os.path.join(d, "b"), "--track_bigwig"])]
times = {}
for it in range(2):
    for label, cwd, extra in runs:
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m", "deepgrp_amd", "predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv")] + extra,
                       cwd=cwd, check=True, timeout=300)
        times.setdefault(label, []).append(round(time.perf_counter() - t0, 3))
size = lambda sub: {f: os.path.getsize(os.path.join(d, sub, f)) for f in sorted(os.listdir(os.path.join(d, sub)))}
tsv = lambda label: open(os.path.join(d, f"{label}.tsv"), "rb").read()
print(json.dumps(dict(what="e2e", mbp=mbp, parent_is_this_tree=parent == here, track_gzip_index_s=times["index"], track_bigwig_s=times["bigwig"],
                      bigwig_over_index=round(min(times["bigwig"]) / min(times["index"]), 4),
                      spread_of_index=round(max(times["index"]) / min(times["index"]) - 1, 4), bw_bytes=size("b"), gz_bytes=size("x"),
                      tsv_identical=tsv("index") == tsv("bigwig"))), flush=True)
