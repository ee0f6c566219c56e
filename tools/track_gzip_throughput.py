"""Cost of predict --track_dir --track_gzip, one JSON line per figure.

    track_gzip_throughput.py [Mbp]

On one synthetic record of Mbp (default 250) with the trained model, defaults (digits 2, bin 1, classes 1..4):
  * the deflate chain at level 0 and level 1 on the first 254 MB of class 1's track text, timed with events (three runs each), and
    the sizes of that piece at both levels;
  * the command line (FASTA file -> TSV file) alone, with --track_dir, and with --track_dir --track_gzip, two runs each, and the
    bytes of the track files either way."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import gz
from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main
from deepgrp_amd.pipeline import ContigPipeline, upload_sequence

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def out(**kw):
    print(json.dumps(kw), flush=True)


w = synthetic.trained_weights()
trained = os.path.join(d, "trained.h5")
dgmodel.save_keras_hdf5(trained, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
torch.cuda.set_device(0)
pipe = ContigPipeline(dgmodel.load_model(trained))
st, d_idx = upload_sequence(raw)
merged = pipe.merged(d_idx)
d_text = pipe.track_text_device(merged, st, b"chr1", 1)[:3894 * gz.BGZF_BLOCK].clone()
del merged, d_idx
for level in (0, 1):
    ms, size = [], 0
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        size = int(gz.bgzf_compress_device(d_text, eof=False, level=level).numel())
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1), 3))
    out(what="deflate chain", level=level, input_bytes=int(d_text.numel()), output_bytes=size, ms=ms,
        gb_per_s=round(d_text.numel() / min(ms) / 1e6, 1), note="events around the call: three kernels, allocations and the size's read-back")
del d_text
torch.cuda.empty_cache()

fa = os.path.join(d, "chr.fa")
with open(fa, "wb") as fh:
    fh.write(b">chr1\n" + b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
times = {}
runs = (("plain", []), ("tracks", ["--track_dir", os.path.join(d, "t")]), ("gzip", ["--track_dir", os.path.join(d, "z"), "--track_gzip"]))
for it in range(2):
    for label, extra in runs:
        t0 = time.perf_counter()
        main(["predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv")] + extra)
        times.setdefault(label, []).append(round(time.perf_counter() - t0, 3))
size = lambda sub: {f: os.path.getsize(os.path.join(d, sub, f)) for f in sorted(os.listdir(os.path.join(d, sub)))}
out(what="e2e", mbp=mbp, plain_s=times["plain"], tracks_s=times["tracks"], track_gzip_s=times["gzip"],
    gzip_over_tracks=round(min(times["gzip"]) / min(times["tracks"]), 4), track_bytes=size("t"), track_gzip_bytes=size("z"),
    tsv_identical=open(os.path.join(d, "plain.tsv"), "rb").read() == open(os.path.join(d, "gzip.tsv"), "rb").read())
