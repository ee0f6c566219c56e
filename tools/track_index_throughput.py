"""Cost of predict --track_gzip --track_index, one JSON line per figure.

    track_index_throughput.py chains [Mbp]     the text chain and the index chain on one record, classes 1..4, bin 1, digits 2
    track_index_throughput.py e2e [Mbp] [PARENT]   the command line with --track_gzip and with --track_gzip --track_index, two runs
                                                   each, every run a process of its own; with PARENT (a built checkout of the parent
                                                   commit) its --track_gzip run as well, interleaved

`chains` is what to run under `rocprofv3 --kernel-trace --stats -- python tools/track_index_throughput.py chains`: the text chain is
tb_bin_*, tb_count, scan_sums, tb_bounds and tb_write; the index chain is the same front half and ix_tile<0|1|2>, ix_carry, ix_ends.
It also times both calls with events.  On one synthetic record of Mbp (default 250) with the trained model."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main
from deepgrp_amd.pipeline import ContigPipeline, upload_sequence

mode = sys.argv[1] if len(sys.argv) > 1 else "chains"
mbp = float(sys.argv[2]) if len(sys.argv) > 2 else 250
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
CLASSES = (1, 2, 3, 4)


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1), 3), res


w = synthetic.trained_weights()
trained = os.path.join(d, "trained.h5")
dgmodel.save_keras_hdf5(trained, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
torch.cuda.set_device(0)

if mode == "chains":
    pipe = ContigPipeline(dgmodel.load_model(trained))
    st, d_idx = upload_sequence(raw)
    merged = pipe.merged(d_idx)
    del d_idx
    args = (merged, [0], [len(merged)], [st], [b"chr1"], CLASSES, 2, 1)
    for it in range(2):
        ms, (text, off) = timed(lambda: pipe.track_text_batch_device(*args))
        out(what="text chain", run=it, ms=ms, bytes=[int(x) for x in off], note="events around the call: a first pass for the size, a second that writes")
        del text
        ms, (chunks, coff, linear, wpref) = timed(lambda: pipe.track_index_batch_device(*args))
        out(what="index chain", run=it, ms=ms, chunks=[int(x) for x in coff], windows=int(wpref[-1]),
            note="events around the call, the read-back of chunks and windows included")
else:
    fa = os.path.join(d, "chr.fa")
    with open(fa, "wb") as fh:
        fh.write(b">chr1\n" + b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
    del raw
    import subprocess
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = sys.argv[3] if len(sys.argv) > 3 else None
    runs = [("gzip", here, ["--track_dir", os.path.join(d, "z"), "--track_gzip"]),
            ("index", here, ["--track_dir", os.path.join(d, "x"), "--track_gzip", "--track_index"])]
    if parent:
        runs.insert(0, ("parent", parent, ["--track_dir", os.path.join(d, "p"), "--track_gzip"]))
    times = {}
    for it in range(2):
        for label, cwd, extra in runs:
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "deepgrp_amd", "predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv")] + extra,
                           cwd=cwd, check=True, timeout=300)
            times.setdefault(label, []).append(round(time.perf_counter() - t0, 3))
    size = lambda sub: {f: os.path.getsize(os.path.join(d, sub, f)) for f in sorted(os.listdir(os.path.join(d, sub)))}
    same = lambda a, b: all(open(os.path.join(d, a, f), "rb").read() == open(os.path.join(d, b, f), "rb").read() for f in os.listdir(os.path.join(d, a)))
    base = times.get("parent", times["gzip"])
    out(what="e2e", mbp=mbp, parent_track_gzip_s=times.get("parent"), track_gzip_s=times["gzip"], track_index_s=times["index"],
        index_over_parent=round(min(times["index"]) / min(base), 4), spread_of_parent=round(max(base) / min(base) - 1, 4), bytes=size("x"),
        gz_identical=same("z", "x") and (parent is None or same("p", "x")))
