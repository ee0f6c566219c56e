"""Cost of predict --track_dir, one JSON line per figure.

    track_throughput.py [Mbp] [all|kernel]

all (default): on one synthetic record of Mbp (default 250) with the trained model, defaults (digits 2, bin 1, classes 1..4):
  * forward + merge and the track entry of every class, timed with events in-process (three runs each);
  * the command line (FASTA file -> TSV file) without and with --track_dir, two runs each;
  * lines and bytes per class at digits 2, bins 1 and 50, trained weights on the whole record, random weights on its first tenth
    (their tracks change value nearly every base: tens of GB of text at base resolution);
  * a draft-assembly-like file of 2000 records of 10 kbp (tools/cli_many_contigs.py's file) without and with --track_dir.
kernel: one forward + merge and one track call per class, nothing else (for rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main
from deepgrp_amd.pipeline import ContigPipeline, upload_sequence

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
mode = sys.argv[2] if len(sys.argv) > 2 else "all"
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def out(**kw):
    print(json.dumps(kw), flush=True)


def save(path, w):
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path


def fasta(path, recs):
    with open(path, "wb") as fh:
        for h, s in recs:
            fh.write(b">" + h + b"\n" + b"\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + b"\n")
    return path


def timed(fn, reps):
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


trained = save(os.path.join(d, "trained.h5"), synthetic.trained_weights())
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
torch.cuda.set_device(0)
pipe = ContigPipeline(dgmodel.load_model(trained))
st, d_idx = upload_sequence(raw)
name = b"chr1"
if mode == "kernel":
    merged = pipe.merged(d_idx)
    for c in (1, 2, 3, 4):
        pipe.track_text(merged, st, name, c)
    torch.cuda.synchronize()
    out(what="kernel run done", mbp=mbp)
    sys.exit(0)

merged, t_fwd = timed(lambda: pipe.merged(d_idx), 3)
texts, t_trk = timed(lambda: [pipe.track_text(merged, st, name, c) for c in (1, 2, 3, 4)], 3)
out(what="in-process", mbp=mbp, forward_merge_ms=t_fwd, tracks_4_classes_ms=t_trk,
    track_share_of_forward=round(min(t_trk) / min(t_fwd), 4),
    note="tracks: 4 one-class calls of the track chain incl. the device->host copy of the text and the bytes object")
text_bytes = sum(len(t) for t in texts)
del merged, texts

fa = fasta(os.path.join(d, "chr.fa"), [(b"chr1", raw)])
times = {}
for label, extra in (("plain", []), ("tracks", ["--track_dir", os.path.join(d, "tracks")])):
    for it in range(2):
        t0 = time.perf_counter()
        main(["predict", trained, fa, "--output", os.path.join(d, f"{label}.tsv")] + extra)
        times.setdefault(label, []).append(round(time.perf_counter() - t0, 3))
out(what="e2e", mbp=mbp, plain_s=times["plain"], tracks_s=times["tracks"],
    overhead=round(min(times["tracks"]) / min(times["plain"]) - 1, 4), track_bytes=text_bytes,
    tsv_identical=open(os.path.join(d, "plain.tsv"), "rb").read() == open(os.path.join(d, "tracks.tsv"), "rb").read())

random = dgmodel.load_model(save(os.path.join(d, "random.h5"), synthetic.synthetic_weights(128, 5, False, seed=7)))
for label, m, n in (("trained", pipe.model, d_idx.numel()), ("random", random, d_idx.numel() // 10)):
    p = ContigPipeline(m)
    merged = p.merged(d_idx[:n])
    for b in (1, 50):
        for c in (1, 2, 3, 4):
            t = p.track_text(merged, st, name, c, 2, b)
            out(what="size", weights=label, mbp=round(n / 1e6, 3), bin=b, cls=c, lines=t.count(b"\n"), bytes=len(t))
            del t
    del merged
del raw, d_idx

ncontig, n = 2000, 10_000
asm = synthetic.synthetic_chromosome(ncontig * n + 40000, contig=0)[20000:-20000]
fa2 = fasta(os.path.join(d, "asm.fa"), [(b"ctg%d" % (k + 1), asm[k * n:(k + 1) * n]) for k in range(ncontig)])
times = {}
for label, extra in (("plain", []), ("tracks", ["--track_dir", os.path.join(d, "tracks2")])):
    for it in range(2):
        t0 = time.perf_counter()
        main(["predict", trained, fa2, "--output", os.path.join(d, f"asm_{label}.tsv")] + extra)
        times.setdefault(label, []).append(round(time.perf_counter() - t0, 3))
out(what="many records", records=ncontig, kbp=n / 1e3, plain_s=times["plain"], tracks_s=times["tracks"],
    ratio=round(min(times["tracks"]) / min(times["plain"]), 3),
    tsv_identical=open(os.path.join(d, "asm_plain.tsv"), "rb").read() == open(os.path.join(d, "asm_tracks.tsv"), "rb").read())
