"""Time of predict --summary_dir's pass beside --seq_dir's on the same input, one JSON line per figure.

    summary_cost.py [Mbp] [runs] [bin]

On one synthetic record of Mbp (default 250, the benchmark chromosome) with the trained model, the command line under -v (FASTA
file -> TSV file), `runs` times (default 5) each of: `--seq_dir --summary_dir` (both second passes behind one prediction) and
`--summary_dir --summary_bin` (default bin 100000).  The milliseconds are those of the passes' own -v lines: the second walk over
the file (its upload included), the kernels, the read-back and the write of the files."""
import json
import logging
import os
import re
import shutil
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepgrp_amd import model as dgmodel
from deepgrp_amd import synthetic
from deepgrp_amd.__main__ import main

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nbin = sys.argv[3] if len(sys.argv) > 3 else "100000"
d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def out(**kw):
    print(json.dumps(kw), flush=True)


class Passes(logging.Handler):
    """Keeps the milliseconds of the two passes' -v lines."""

    def __init__(self):
        super().__init__(logging.INFO)
        self.seq, self.summary = [], []

    def emit(self, record):
        text = record.getMessage()
        m = re.search(r" in ([0-9.]+) ms$", text)
        if m and "bytes of FASTA" in text:
            self.seq.append(float(m.group(1)))
        elif m and "repeat content" in text:
            self.summary.append(float(m.group(1)))


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
log.propagate = False                                   # the lines of the runs stay out of the output
passes = Passes()
log.addHandler(passes)
main(["predict", trained, fa, "--output", os.path.join(d, "warm.tsv"), "--seq_dir", os.path.join(d, "warm"), "--summary_dir",
      os.path.join(d, "warm"), "--summary_bin", nbin])    # the first run pays for the kernels' load
binned = []
for it in range(runs):
    main(["-v", "predict", trained, fa, "--output", os.path.join(d, "a.tsv"), "--seq_dir", os.path.join(d, "a"), "--summary_dir",
          os.path.join(d, "a")])
    n = len(passes.summary)
    main(["-v", "predict", trained, fa, "--output", os.path.join(d, "b.tsv"), "--summary_dir", os.path.join(d, "b"), "--summary_bin", nbin])
    binned += passes.summary[n:]
    del passes.summary[n:]


def spread(v):
    return {"median": statistics.median(v), "fastest": min(v), "slowest": max(v), "runs": len(v)}


summary = open(os.path.join(d, "b", "chr.fa.summary.tsv"), "rb").read()
out(what="second passes under -v, ms", mbp=mbp, file_bytes=os.path.getsize(fa), rows=int(summary.split(b"\n")[-2].split(b"\t")[2]),
    seq_dir=spread(passes.seq), summary_dir=spread(passes.summary), summary_dir_with_bin=spread(binned), bin=int(nbin))
out(what="bytes", repeats_fa=os.path.getsize(os.path.join(d, "a", "chr.fa.repeats.fa")), summary_tsv=len(summary),
    density_tsv=os.path.getsize(os.path.join(d, "b", "chr.fa.density.tsv")),
    same_summary=summary == open(os.path.join(d, "a", "chr.fa.summary.tsv"), "rb").read())
out(what="the file's totals", lines=[ln.decode() for ln in summary.split(b"\n")[-7:-1]])

# the entry alone on the resident file and the TSV's rows: device events around `reps` calls (memsets, table copy and the five kernels)
import numpy as np

from deepgrp_amd._lib import check, lib
from deepgrp_amd.pipeline import SEGMENT_DTYPE

L = lib()
dev = torch.device("cuda", 0)
data = np.fromfile(fa, np.uint8)
rows = np.array([(int(f[2]), int(f[3]), int(f[4]), 0) for f in (ln.split(b"\t") for ln in open(os.path.join(d, "b.tsv"), "rb").read().split(b"\n")[:-1])],
                SEGMENT_DTYPE)
d_raw, d_rows = torch.from_numpy(data).to(dev), torch.from_numpy(rows.view(np.uint8)).to(dev)
head = len(b">chr1\n")
h_off, h_len, row_off = np.array([head], np.int64), np.array([data.size - head], np.int64), np.array([0, len(rows)], np.int64)
wb = int(L.dgrp_repeat_summary_workspace_bytes(1, int(h_len[0]), len(rows)))
work = torch.empty(wb, dtype=torch.uint8, device=dev)
for label, b in (("no bins", 0), ("bin %s" % nbin, int(nbin)), ("bin 1000", 1000)):
    bin_off = np.array([0, (int(h_len[0]) + b - 1) // b if b else 0], np.int64)
    d_counts = torch.empty(5 * 10, dtype=torch.int64, device=dev)
    d_bins = torch.empty(max(int(bin_off[1]), 1) * 5, dtype=torch.int64, device=dev)
    d_bad = torch.empty(1, dtype=torch.int64, device=dev)

    def call():
        check(L.dgrp_repeat_summary_batch(d_raw.data_ptr(), 1, h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(), row_off.ctypes.data,
                                          5, b, bin_off.ctypes.data, d_counts.data_ptr(), d_bins.data_ptr(), d_bad.data_ptr(),
                                          work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream))

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1) / 10, 4))
    out(what="dgrp_repeat_summary_batch, ms per call (device events around 10 calls)", form=label, body_bytes=int(h_len[0]), rows=len(rows),
        gb_per_s_of_body_bytes=round(int(h_len[0]) / (statistics.median(ms) * 1e-3) / 1e9, 1), bad=int(d_bad.cpu()[0]),
        positions=int(d_counts.cpu().sum()), **spread(ms))
shutil.rmtree(d, ignore_errors=True)
