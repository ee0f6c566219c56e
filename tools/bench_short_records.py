"""Forward + merge time (ContigPipeline.merged, HIP events) of short records -- 0.1, 1 and 50 Mbp -- with the benchmark's model: min and
median of 7 timed calls per size after 3 warm-up calls.  `python tools/bench_short_records.py LABEL`: LABEL starts every line (two trees
run alternately write into one file)."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepgrp_amd import synthetic
from deepgrp_amd.pipeline import ContigPipeline, DeviceModel, upload_sequence
label = sys.argv[1] if len(sys.argv) > 1 else ""
w = synthetic.trained_weights()
m = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
pipe = ContigPipeline(m, 50, 256)
for mbp in (0.1, 1, 50):
    _st, d = upload_sequence(synthetic.synthetic_chromosome(int(mbp * 1e6)))
    for _ in range(3):
        pipe.merged(d)
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); pipe.merged(d); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(f"{label:8s} {mbp:5g} Mbp forward+merge: min {min(ts):8.3f} ms  median {float(np.median(ts)):8.3f} ms", flush=True)
