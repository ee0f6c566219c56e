"""Cost of predict --mask_dir: the command line on one synthetic 250 Mbp record (file -> TSV file), two runs without and two runs
with a soft-masked copy of the file.  Under `rocprofv3 --kernel-trace --stats` the mask kernels' device time shows next to the rest."""
import os, sys, time, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepgrp_amd import synthetic, model as dgmodel
from deepgrp_amd.__main__ import main

mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250
d = tempfile.mkdtemp()
w = synthetic.trained_weights()
mpath = os.path.join(d, "model.hdf5")
dgmodel.save_keras_hdf5(mpath, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
fa = os.path.join(d, "chr.fa")
raw = synthetic.synthetic_chromosome(int(mbp * 1e6), contig=0)
with open(fa, "wb") as fh:
    fh.write(b">chr1\n")
    fh.write(b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
times = {}
for label, extra in (("plain", []), ("mask", ["--mask_dir", os.path.join(d, "masked")])):
    for it in range(2):
        t0 = time.perf_counter()
        main(["predict", mpath, fa, "--output", os.path.join(d, "out.tsv")] + extra)
        dt = time.perf_counter() - t0
        times.setdefault(label, []).append(dt)
        print(f"{label} run {it}: {mbp:g} Mbp FASTA -> TSV{' + masked FASTA' if extra else ''} in {dt:.3f} s = {mbp / dt:.0f} Mbp/s",
              flush=True)
print(f"best with / without --mask_dir: {min(times['mask']):.3f} / {min(times['plain']):.3f} s = "
      f"{min(times['mask']) / min(times['plain']):.2f}x", flush=True)
