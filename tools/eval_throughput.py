"""Cost of `evaluate` against `predict`: one synthetic record (250 Mbp by default) and its planted annotation written to a temporary
directory, two runs of each command line on the same file (file -> TSV), then the evaluate report of the trained synthetic model.
With --curves also two runs of `evaluate --curves` (the merged path, the probability histograms, the rows' scores and the two
curve files) and the summaries of its JSON.  Under `rocprofv3 --kernel-trace --stats` the evaluation kernels' device time shows
next to the rest.

    python tools/eval_throughput.py [MBP] [--curves]"""
import json, os, sys, time, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepgrp_amd import synthetic, model as dgmodel
from deepgrp_amd.__main__ import main

argv = [a for a in sys.argv[1:] if a != "--curves"]
with_curves = "--curves" in sys.argv[1:]
mbp = float(argv[0]) if argv else 250
tmp = tempfile.TemporaryDirectory()                  # (about 250 MB of FASTA, annotation and reports: removed at exit)
d = tmp.name
w = synthetic.trained_weights()
mpath = os.path.join(d, "model.hdf5")
dgmodel.save_keras_hdf5(mpath, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
n = int(mbp * 1e6)
fa, ann = os.path.join(d, "chr.fa"), os.path.join(d, "chr.bed")
raw = synthetic.synthetic_chromosome(n, contig=0)
with open(fa, "wb") as fh:
    fh.write(b">chr1\n")
    fh.write(b"\n".join(raw[i:i + 60] for i in range(0, len(raw), 60)) + b"\n")
del raw
lines = synthetic.synthetic_annotation(n, contig=0, name="chr1")
with open(ann, "w") as fh:
    fh.writelines(lines)
print(f"{mbp:g} Mbp record, {len(lines)} planted repeats", flush=True)
times = {}
commands = [("predict", ["predict", mpath, fa, "--output", os.path.join(d, "out.tsv")]),
            ("evaluate", ["evaluate", mpath, ann, fa, "--output", os.path.join(d, "report.tsv"),
                          "--json", os.path.join(d, "report.json")])]
if with_curves:
    commands.append(("evaluate --curves", ["evaluate", mpath, ann, fa, "--output", os.path.join(d, "report_curves.tsv"),
                                           "--json", os.path.join(d, "report_curves.json"), "--curves", os.path.join(d, "curves")]))
for label, argv in commands:
    for it in range(2):
        t0 = time.perf_counter()
        main(argv)
        dt = time.perf_counter() - t0
        times.setdefault(label, []).append(dt)
        print(f"{label} run {it}: {dt:.3f} s = {mbp / dt:.0f} Mbp/s", flush=True)
print(f"best evaluate / predict: {min(times['evaluate']):.3f} / {min(times['predict']):.3f} s = "
      f"{min(times['evaluate']) / min(times['predict']):.3f}x", flush=True)
if with_curves:
    print(f"best evaluate --curves / evaluate: {min(times['evaluate --curves']):.3f} / {min(times['evaluate']):.3f} s = "
          f"{min(times['evaluate --curves']) / min(times['evaluate']):.3f}x", flush=True)
    same = open(os.path.join(d, "report.tsv"), "rb").read() == open(os.path.join(d, "report_curves.tsv"), "rb").read()
    print("report with --curves", "identical" if same else "DIFFERENT", flush=True)
    print("curves", json.dumps(json.load(open(os.path.join(d, "report_curves.json")))["curves"]), flush=True)
    for f in ("curves.bases.tsv", "curves.rows.tsv"):
        print(f, os.path.getsize(os.path.join(d, f)), "bytes", flush=True)
print(open(os.path.join(d, "report.tsv")).read(), end="")
rep = json.load(open(os.path.join(d, "report.json")))
print("TPR", rep["metrics"]["TPR"], "\nPPV", rep["metrics"]["PPV"], "\nMCC", rep["metrics"]["MCC"], flush=True)
tmp.cleanup()
