#!/usr/bin/env python3
"""The entries of `evaluate --boundaries` beside the entry they stand next to, HIP events around each call, the median
of --reps (default 7) after one untimed call:

  record    the record and the generated rows of tools/bench_offtarget.py -- one record of --bases evaluated bases (default
            49 980 000), a truth track painted from 42 000 modelled rows, predicted rows that do not overlap: dgrp_row_bounds_batch
            at W = --max (default 200) beside dgrp_row_hits_batch on the same rows (the predicted rows against the truth), and
            dgrp_bound_hist_batch on the same rows;
  command   `evaluate` on a synthetic genome of --genome bases (default 4 000 000) with the synthetic model, with and without
            --boundaries, interleaved, --runs times each (default 5), wall clock of the child process.

Prints one JSON object; --out writes it to a file as well.  --skip record,command leaves parts out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, reps):
    """call() once untimed, then `reps` times between two events on the current stream -> {median_ms, min_ms, max_ms}"""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def record_part(bases, W, reps):
    import numpy as np
    import torch
    from deepgrp_amd import boundaries
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.curves import need_of
    from deepgrp_amd.pipeline import SEGMENT_DTYPE
    L, rng = lib(), np.random.default_rng(3)
    s = torch.cuda.current_stream().cuda_stream

    def rows_of(count, lo, hi, labels):
        r = np.zeros(count, SEGMENT_DTYPE)
        r["start"] = np.sort(rng.integers(0, bases - hi, count))
        r["end"] = r["start"] + rng.integers(lo, hi, count)
        r["label"] = labels(count)
        return r
    modelled = rows_of(42_000, 50, 600, lambda k: rng.integers(1, 5, k))
    rows_of(120_000, 50, 2000, lambda k: np.zeros(k, np.int64))                 # (the generator of bench_offtarget.py draws these in between)
    pred = rows_of(40_000, 50, 600, lambda k: rng.integers(1, 5, k))
    pred = pred[np.r_[True, pred["start"][1:] >= pred["end"][:-1]]]             # predicted rows do not overlap
    ln, org, off = np.array([bases], np.int64), np.zeros(1, np.int64), np.array([0, bases], np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_mrows, d_prows = up(modelled), up(pred)
    mo, po = (np.array([0, len(x)], np.int64) for x in (modelled, pred))
    wb = max(int(L.dgrp_row_bounds_workspace_bytes(1, len(modelled))), int(L.dgrp_bound_hist_workspace_bytes(1)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    d_true = torch.zeros(bases, dtype=torch.int8, device="cuda")
    tab = (1, off.ctypes.data, ln.ctypes.data, org.ctypes.data)
    check(L.dgrp_paint_rows_batch(d_true.data_ptr(), *tab, d_mrows.data_ptr(), mo.ctypes.data, work.data_ptr(), wb, s))
    clen = np.clip(pred["end"], 0, bases) - np.clip(pred["start"], 0, bases)
    d_need = torch.from_numpy(need_of(0.5, clen)).cuda()
    d_hits = torch.empty(len(pred), dtype=torch.int64, device="cuda")
    d_bounds = torch.empty((len(pred), 5), dtype=torch.int64, device="cuda")
    d_frag = torch.empty((5, boundaries.FRAG), dtype=torch.int64, device="cuda")
    d_edge = torch.empty((5, 2, 2 * W + 1), dtype=torch.int64, device="cuda")
    d_tally = torch.empty((5, 2), dtype=torch.int64, device="cuda")
    d_bad = torch.empty(1, dtype=torch.int32, device="cuda")
    res = {"bases": bases, "W": W, "truth_rows": len(modelled), "predicted_rows": len(pred), "clipped_bases": int(clen.sum()),
           "line_positions_bound": int(clen.sum()) + 2 * W * len(pred)}
    res["dgrp_row_hits_batch"] = timed(lambda: check(L.dgrp_row_hits_batch(d_true.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data,
                                                                           d_hits.data_ptr(), work.data_ptr(), wb, s)), reps)
    res["dgrp_row_bounds_batch"] = timed(lambda: check(L.dgrp_row_bounds_batch(d_true.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data, W,
                                                                               d_bounds.data_ptr(), work.data_ptr(), wb, s)), reps)
    res["dgrp_row_bounds_batch_W0"] = timed(lambda: check(L.dgrp_row_bounds_batch(d_true.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data, 0,
                                                                                  d_bounds.data_ptr(), work.data_ptr(), wb, s)), reps)
    check(L.dgrp_row_bounds_batch(d_true.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data, W, d_bounds.data_ptr(), work.data_ptr(), wb, s))
    res["dgrp_bound_hist_batch"] = timed(lambda: check(L.dgrp_bound_hist_batch(*tab, d_prows.data_ptr(), po.ctypes.data, d_bounds.data_ptr(),
                                                                               d_need.data_ptr(), 5, W, d_frag.data_ptr(), d_edge.data_ptr(),
                                                                               d_tally.data_ptr(), d_bad.data_ptr(), work.data_ptr(), wb, s)), reps)
    b = np.ascontiguousarray(d_bounds.cpu().numpy()).view(boundaries.BOUND_DTYPE).reshape(-1)
    assert (b["hits"] == d_hits.cpu().numpy()).all() and int(d_bad.item()) == 0
    frag, tally = d_frag.cpu().numpy(), d_tally.cpu().numpy()
    assert frag.sum() == len(pred)
    res["ratio_bounds_to_hits"] = res["dgrp_row_bounds_batch"]["median_ms"] / res["dgrp_row_hits_batch"]["median_ms"]
    res["found_rows"], res["rows_with_two_runs_or_more"] = int(tally[:, 0].sum()), int(frag[:, 2:].sum())
    return res


def command_part(genome, runs):
    import rm_cases
    from deepgrp_amd import model as dgmodel, synthetic
    res = {"genome_bases": genome, "runs": runs, "plain_s": [], "boundaries_s": []}
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        w = synthetic.trained_weights()
        model = os.path.join(tmp, "synth.hdf5")
        dgmodel.save_keras_hdf5(model, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
        seq = synthetic.synthetic_chromosome(genome, contig=10, flank=1000)
        fa = os.path.join(tmp, "genome.fa")
        with open(fa, "wb") as fh:
            fh.write(b">chr1\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
        lines = []
        for k, row in enumerate(synthetic.synthetic_annotation(genome, contig=10, name="chr1", flank=1000)):
            ctg, b, e, lab = row.split("\t")[:4]
            fam = rm_cases.FAMILIES[int(lab) - 1] if int(lab) < 4 else rm_cases.OTHER_FAMILIES[k % len(rm_cases.OTHER_FAMILIES)]
            lines.append(rm_cases.out_line(ctg, int(b) + 1, int(e), "x", fam))
            lines.append(rm_cases.out_line(ctg, int(b) + 31, int(e) + 300, "x", rm_cases.OTHER_FAMILIES[(k + 3) % len(rm_cases.OTHER_FAMILIES)]))
        listing = os.path.join(tmp, "genome.fa.out")
        with open(listing, "w") as fh:
            fh.write(rm_cases.HEADER + "\n".join(lines) + "\n")
        res["listing_lines"] = len(lines)
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cmd = [sys.executable, "-m", "deepgrp_amd", "evaluate", model, listing, fa, "--repeats", "1,2,3", "--output", os.path.join(tmp, "report.tsv")]
        for k in range(runs + 1):                                          # the first pair is untimed
            for key, flags in (("plain_s", []), ("boundaries_s", ["--boundaries", os.path.join(tmp, "run")])):
                t = time.perf_counter()
                subprocess.run(cmd + flags, env=env, check=True, capture_output=True, timeout=600)
                if k:
                    res[key].append(time.perf_counter() - t)
    for key in ("plain_s", "boundaries_s"):
        res[key + "_median"] = statistics.median(res[key])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=49_980_000)
    ap.add_argument("--max", type=int, default=200)
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", type=str, default="")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_boundaries.py measures on the GPU: none is visible")
    skip = set(filter(None, args.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if "record" not in skip:
        res["record"] = record_part(args.bases, args.max, args.reps)
    if "command" not in skip:
        res["command"] = command_part(args.genome, args.runs)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
