#!/usr/bin/env python3
"""The entries of `evaluate --offtarget` beside the entries they stand next to, HIP events around each call, the median
of --reps (default 7) after one untimed call:

  listing   dgrp_rm_parse_all against dgrp_rm_parse_fields, and dgrp_token_ids on the rows of the former, on the generated `.out`
            text of tools/bench_annotation.py (--lines lines, default 10^6; tests/rm_cases.generated);
  record    one record of --bases evaluated bases (default 49 980 000) with generated annotation rows -- modelled rows of four
            labels, un-modelled rows of 60 families -- and a predicted track painted from generated rows: dgrp_paint_keys_batch
            beside dgrp_paint_strata_batch (the modelled rows), dgrp_key_crosstab_batch beside dgrp_confusion_matrix, and
            dgrp_row_key_classes_batch beside dgrp_row_hits_batch;
  command   `evaluate` on a synthetic genome of --genome bases (default 4 000 000) with the synthetic model, with and without
            --offtarget, interleaved, --runs times each (default 5), wall clock of the child process.

Prints one JSON object; --out writes it to a file as well.  --skip listing,record,command leaves parts out."""
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


def listing_part(lines, reps):
    import rm_cases
    import torch
    from deepgrp_amd import annotation
    data = rm_cases.generated(lines, seed=11, contigs=24)
    d_text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    n = len(data)
    res = {"text_bytes": n}
    c_f, _o, rc = annotation.parse_device(d_text, n, fields=True)
    c_a, out, rc_a = annotation.parse_device(d_text, n, all_rows=True)
    assert rc == rc_a == 0 and c_a[3] == 0
    res["lines"], res["rows_fields"], res["rows_all"] = c_a[0], c_f[1], c_a[1]
    res["dgrp_rm_parse_fields"] = timed(lambda: annotation.parse_device(d_text, n, fields=True), reps)
    res["dgrp_rm_parse_all"] = timed(lambda: annotation.parse_device(d_text, n, all_rows=True), reps)
    spans = [out[k] for k in ("fam_pos", "fam_len", "fam2_pos", "fam2_len")]
    ids = annotation.token_ids_device(d_text, n, c_a[1], *spans)
    res["families"] = len(ids[1])
    res["dgrp_token_ids"] = timed(lambda: annotation.token_ids_device(d_text, n, c_a[1], *spans), reps)
    return res


def record_part(bases, reps):
    import numpy as np
    import torch
    from deepgrp_amd._lib import check, lib
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
    other = rows_of(120_000, 50, 2000, lambda k: np.zeros(k, np.int64))
    pred = rows_of(40_000, 50, 600, lambda k: rng.integers(1, 5, k))
    pred = pred[np.r_[True, pred["start"][1:] >= pred["end"][:-1]]]             # predicted rows do not overlap
    F = 60
    K = 64 + F + 1
    key_rows = np.concatenate([modelled, other])
    row_key = np.concatenate([modelled["label"].astype(np.uint32), (64 + rng.integers(0, F, len(other))).astype(np.uint32)])
    ln, org, off = np.array([bases], np.int64), np.zeros(1, np.int64), np.array([0, bases], np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_krows, d_rk, d_mrows, d_prows = up(key_rows), up(row_key), up(modelled), up(pred)
    d_st = torch.from_numpy(rng.integers(0, 40, len(modelled)).astype(np.uint8)).cuda()
    ko, mo, po = (np.array([0, len(x)], np.int64) for x in (key_rows, modelled, pred))
    wb = int(L.dgrp_eval_workspace_bytes(1, len(key_rows)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    d_keys = torch.empty(bases, dtype=torch.int32, device="cuda")
    d_skeys = torch.empty(bases, dtype=torch.int32, device="cuda")
    d_true = torch.zeros(bases, dtype=torch.int8, device="cuda")
    d_pred = torch.zeros(bases, dtype=torch.int8, device="cuda")
    tab = (1, off.ctypes.data, ln.ctypes.data, org.ctypes.data)
    for d_lab, d_rows, ro in ((d_true, d_mrows, mo), (d_pred, d_prows, po)):
        check(L.dgrp_paint_rows_batch(d_lab.data_ptr(), *tab, d_rows.data_ptr(), ro.ctypes.data, work.data_ptr(), wb, s))
    d_hist = torch.empty((5, K), dtype=torch.int64, device="cuda")
    d_cnf = torch.empty((5, 5), dtype=torch.int64, device="cuda")
    d_bad = torch.empty(1, dtype=torch.int32, device="cuda")
    d_cls = torch.empty((len(pred), 4), dtype=torch.int64, device="cuda")
    d_hits = torch.empty(len(pred), dtype=torch.int64, device="cuda")
    res = {"bases": bases, "modelled_rows": len(modelled), "unmodelled_rows": len(other), "predicted_rows": len(pred), "families": F}
    res["dgrp_paint_keys_batch"] = timed(lambda: check(L.dgrp_paint_keys_batch(d_keys.data_ptr(), *tab, d_krows.data_ptr(), ko.ctypes.data,
                                                                               d_rk.data_ptr(), work.data_ptr(), wb, s)), reps)
    res["dgrp_paint_strata_batch"] = timed(lambda: check(L.dgrp_paint_strata_batch(d_skeys.data_ptr(), *tab, d_mrows.data_ptr(), mo.ctypes.data,
                                                                                   d_st.data_ptr(), work.data_ptr(), wb, s)), reps)
    res["dgrp_key_crosstab_batch"] = timed(lambda: check(L.dgrp_key_crosstab_batch(d_pred.data_ptr(), d_keys.data_ptr(), bases, 5, K,
                                                                                   d_hist.data_ptr(), d_bad.data_ptr(), s)), reps)
    res["dgrp_confusion_matrix"] = timed(lambda: check(L.dgrp_confusion_matrix(d_true.data_ptr(), d_pred.data_ptr(), bases, 5, d_cnf.data_ptr(),
                                                                               d_bad.data_ptr(), s)), reps)
    res["dgrp_row_key_classes_batch"] = timed(lambda: check(L.dgrp_row_key_classes_batch(d_keys.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data,
                                                                                         d_cls.data_ptr(), work.data_ptr(), wb, s)), reps)
    res["dgrp_row_hits_batch"] = timed(lambda: check(L.dgrp_row_hits_batch(d_true.data_ptr(), *tab, d_prows.data_ptr(), po.ctypes.data,
                                                                           d_hits.data_ptr(), work.data_ptr(), wb, s)), reps)
    hist, cnf = d_hist.cpu().numpy(), d_cnf.cpu().numpy()
    assert hist.sum() == bases and all((hist[:, lab] == cnf[lab]).all() for lab in range(1, 5)) and (hist[:, 64:].sum(axis=1) == cnf[0]).all()
    assert (d_cls.cpu().numpy()[:, 0] == d_hits.cpu().numpy()).all()
    res["covered_bases"] = int(bases - hist[:, -1].sum())
    return res


def command_part(genome, runs):
    import rm_cases
    from deepgrp_amd import model as dgmodel, synthetic
    res = {"genome_bases": genome, "runs": runs, "plain_s": [], "offtarget_s": []}
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
            for key, flags in (("plain_s", []), ("offtarget_s", ["--offtarget", os.path.join(tmp, "run")])):
                t = time.perf_counter()
                subprocess.run(cmd + flags, env=env, check=True, capture_output=True, timeout=600)
                if k:
                    res[key].append(time.perf_counter() - t)
    for key in ("plain_s", "offtarget_s"):
        res[key + "_median"] = statistics.median(res[key])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--bases", type=int, default=49_980_000)
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", type=str, default="")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_offtarget.py measures on the GPU: none is visible")
    skip = set(filter(None, args.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if "listing" not in skip:
        res["listing"] = listing_part(args.lines, args.reps)
    if "record" not in skip:
        res["record"] = record_part(args.bases, args.reps)
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
