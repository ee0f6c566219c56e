#!/usr/bin/env python3
"""What `train` spends between its input paths and the first enqueued step, for the two forms of input: a sequence file
(device ingest, truth and sampler sets built on the GPU) and the `.npz` of preprocess_sequence (loaded, labelled and indexed on the
host, then uploaded).  One synthetic record of --bases (default 50 Mbp) with the annotation of its planted repeats is both sides of
the data, as FASTA and as `.fa.gz.npz`; the time preprocess_sequence's steps take to write that .npz is reported beside, not inside.

Each path is what the command runs up to the first step: both sides prepared, both samplers built, the first batch of starts on the
device, then one device synchronise.  One untimed pass of each path first; then --repeats passes, the two paths alternating.  The
device path's parts (ingest, truth entry, class-set entry per class) are timed once more on their own, each ending in a synchronise.
Prints one JSON object; --out writes it to a file as well."""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write_inputs(tmp, bases):
    from deepgrp_amd import synthetic
    from deepgrp_amd._scripts import preprocess_sequence as pp
    t = time.perf_counter()
    seq = synthetic.synthetic_chromosome(bases, contig=0)
    fasta, bed = os.path.join(tmp, "chr1.fa"), os.path.join(tmp, "rm.bed")
    with open(fasta, "wb") as fh:
        fh.write(b">chr1 synthetic\n")
        view = memoryview(seq)
        for o in range(0, bases, 60 << 14):                               # lines of 60 bases, written in pieces
            piece = np.frombuffer(view[o:o + (60 << 14)], np.uint8)
            full = piece.size // 60 * 60
            lines = np.concatenate([piece[:full].reshape(-1, 60), np.full((full // 60, 1), 10, np.uint8)], axis=1).tobytes()
            fh.write(lines + (piece[full:].tobytes() + b"\n" if piece.size > full else b""))
    with open(bed, "w") as fh:
        fh.writelines(synthetic.synthetic_annotation(bases, contig=0, name="chr1"))
    made = time.perf_counter() - t
    # preprocess_sequence's own steps on the gzip of that file: parse, one-hot, np.savez_compressed
    gz_path = os.path.join(tmp, "chr1.fa.gz")
    with open(fasta, "rb") as src, gzip.open(gz_path, "wb", compresslevel=1) as dst:
        while True:
            block = src.read(1 << 24)
            if not block:
                break
            dst.write(block)
    t = time.perf_counter()
    pp.main([gz_path, "--force"])
    return fasta, gz_path + ".npz", bed, made, time.perf_counter() - t


def device_path(fasta, bed, opt):
    import torch
    from deepgrp_amd import training
    rng = np.random.default_rng(1)
    sides = [training.DeviceData.from_sequence_file(fasta, bed, opt.repeats_to_search, vecsize=opt.vecsize) for _ in range(2)]
    gens = [training.DeviceSampler(opt, side, rng).batches() for side in sides]
    starts = next(gens[0])
    torch.cuda.synchronize()
    return starts


def host_path(npz, bed, opt):
    import torch
    from deepgrp_amd import preprocessing, training
    rng = np.random.default_rng(1)
    name = os.path.basename(npz).split(".")[0]
    data = []
    for _ in range(2):
        fwd = preprocessing.load_onehot_npz(npz)
        y = preprocessing.preprocess_y(bed, name, fwd.shape[1], opt.repeats_to_search)
        data.append(preprocessing.Data(*preprocessing.drop_start_end_n(fwd, y)))
    records = [training.DeviceRecord.from_data(d) for d in data]
    gens = [training.fetch_batch(opt, d, rng)() for d in data]
    starts = torch.from_numpy(next(gens[0])).cuda()
    torch.cuda.synchronize()
    return starts, records


def device_parts(fasta, bed, opt):
    """Ingest, truth entry and class-set entry of ONE side, each on its own between synchronises (seconds)."""
    import ctypes as C

    import torch
    from deepgrp_amd import _lib, training
    from deepgrp_amd.fasta import read_multi_fasta_device
    from deepgrp_amd.pipeline import record_indices, stream_ptr
    L = _lib.lib()
    out = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    kept = [record_indices(rec) for _header, rec in read_multi_fasta_device(fasta)]
    torch.cuda.synchronize()
    out["ingest_s"] = time.perf_counter() - t
    del kept
    t = time.perf_counter()
    rows = training.read_truth_rows(bed, ["chr1"], opt.repeats_to_search)
    out["annotation_parse_s"] = time.perf_counter() - t
    out["annotation_rows"] = int(len(rows["chr1"]))
    side = training.DeviceData.from_sequence_file(fasta, bed, opt.repeats_to_search, vecsize=opt.vecsize)
    nrec, n = len(side.lengths), side.n
    flat = rows["chr1"]
    row_off = np.array([0, len(flat)], np.int64)
    d_rows = torch.from_numpy(flat.view(np.uint8)).cuda()
    d_truth = torch.empty_like(side.d_truth)
    wb = L.dgrp_truth_workspace_bytes(nrec, len(flat))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(4):
        torch.cuda.synchronize()
        t = time.perf_counter()
        _lib.check(L.dgrp_truth_multihot_batch(d_truth.data_ptr(), side.classes, n, nrec, side.base.ctypes.data, side.lengths.ctypes.data,
                                               side.startpos.ctypes.data, d_rows.data_ptr(), row_off.ctypes.data, work.data_ptr(), wb,
                                               stream_ptr()), "dgrp_truth_multihot_batch")
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    assert torch.equal(d_truth, side.d_truth)
    out["truth_s"] = min(times[1:])
    wb = L.dgrp_class_starts_workspace_bytes(nrec, n)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    count = C.c_int64(0)
    d_out = torch.empty(n, dtype=torch.int64, device="cuda")
    per_class = []
    for c in range(1, side.classes):
        times = []
        for _ in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            _lib.check(L.dgrp_class_window_starts(side.d_truth[c].data_ptr(), n, nrec, side.base.ctypes.data, side.lengths.ctypes.data,
                                                  int(opt.vecsize), d_out.data_ptr(), n, C.byref(count), work.data_ptr(), wb, stream_ptr()),
                       "dgrp_class_window_starts")
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        per_class.append({"class": c, "starts": int(count.value), "count_and_write_s": min(times[1:])})
    out["class_sets"] = per_class
    out["bases"] = n
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--vecsize", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from deepgrp_amd.model import Options
    if not torch.cuda.is_available():
        sys.exit("train_prep_time.py measures on the GPU: none is visible")
    opt = Options(vecsize=args.vecsize)
    with tempfile.TemporaryDirectory() as tmp:
        fasta, npz, bed, made_s, preprocess_s = _write_inputs(tmp, args.bases)
        res = {"bases": args.bases, "vecsize": args.vecsize, "batch_size": int(opt.batch_size), "device": torch.cuda.get_device_name(0),
               "fasta_bytes": os.path.getsize(fasta), "npz_bytes": os.path.getsize(npz), "inputs_generated_s": made_s,
               "preprocess_sequence_s": preprocess_s, "device_path_s": [], "npz_path_s": []}
        # the two paths give the same first batch
        a = device_path(fasta, bed, opt)
        b, _records = host_path(npz, bed, opt)
        res["first_batch_equal"] = bool(torch.equal(a, b))
        del a, b, _records
        for _ in range(args.repeats):
            for key, run in (("device_path_s", lambda: device_path(fasta, bed, opt)), ("npz_path_s", lambda: host_path(npz, bed, opt))):
                torch.cuda.synchronize()
                t = time.perf_counter()
                kept = run()
                res[key].append(time.perf_counter() - t)
                del kept
        for key in ("device_path_s", "npz_path_s"):
            res[key + "_median"] = statistics.median(res[key])
        res["npz_over_device"] = res["npz_path_s_median"] / res["device_path_s_median"]
        res["parts_of_one_side"] = device_parts(fasta, bed, opt)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
