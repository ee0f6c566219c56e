#!/usr/bin/env python3
"""Time of dgrp_fasta_extract_batch (predict --seq_dir) next to dgrp_fasta_mask_batch, an existing streaming pass over the same
bytes: one record of 256 MiB of synthetic FASTA text (60-column lines) on the device, 10^5 rows of 300 bases spread evenly plus one
row of 3 Mbp.  Each entry is timed as a whole (it synchronises once), best and median of --repeats calls after one warm-up; one JSON
line on standard output, also written to --out when given."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--row_bases", type=int, default=300)
    ap.add_argument("--long_bases", type=int, default=3_000_000)
    ap.add_argument("--flank", type=int, default=0)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    import torch

    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import SEGMENT_DTYPE, require_gpu, stream_ptr
    L, dev = lib(), require_gpu()
    nbytes = args.bytes // 61 * 61
    nseq = nbytes // 61 * 60
    d_raw = torch.randint(0, 4, (nbytes,), dtype=torch.uint8, device=dev)
    d_raw = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[d_raw.long()]
    d_raw[60::61] = 10
    # the long row first, then the short rows evenly over the rest
    rows = np.zeros(args.rows + 1, SEGMENT_DTYPE)
    rows[0] = (1000, 1000 + args.long_bases, 1, 0)
    first = 1000 + args.long_bases + 1000
    step = (nseq - first - args.row_bases) // args.rows
    assert step > args.row_bases
    rows["start"][1:] = first + step * np.arange(args.rows)
    rows["end"][1:] = rows["start"][1:] + args.row_bases
    rows["label"][1:] = 1 + np.arange(args.rows) % 4
    d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
    h_off, h_len = np.zeros(1, np.int64), np.array([nbytes], np.int64)
    row_off, name_off = np.array([0, len(rows)], np.int64), np.array([0, 4], np.int64)
    d_names = torch.tensor(list(b"chr1"), dtype=torch.uint8, device=dev)
    bits = 0b11110
    wb = int(L.dgrp_fasta_extract_workspace_bytes(1, nbytes, len(rows)))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    cap = int((rows["end"] - rows["start"] + 2 * args.flank).sum() * 62 // 60 + 64 * len(rows))
    d_text = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_entries = torch.empty(len(rows) * 24, dtype=torch.uint8, device=dev)
    size, kept = C.c_int64(0), C.c_int64(0)

    def extract():
        check(L.dgrp_fasta_extract_batch(d_raw.data_ptr(), 1, h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(), row_off.ctypes.data,
                                         d_names.data_ptr(), name_off.ctypes.data, args.flank, args.width, bits, d_text.data_ptr(), cap,
                                         C.byref(size), d_entries.data_ptr(), C.byref(kept), work.data_ptr(), wb, stream_ptr()), "extract")

    mwb = int(L.dgrp_fasta_mask_workspace_bytes(1, nbytes, len(rows)))
    mwork = torch.empty(mwb, dtype=torch.uint8, device=dev)
    d_out = torch.empty_like(d_raw)

    def mask():
        check(L.dgrp_fasta_mask_batch(d_raw.data_ptr(), 1, h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(), row_off.ctypes.data, 0,
                                      bits, d_out.data_ptr(), mwork.data_ptr(), mwb, stream_ptr()), "mask")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return dict(best_ms=round(min(ms), 3), median_ms=round(statistics.median(ms), 3))

    res = dict(input_bytes=nbytes, rows=len(rows), flank=args.flank, width=args.width, extract=timed(extract), mask=timed(mask))
    res["text_bytes"], res["kept_rows"] = size.value, kept.value
    res["device"] = torch.cuda.get_device_name(dev)
    res["timing"] = "host clock around each entry call and a device synchronise; the entry itself synchronises once"
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
