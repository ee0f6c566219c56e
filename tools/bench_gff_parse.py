#!/usr/bin/env python3
"""dgrp_gff_parse beside dgrp_rows_parse (table) on files of the same --rows rows (default 10^6): the rows of a seeded
table `contig begin end number name family`, and the same rows as GFF3 feature lines as `predict --bed_gff3` words them
(`Name=class<number>`, twelve figures' worth of further attributes).  Both texts are uploaded once; each entry is called once
untimed, then --runs times (default 7), the two alternating, with device events around the call (its kernels, its two
synchronisations; the outputs and the workspace are allocated in front of the first event).  The rows of the two entries are compared
before anything is timed.  Prints one JSON object -- per entry the times, their median, the text bytes and the bytes per second over
the median; --out writes it to a file as well.  `--kernels-only N`: N calls of the GFF3 entry and nothing else, the command for a
`rocprofv3 --kernel-trace --stats` run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("HSATII", "ALR/Alpha", "SINE/Alu", "LINE/L1")


def generated(rows: int, seed: int = 11, contigs: int = 24):
    """(the table, the GFF3 of the same rows) as bytes."""
    rng = np.random.default_rng(seed)
    per = np.full(contigs, rows // contigs)
    per[: rows % contigs] += 1
    table, gff, j = [], ["##gff-version 3\n"], 0
    for c, k in enumerate(per):
        name = f"chr{c + 1}"
        begin = np.cumsum(rng.integers(20, 4000, k))
        end = begin + rng.integers(10, 3000, k)
        number = rng.integers(1, len(FAMILIES) + 1, k)
        for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist()):
            j += 1
            table.append(f"{name}\t{b}\t{e}\t{n}\trep{n}\t{FAMILIES[n - 1]}\n")
            gff.append(f"{name}\tdeepgrp\trepeat_region\t{b + 1}\t{e}\t0.9312\t.\t.\tID=r{j};Name=class{n};label={n};score=931;min=0.4100;agree=0.9562\n")
    return "".join(table).encode(), "".join(gff).encode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gff_parse.py measures on the GPU: none is visible")
    from deepgrp_amd import gffin
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import require_gpu, stream_ptr
    L, dev = lib(), require_gpu()
    table, gff = generated(args.rows)
    up = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev)
    d_table, d_gff = up(table), up(gff)
    names = gffin.default_names(len(FAMILIES) + 1)
    blob, off, number, count = gffin.names_table(names)
    d_blob, d_off, d_number, d_key = (torch.from_numpy(a).to(dev) for a in (blob, off, number, np.frombuffer(b"Name", np.uint8).copy()))
    cap = args.rows + 1
    i64 = lambda: torch.empty(cap, dtype=torch.int64, device=dev)
    out = {k: (torch.empty(cap, dtype=torch.int32, device=dev) if k == "name_len" else i64())
           for k in ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")}
    ptrs = [out[k].data_ptr() for k in ("begin", "end", "number", "name_pos", "name_len")]
    wb = max(int(L.dgrp_rows_parse_workspace_bytes(len(table))), int(L.dgrp_gff_parse_workspace_bytes(len(gff))))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)

    def rows_call():
        c = (C.c_int64 * 6)()
        rc = L.dgrp_rows_parse(d_table.data_ptr(), len(table), 0, *ptrs, None, None, out["line"].data_ptr(), out["run_first"].data_ptr(), cap, c,
                               work.data_ptr(), wb, stream_ptr())
        assert rc == 0 and list(c)[3:] == [0, 0, 0], (rc, list(c))
        return list(c)

    def gff_call():
        c = (C.c_int64 * 7)()
        rc = L.dgrp_gff_parse(d_gff.data_ptr(), len(gff), d_blob.data_ptr(), d_off.data_ptr(), d_number.data_ptr(), count, d_key.data_ptr(), 4, *ptrs,
                              out["line"].data_ptr(), out["run_first"].data_ptr(), cap, c, work.data_ptr(), wb, stream_ptr())
        assert rc == 0 and list(c)[3:6] == [0, 0, 0], (rc, list(c))
        return list(c)

    if args.kernels_only:
        for _ in range(args.kernels_only):
            counts = gff_call()
        torch.cuda.synchronize()
        print(json.dumps({"kernels_only": args.kernels_only, "gff_bytes": len(gff), "lines": counts[0], "rows": counts[1]}))
        return
    # the two entries give the same rows (and this is the untimed call of each)
    c_rows = rows_call()
    want = {k: out[k][:args.rows].clone() for k in ("begin", "end", "number")}
    c_gff = gff_call()
    torch.cuda.synchronize()
    assert c_rows[1] == c_gff[1] == args.rows and c_rows[2] == c_gff[2] and c_gff[6] == len(gff)
    assert all(torch.equal(out[k][:args.rows], want[k]) for k in want)
    res = {"rows": args.rows, "runs": args.runs, "device": torch.cuda.get_device_name(0), "table_bytes": len(table), "gff_bytes": len(gff),
           "rows_parse_ms": [], "gff_parse_ms": []}
    for _ in range(args.runs):
        for key, fn in (("rows_parse_ms", rows_call), ("gff_parse_ms", gff_call)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            res[key].append(a.elapsed_time(b))
    for key, size in (("rows_parse", len(table)), ("gff_parse", len(gff))):
        med = statistics.median(res[key + "_ms"])
        res[key + "_median_ms"] = med
        res[key + "_GBps"] = size / med / 1e6
        res[key + "_ns_per_row"] = med * 1e6 / args.rows
    res["gff_over_rows_time"] = res["gff_parse_median_ms"] / res["rows_parse_median_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
