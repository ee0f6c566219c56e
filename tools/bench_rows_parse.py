#!/usr/bin/env python3
"""A table `contig begin end number name family` as annotation or as predicted rows, the two routes to {contig: rows}, on
a seeded table of --rows rows (default 10^6; the six columns parse_rm writes, 24 contigs in runs, ascending begins):

  host     evaluation.read_annotation(path, repeats) -- what `evaluate` runs, and what `compare` ran without the device parser;
  device   compare.read_table(path, repeats): the file uploaded, dgrp_rows_parse, the row arrays copied back and grouped.

Each route runs once untimed, then --runs times (default 3), the two alternating; the device route's parts -- upload, the
dgrp_rows_parse call (its kernels and two synchronisations), copies and grouping on the host -- are timed once more on their own,
each ending in a device synchronise.  The routes' rows are compared before anything is timed.  The same for a prediction TSV of
the same rows (compare.tsv_flat_host against format 1).  `--kernels-only N`: N parse calls on the uploaded text and nothing else,
the command for a `rocprofv3 --kernel-trace --stats` run.  Prints one JSON object; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = [1, 2, 3, 4]
FAMILIES = ("HSATII", "ALR/Alpha", "SINE/Alu", "LINE/L1", "SINE/MIR", "LINE/L2")


def generated(rows: int, seed: int = 11, contigs: int = 24):
    """(the table, the TSV of the rows 1..4) as bytes."""
    rng = np.random.default_rng(seed)
    per = np.full(contigs, rows // contigs)
    per[: rows % contigs] += 1
    table, tsv = [], []
    for c, k in enumerate(per):
        name = f"chr{c + 1}"
        begin = np.cumsum(rng.integers(20, 4000, k))
        end = begin + rng.integers(10, 3000, k)
        number = rng.integers(1, len(FAMILIES) + 1, k)
        table += [f"{name}\t{b}\t{e}\t{n}\trep{n}\t{FAMILIES[n - 1]}\n" for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist())]
        tsv += [f"genome.fa\t{name} synthetic\t{b}\t{e}\t{n}\n" for b, e, n in zip(begin.tolist(), end.tolist(), number.tolist()) if n <= 4]
    return "".join(table).encode(), "".join(tsv).encode()


def device_parts(path, tsv: bool):
    """Upload, the parse call, the host's share: seconds, each between synchronises."""
    import torch
    from deepgrp_amd import compare
    from deepgrp_amd.fasta import _upload_file
    from deepgrp_amd.pipeline import require_gpu
    out = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    size = os.path.getsize(path)
    d_text = _upload_file(path, size, require_gpu())
    torch.cuda.synchronize()
    out["upload_s"] = time.perf_counter() - t
    calls = []
    for _ in range(6):
        torch.cuda.synchronize()
        t = time.perf_counter()
        counts, _arrays, rc = compare.rows_parse_device(d_text, size, tsv)
        torch.cuda.synchronize()
        calls.append(time.perf_counter() - t)
        assert rc == 0 and counts[3] == 0 and counts[4] == 0
        del _arrays
    out["parse_call_s"] = min(calls[1:])
    out["parse_call_first_s"] = calls[0]
    out["parse_calls_s"] = calls[1:]
    out["text_bytes"], out["lines"], out["rows"], out["runs"] = size, counts[0], counts[1], counts[2]
    out["parse_call_GBps"] = size / out["parse_call_s"] / 1e9          # (text bytes over the call: allocation of the outputs included)
    t = time.perf_counter()
    flat, _bad = compare.flat_of_device_text(d_text, size, tsv)
    compare._grouped(path, flat, np.ones(flat.begin.size, bool))
    torch.cuda.synchronize()
    out["parse_copy_back_and_group_s"] = time.perf_counter() - t
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rows_parse.py measures on the GPU: none is visible")
    from deepgrp_amd import compare
    from deepgrp_amd.evaluation import read_annotation
    t = time.perf_counter()
    table_bytes, tsv_bytes = generated(args.rows)
    made = time.perf_counter() - t
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        table, tsv = os.path.join(tmp, "table.bed"), os.path.join(tmp, "pred.tsv")
        for path, data in ((table, table_bytes), (tsv, tsv_bytes)):
            with open(path, "wb") as fh:
                fh.write(data)
        if args.kernels_only:
            from deepgrp_amd.fasta import _upload_file
            from deepgrp_amd.pipeline import require_gpu
            d_text = _upload_file(table, len(table_bytes), require_gpu())
            for _ in range(args.kernels_only):
                counts, _arrays, rc = compare.rows_parse_device(d_text, len(table_bytes), False)
                assert rc == 0 and counts[3] == 0
            torch.cuda.synchronize()
            print(json.dumps({"kernels_only": args.kernels_only, "text_bytes": len(table_bytes), "lines": counts[0], "rows": counts[1]}))
            return
        res = {"rows_asked": args.rows, "table_bytes": len(table_bytes), "tsv_bytes": len(tsv_bytes), "generated_s": made,
               "device": torch.cuda.get_device_name(0), "runs": args.runs}
        # the routes agree, and every shape is warm
        want = read_annotation(table, REPEATS)
        got = compare.read_table(table, REPEATS)
        assert got.route == "device" and list(got) == list(want) and all(got[k].tobytes() == want[k].tobytes() for k in want)
        host_tsv, dev_tsv = compare.read_predicted(tsv, "tsv", 5, device=False), compare.read_predicted(tsv, "tsv", 5)
        assert dev_tsv.route == "device" and list(dev_tsv) == list(host_tsv) and all(dev_tsv[k].tobytes() == host_tsv[k].tobytes() for k in host_tsv)
        res["rows_kept"] = int(sum(len(v) for v in want.values()))
        res["contigs"] = len(want)
        routes = (("table_host_s", lambda: read_annotation(table, REPEATS)), ("table_device_s", lambda: compare.read_table(table, REPEATS)),
                  ("tsv_host_s", lambda: compare.read_predicted(tsv, "tsv", 5, device=False)),
                  ("tsv_device_s", lambda: compare.read_predicted(tsv, "tsv", 5)))
        res.update({k: [] for k, _f in routes})
        for _ in range(args.runs):
            for key, fn in routes:
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                res[key].append(time.perf_counter() - t)
        for k, _f in routes:
            res[k + "_median"] = statistics.median(res[k])
        res["table_host_over_device"] = res["table_host_s_median"] / res["table_device_s_median"]
        res["tsv_host_over_device"] = res["tsv_host_s_median"] / res["tsv_device_s_median"]
        res["parts_table"] = device_parts(table, False)
        res["parts_tsv"] = device_parts(tsv, True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
