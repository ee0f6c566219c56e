#!/usr/bin/env python3
"""A RepeatMasker listing as annotation, the two routes to {contig: rows}, on a generated `.out` text of --lines lines
(default 10^6; tests/rm_cases.generated):

  parent   parse_rm.read_repeatmasker over the file, its six-column table written, evaluation.read_annotation on that table -- what
           a user ran before `evaluate` and `train` took the listing itself;
  device   annotation.read_rows: the file uploaded (or inflated on the device), dgrp_rm_parse, the row arrays copied back and grouped.

Each route runs once untimed, then --runs times (default 3), the two alternating, for the plain file and for its BGZF copy; the
device route's parts -- upload (with inflate for BGZF), the dgrp_rm_parse call (its kernels and two synchronisations), copies and
grouping on the host -- are timed once more on their own, each ending in a device synchronise.  The routes' rows are compared before
anything is timed.  `--kernels-only N`: N parse calls on the uploaded text and nothing else, the command for a
`rocprofv3 --kernel-trace --stats` run.  Prints one JSON object; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parent_route(listing, table):
    from deepgrp_amd._scripts import parse_rm
    from deepgrp_amd.evaluation import read_annotation
    t0 = time.perf_counter()
    parse_rm.main([listing, "-o", table])
    t1 = time.perf_counter()
    rows = read_annotation(table, None)
    return rows, t1 - t0, time.perf_counter() - t1


def device_route(path):
    import torch
    from deepgrp_amd import annotation
    rows = annotation.read_rows(path, fmt="repeatmasker")
    torch.cuda.synchronize()
    assert rows.route == "device"
    return rows


def device_parts(path):
    """Upload (+ inflate), the parse call, the host's share: seconds, each between synchronises."""
    import torch
    from deepgrp_amd import annotation, gz
    from deepgrp_amd.fasta import RESIDENT_BYTES, _upload_file
    from deepgrp_amd.pipeline import require_gpu
    out = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    if gz.is_gzip(path):
        _text, d_text, size = gz.open_inflated(path, RESIDENT_BYTES, require_gpu, _upload_file)
    else:
        size = os.path.getsize(path)
        d_text = _upload_file(path, size, require_gpu())
    torch.cuda.synchronize()
    out["upload_and_inflate_s" if gz.is_gzip(path) else "upload_s"] = time.perf_counter() - t
    calls = []
    for _ in range(4):
        torch.cuda.synchronize()
        t = time.perf_counter()
        counts, _arrays, rc = annotation.parse_device(d_text, size)
        torch.cuda.synchronize()
        calls.append(time.perf_counter() - t)
        assert rc == 0 and counts[3] == 0
        del _arrays
    out["parse_call_s"] = min(calls[1:])
    out["parse_call_first_s"] = calls[0]
    out["text_bytes"], out["lines"], out["rows"], out["runs"] = size, counts[0], counts[1], counts[2]
    out["parse_GBps"] = size / out["parse_call_s"] / 1e9
    t = time.perf_counter()
    listing = annotation.listing_of_device_text(path, d_text, size)
    rows, _lines = listing.grouped(listing.table_mask())
    torch.cuda.synchronize()
    out["parse_copy_back_and_group_s"] = time.perf_counter() - t
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_annotation.py measures on the GPU: none is visible")
    import rm_cases
    from deepgrp_amd import annotation, gz
    t = time.perf_counter()
    data = rm_cases.generated(args.lines, seed=11, contigs=24)
    made = time.perf_counter() - t
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        plain, packed, table = (os.path.join(tmp, x) for x in ("genome.fa.out", "genome.fa.out.gz", "table.bed"))
        with open(plain, "wb") as fh:
            fh.write(data)
        if args.kernels_only:
            from deepgrp_amd.fasta import _upload_file
            from deepgrp_amd.pipeline import require_gpu
            d_text = _upload_file(plain, len(data), require_gpu())
            for _ in range(args.kernels_only):
                counts, _arrays, rc = annotation.parse_device(d_text, len(data))
                assert rc == 0 and counts[3] == 0
            torch.cuda.synchronize()
            print(json.dumps({"kernels_only": args.kernels_only, "text_bytes": len(data), "lines": counts[0], "rows": counts[1]}))
            return
        with open(packed, "wb") as fh:
            fh.write(gz.bgzf_compress(data, level=1))
        res = {"lines_asked": args.lines, "text_bytes": len(data), "bgzf_bytes": os.path.getsize(packed), "generated_s": made,
               "device": torch.cuda.get_device_name(0), "runs": args.runs}
        # the routes agree, and every shape is warm
        want, _a, _b = parent_route(plain, table)
        for path in (plain, packed):
            got = device_route(path)
            assert sorted(got) == sorted(want) and all(got[k].tobytes() == want[k].tobytes() for k in want), path
        res["rows"] = int(sum(len(v) for v in want.values()))
        res["contigs"] = len(want)
        keys = ("parent_parse_rm_s", "parent_read_annotation_s", "parent_s", "device_plain_s", "device_bgzf_s")
        res.update({k: [] for k in keys})
        for _ in range(args.runs):
            _rows, a, b = parent_route(plain, table)
            res["parent_parse_rm_s"].append(a)
            res["parent_read_annotation_s"].append(b)
            res["parent_s"].append(a + b)
            for key, path in (("device_plain_s", plain), ("device_bgzf_s", packed)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                device_route(path)
                res[key].append(time.perf_counter() - t)
        for k in keys:
            res[k + "_median"] = statistics.median(res[k])
        res["parent_over_device_plain"] = res["parent_s_median"] / res["device_plain_s_median"]
        res["parent_over_device_bgzf"] = res["parent_s_median"] / res["device_bgzf_s_median"]
        res["parts_plain"] = device_parts(plain)
        res["parts_bgzf"] = device_parts(packed)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
