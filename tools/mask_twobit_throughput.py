"""predict --mask_twobit: the write of the masked copy of the benchmark's synthetic chromosome of [Mbp] (default 250),
as `predict` does it -- masking.write_mask from the FASTA file in /dev/shm (60-column lines, as bench.py writes it) to a
file beside it, rows of a synthetic annotation (one row of 1 kb in every 5 kb, labels 1..3, soft mask) -- as a .2bit and as the
plain masked text.  The plain copy is the yardstick: that path is what it was before --mask_twobit existed.  [warm-up] untimed rounds
(default 1), then [rounds] timed rounds (default 5), the two forms alternating in every round; host clock around the call and a
device synchronise; median, fastest and slowest of each.  The 2bit file is first checked against the plain copy through
twobit.pack_record (the numpy packer).  One JSON line per result.
    python tools/mask_twobit_throughput.py [Mbp] [rounds] [warm-up] [both|twobit|plain]
Kernel times come from a run of its own: rocprofv3 --kernel-trace --stats -- python tools/mask_twobit_throughput.py 250 1 0 twobit"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import write_fasta  # noqa: E402
from deepgrp_amd import masking, synthetic, twobit  # noqa: E402
from deepgrp_amd.pipeline import SEGMENT_DTYPE  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def spread(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(float(np.min(xs)), 3), max=round(float(np.max(xs)), 3), n=len(xs))


def write(path, final, rows, form):
    plan = masking.MaskPlan({}, "soft", None, twobit=form == "twobit")
    torch.cuda.synchronize()
    t = time.perf_counter()
    masking.write_mask(path, final, rows, plan)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250.0
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    which = sys.argv[4] if len(sys.argv) > 4 else "both"
    forms = ("plain", "twobit") if which == "both" else (which,)
    n = int(mbp * 1e6)
    torch.cuda.set_device(0)
    raw = synthetic.synthetic_chromosome(n, contig=0)
    rows = np.zeros(n // 5000, SEGMENT_DTYPE)
    rows["start"] = np.arange(rows.size, dtype=np.int64) * 5000 + 2000
    rows["end"] = rows["start"] + 1000
    rows["label"] = 1 + np.arange(rows.size) % 3
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else "/tmp"
    src = os.path.join(shm, f"dgrp_mask2bit_{os.getpid()}.fa")
    out = {"plain": src + ".masked.fa", "twobit": src + ".masked.2bit"}
    try:
        write_fasta(src, b"chr_bench", raw)
        del raw
        emit(what="input", mbp=mbp, device=torch.cuda.get_device_name(0), bytes=os.path.getsize(src), rows=int(rows.size))
        if which == "both":
            write(src, out["plain"], rows, "plain")
            write(src, out["twobit"], rows, "twobit")
            with open(out["plain"], "rb") as fh:
                text = fh.read()
            seq = text[text.index(b"\n") + 1:].replace(b"\n", b"")
            want = twobit.pack_record(seq)
            with open(out["twobit"], "rb") as fh:
                got = fh.read()
            tb = twobit.open_twobit(out["twobit"])
            same = got[int(tb.rec_off[0]):] == want and tb.names == [b"chr_bench"]
            emit(what="2bit file is the file of the plain copy", ok=bool(same), bytes={k: os.path.getsize(p) for k, p in out.items()},
                 n_blocks=int(len(tb.n_iv)), mask_blocks=int(len(tb.m_iv)))
            del text, seq, want, got
            if not same:
                sys.exit("the two forms disagree: nothing is timed")
        ms = {f: [] for f in forms}
        for rep in range(warm + rounds):
            for form in forms:
                t = write(src, out[form], rows, form)
                if rep >= warm:
                    ms[form].append(t)
        for form in forms:
            emit(what="write_mask", form=form, ms=spread(ms[form]), mbp_per_s=round(n / (float(np.median(ms[form])) * 1e-3) / 1e6, 1),
                 note="file bytes in the page cache -> masked copy renamed into place in /dev/shm; upload, chunk table, mask, "
                      + ("pack, read-back of the blobs, spool and assembly" if form == "twobit" else "read-back of the text, write"))
    finally:
        for p in [src] + list(out.values()):
            if os.path.exists(p):
                os.unlink(p)


if __name__ == "__main__":
    main()
