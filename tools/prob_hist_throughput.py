"""The histogram kernel of `evaluate --curves` alone (dgrp_prob_hist_batch): one record of MBP million bases, C classes,
trained-model-like probabilities (98 % of the elements within 1e-4 of 0 or 1) and a random truth track, both made on the GPU.
Prints the kernel's time (events around the entry, median of RUNS), the floor (4 C + 1) n bytes at the HBM rate the project's
streaming kernels reach, and the time of a plain torch statement of the same counts on the same arrays (one multiply, one clamp and
one bincount over a combined key), after checking that the two agree.  Under `rocprofv3 --kernel-trace --stats` (a run of its own,
with --no-torch) prob_hist_kernel's own device time shows.

    python tools/prob_hist_throughput.py [MBP] [--classes C] [--bins N] [--runs R] [--uniform] [--no-torch] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepgrp_amd._lib import check, lib
from deepgrp_amd.pipeline import require_gpu, stream_ptr

HBM_RATE = 4.5e12                                   # bytes per second: the read-side streaming kernels reach 4.2-5.2 TB/s

ap = argparse.ArgumentParser()
ap.add_argument("mbp", nargs="?", type=float, default=250.0)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--bins", type=int, default=1000)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--uniform", action="store_true", help="uniform probabilities instead of the trained-model-like mix")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = require_gpu()
L = lib()
n, C, bins = int(args.mbp * 1e6), args.classes, args.bins
g = torch.Generator(device=dev).manual_seed(1)
truth = torch.randint(0, C, (n,), generator=g, device=dev, dtype=torch.int8)
probs = torch.rand((n, C), generator=g, device=dev, dtype=torch.float32)
if not args.uniform:
    probs.mul_(1e-4)                                                    # near 0 ...
    call = torch.where(torch.rand(n, generator=g, device=dev) < 0.9, truth.long(), torch.randint(0, C, (n,), generator=g, device=dev))
    probs.scatter_(1, call[:, None], 1 - probs.gather(1, call[:, None]))        # ... the called class near 1 ...
    loose = torch.rand((n, C), generator=g, device=dev) < 0.02
    probs = torch.where(loose, torch.rand((n, C), generator=g, device=dev), probs)      # ... and 2 % anywhere
    del call, loose
row0, ln, off = (np.array([v], np.int64) for v in (0, n, 0))
wb = int(L.dgrp_prob_hist_workspace_bytes(1, C, bins))
work = torch.empty(wb, dtype=torch.uint8, device=dev)
d_hist = torch.empty((C, 2, bins), dtype=torch.int64, device=dev)
d_bad = torch.empty(1, dtype=torch.int32, device=dev)


def hip():
    check(L.dgrp_prob_hist_batch(probs.data_ptr(), C, 1, row0.ctypes.data, ln.ctypes.data, truth.data_ptr(), off.ctypes.data, bins,
                                 d_hist.data_ptr(), d_bad.data_ptr(), work.data_ptr(), wb, stream_ptr()), "dgrp_prob_hist_batch")
    return d_hist


def plain_torch():
    """The same counts with stock operators: key = (class, truth == class, bin) per element, one bincount."""
    k = (probs * float(bins)).to(torch.int64).clamp_(max=bins - 1)
    cls = torch.arange(C, device=dev, dtype=torch.int64)
    k += (cls * 2 + (truth[:, None] == cls).to(torch.int64)) * bins
    return torch.bincount(k.view(-1), minlength=C * 2 * bins).view(C, 2, bins)


def timed(f, runs):
    f()                                                                 # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


out = dict(mbp=args.mbp, classes=C, bins=bins, values="uniform" if args.uniform else "trained-like", runs=args.runs,
           bytes=(4 * C + 1) * n, floor_ms=(4 * C + 1) * n / HBM_RATE * 1e3)
out["hip_ms_median"], out["hip_ms_best"] = timed(hip, args.runs)
assert int(d_bad.item()) == 0 and int(d_hist.sum().item()) == n * C
out["hip_GBps"] = out["bytes"] / out["hip_ms_median"] / 1e6
out["hip_over_floor"] = out["hip_ms_median"] / out["floor_ms"]
if not args.no_torch:
    assert torch.equal(plain_torch(), hip())
    out["torch_ms_median"], out["torch_ms_best"] = timed(plain_torch, max(3, args.runs // 2))
    out["torch_over_hip"] = out["torch_ms_median"] / out["hip_ms_median"]
end = d_hist[:, :, [0, bins - 1]].sum().item() / (n * C)
out["share_in_end_bins"] = end
print(json.dumps(out), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
