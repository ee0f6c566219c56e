#!/usr/bin/env python3
"""Time K independent training steps as ONE dgrp_train_step_multi (plus their K optimizer steps) against the same K jobs as K
sequential dgrp_train_step calls (each followed by its optimizer step), in the same process on the same buffers.

Cases: K = 1, 2, 4, 8 copies (own parameters, starts and masks) of the two shapes of tools/bench_train.py, and one cohort of eight
models drawn with a fixed seed from the space of the reference's notebook (vecsize ~ qnormal(200, 20, 2), gru_units ~
qnormal(34, 5, 2), batch 256, attention).

Method (as tools/bench_train.py): inputs on the device before the clock starts; 5 warm-up steps of each side, then `--rounds`
rounds, each a block of `--steps` multi steps and a block of `--steps` sequential steps, alternating (the order swaps every round),
each block timed with one pair of events; the median block, the fastest and the slowest are reported per step (a step = all K
jobs).  `--multi-only N` runs N multi steps per case and nothing else: the pass for `rocprofv3 --kernel-trace --stats`.  Prints one
JSON line per case.

    python tools/bench_train_multi.py [--steps 10] [--rounds 5] [--cases defaults:8,notebook] [--out profiles/train_multi.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_train import SHAPES, timed_pair  # noqa: E402

NOTEBOOK_SPACE = {"vecsize": ["qnormal", 200, 20, 2], "gru_units": ["qnormal", 34, 5, 2]}
NOTEBOOK_SEED = 2020


def cases():
    from deepgrp_amd import optimization
    out = []
    for name, sh in SHAPES.items():
        for k in (1, 2, 4, 8):
            out.append((f"{name}:{k}", [dict(sh)] * k))
    rng = np.random.default_rng(NOTEBOOK_SEED)
    drawn = [optimization.sample_space(NOTEBOOK_SPACE, rng) for _ in range(8)]
    out.append(("notebook", [dict(batch=256, T=int(d["vecsize"]), units=int(d["gru_units"]), attention=True) for d in drawn]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=None, help="comma-separated case names (defaults:1 .. benchmark:8, notebook); default all")
    ap.add_argument("--out", default=None)
    ap.add_argument("--multi-only", type=int, default=0, help="run this many multi steps per case and nothing else (profiler pass)")
    args = ap.parse_args()
    from deepgrp_amd import synthetic, training
    C = 5
    idx, lab = synthetic.synthetic_truth(400_000, contig=1, flank=0)
    truth = np.zeros((C, idx.size), np.int8)
    truth[lab, np.arange(idx.size)] = 1
    record = training.DeviceRecord(idx, truth)
    wanted = args.cases.split(",") if args.cases else None
    results = []
    for name, models in cases():
        if wanted is not None and name not in wanted:
            continue
        rng = np.random.default_rng(0)
        trainers, inputs = [], []
        for k, m in enumerate(models):
            starts = torch.from_numpy(rng.integers(0, idx.size - m["T"], m["batch"]).astype(np.int64)).cuda()
            masks = torch.from_numpy(training.dropout_masks(rng, m["batch"], 0.25)).cuda()
            trainers.append(training.DeviceTrainer(synthetic.synthetic_weights(m["units"], C, m["attention"], seed=1 + k), m["T"], m["batch"]))
            inputs.append((starts, masks, torch.empty(1, device="cuda")))

        def apply(tr):
            tr.apply("RMSprop", 1e-3, 0.9, 0.9, 1e-10)

        def multi_step():
            training.run_jobs([tr.job(record, s, m, loss_out=l) for tr, (s, m, l) in zip(trainers, inputs)])
            for tr in trainers:
                apply(tr)

        def sequential_step():
            for tr, (s, m, l) in zip(trainers, inputs):
                tr.run(record, s, m, loss_out=l)
                apply(tr)

        if args.multi_only:
            for _ in range(args.multi_only):
                multi_step()
            torch.cuda.synchronize()
            continue
        multi, seq = timed_pair(multi_step, sequential_step, args.steps, args.rounds)
        K = len(models)
        row = dict(case=name, jobs=K, models=models if name == "notebook" else models[0], steps=args.steps, rounds=args.rounds,
                   multi=multi, sequential=seq, multi_over_sequential=multi["median_ms"] / seq["median_ms"],
                   multi_ms_per_job=multi["median_ms"] / K, sequential_ms_per_job=seq["median_ms"] / K,
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        results.append(row)
        del trainers, inputs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
