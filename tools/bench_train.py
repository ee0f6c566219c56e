#!/usr/bin/env python3
"""Time one training step (forward, backward through time, optimizer) of the hand-written kernels and of the same model built from
torch.nn.GRU with autograd and torch.optim.RMSprop on the same GPU, at two shapes:

  defaults   batch 256, T 342, 60 units, attention      (the reference's defaults.toml)
  benchmark  batch 256, T 200, 128 units, no attention  (the benchmark model)

Method: the inputs of a step (start positions, dropout masks; for torch the one-hot windows and targets) are on the device before the
clock starts; 5 warm-up steps of each, then `--rounds` rounds, each a block of `--steps` HIP steps and a block of `--steps` torch steps
in the same process, alternating (the order of the two blocks swaps every round), each block timed with one pair of events; the median
block, the fastest and the slowest are reported per step.  `--hip-only N` runs N HIP steps per shape and nothing else: the pass for
`rocprofv3 --kernel-trace --stats` (where the step's time goes).  The torch model gets what this trainer cannot avoid either: dropout
of the inputs, both directions with shared weights, the attention head, Keras' loss.  Prints one JSON line per shape.

    python tools/bench_train.py [--steps 20] [--rounds 5] [--out profiles/train_step.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"defaults": dict(batch=256, T=342, units=60, attention=True), "benchmark": dict(batch=256, T=200, units=128, attention=False)}
COMP = [3, 2, 1, 0, 4]


class TorchModel(torch.nn.Module):
    def __init__(self, units, classes, attention):
        super().__init__()
        self.gru = torch.nn.GRU(5, units, batch_first=True)
        self.scale = torch.nn.Parameter(torch.randn(units) * 0.1) if attention else None
        self.ff = torch.nn.Linear(units * (2 if attention else 1), classes)

    def forward(self, x, masks):
        rc = x.flip(1)[:, :, COMP]
        fwd, hf = self.gru(x * masks[:, 0, None, :])
        rev, hr = self.gru(rc * masks[:, 1, None, :])
        avg = (fwd + rev) / 2
        if self.scale is not None:
            q = ((hf[0] + hr[0]) / 2)[:, None, :]
            a = torch.softmax((self.scale * torch.tanh(q + avg)).sum(-1), 1)
            ctx = (a[:, :, None] * avg).sum(1)
            avg = torch.cat([ctx[:, None, :].expand(-1, avg.shape[1], -1), avg], 2)
        return torch.softmax(self.ff(avg), 2)


def block_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def timed_pair(first, second, steps, rounds):
    """Alternating blocks of the two step functions; per function median / min / max milliseconds per step."""
    for fn in (first, second):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = ([], [])
    for r in range(rounds):
        for k in ((0, 1) if r % 2 == 0 else (1, 0)):
            out[k].append(block_ms((first, second)[k], steps))
    return [dict(median_ms=float(np.median(o)), min_ms=float(min(o)), max_ms=float(max(o))) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", type=int, default=0, help="run this many HIP steps per shape and nothing else (profiler pass)")
    args = ap.parse_args()
    from deepgrp_amd import synthetic, training
    results = []
    for name, sh in SHAPES.items():
        B, T, u, att, C = sh["batch"], sh["T"], sh["units"], sh["attention"], 5
        idx, lab = synthetic.synthetic_truth(400_000, contig=1, flank=0)
        truth = np.zeros((C, idx.size), np.int8)
        truth[lab, np.arange(idx.size)] = 1
        rng = np.random.default_rng(0)
        starts = torch.from_numpy(rng.integers(0, idx.size - T, B).astype(np.int64)).cuda()
        masks = torch.from_numpy(training.dropout_masks(rng, B, 0.25)).cuda()
        trainer = training.DeviceTrainer(synthetic.synthetic_weights(u, C, att, seed=1), T, B)
        record = training.DeviceRecord(idx, truth)
        loss = torch.empty(1, device="cuda")

        def hip_step():
            trainer.run(record, starts, masks, loss_out=loss)
            trainer.apply("RMSprop", 1e-3, 0.9, 0.9, 1e-10)

        if args.hip_only:
            for _ in range(args.hip_only):
                hip_step()
            torch.cuda.synchronize()
            continue

        model = TorchModel(u, C, att).cuda()
        opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, alpha=0.9, momentum=0.9, eps=1e-10)
        win = record.d_idx[(starts[:, None] + torch.arange(T, device="cuda")[None, :])].long().clamp(max=4)
        x = torch.eye(5, device="cuda")[win]
        y = record.d_truth[:, starts[:, None] + torch.arange(T, device="cuda")[None, :]].permute(1, 2, 0).float()

        def torch_step():
            opt.zero_grad(set_to_none=True)
            p = model(x, masks)
            p = (p / p.sum(-1, keepdim=True)).clamp(1e-7, 1 - 1e-7)
            (-(y * torch.log(p)).sum(-1).mean()).backward()
            opt.step()

        hip, ref = timed_pair(hip_step, torch_step, args.steps, args.rounds)
        row = dict(shape=name, **sh, steps=args.steps, rounds=args.rounds, hip=hip, torch=ref,
                   hip_over_torch=hip["median_ms"] / ref["median_ms"], device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
