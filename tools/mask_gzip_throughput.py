"""Cost of predict --mask_dir --mask_gzip on one synthetic 250 Mbp record (60-column lines, trained synthetic model, soft mask).
  cli      wall clock, best of two: predict alone, --mask_dir, --mask_dir --mask_gzip on the .fa and on its BGZF copy
  kernels  the encoder's kernel chain on the soft-masked text and the inflate kernel on the result, three times each in one process:
           run it under `rocprofv3 --kernel-trace --stats` (no counters) to see them side by side
  sizes    the unmasked, soft- and hard-masked text through the device encoder against host zlib (level 6 and Z_HUFFMAN_ONLY)
usage: mask_gzip_throughput.py cli|kernels|sizes [Mbp]"""
import os, sys, time, tempfile, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from deepgrp_amd import gz, synthetic, model as dgmodel
from deepgrp_amd.__main__ import main

what = sys.argv[1] if len(sys.argv) > 1 else "cli"
mbp = float(sys.argv[2]) if len(sys.argv) > 2 else 250
d = tempfile.mkdtemp()


def fasta_of(seq: bytes) -> bytes:
    return b">chr1\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n"


def texts():
    idx, lab = synthetic.synthetic_truth(int(mbp * 1e6))
    seq = np.frombuffer(b"ACGTN", np.uint8)[idx]
    out = {"unmasked": fasta_of(seq.tobytes())}
    if what != "cli":
        out["soft"] = fasta_of(np.where(lab > 0, seq | 0x20, seq).astype(np.uint8).tobytes())
    if what == "sizes":
        out["hard"] = fasta_of(np.where(lab > 0, np.uint8(78), seq).astype(np.uint8).tobytes())
    return out


if what == "cli":
    w = synthetic.trained_weights()
    mpath = os.path.join(d, "model.hdf5")
    dgmodel.save_keras_hdf5(mpath, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    fa, fz = os.path.join(d, "chr.fa"), os.path.join(d, "packed", "chr.fa.gz")
    os.makedirs(os.path.dirname(fz))
    data = texts()["unmasked"]
    with open(fa, "wb") as fh:
        fh.write(data)
    packed = "--mask_gzip" in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepgrp_amd", "__main__.py")).read()
    runs = [("predict", fa, []), ("mask_dir", fa, ["--mask_dir", os.path.join(d, "m1")])]
    if packed:                                                         # (a tree without the flag: the first two only)
        with open(fz, "wb") as fh:
            fh.write(gz.bgzf_compress_host(data))
        runs += [("mask_gzip", fa, ["--mask_dir", os.path.join(d, "m2"), "--mask_gzip"]),
                 ("mask_gzip_bgzf_in", fz, ["--mask_dir", os.path.join(d, "m3"), "--mask_gzip"])]
    del data
    best = {}
    for label, src, extra in runs:
        for it in range(2):
            t0 = time.perf_counter()
            main(["predict", mpath, src, "--output", os.path.join(d, "out.tsv")] + extra)
            dt = time.perf_counter() - t0
            best[label] = min(best.get(label, dt), dt)
            print(f"{label} run {it}: {mbp:g} Mbp in {dt:.3f} s = {mbp / dt:.0f} Mbp/s", flush=True)
    for label in best:
        print(f"best {label}: {best[label]:.3f} s = {best[label] / best['predict']:.3f}x of predict alone"
              + (f", {best[label] / best['mask_dir']:.3f}x of --mask_dir" if "mask_dir" in best else ""), flush=True)
    for sub in ("m1", "m2", "m3"):
        for name in sorted(os.listdir(os.path.join(d, sub))) if os.path.isdir(os.path.join(d, sub)) else []:
            print(f"{sub}/{name}: {os.path.getsize(os.path.join(d, sub, name))} bytes")
else:
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, data in texts().items():
        if what == "kernels" and name != "soft":
            continue
        d_text = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
        for it in range(3 if what == "kernels" else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_comp = gz.bgzf_compress_device(d_text)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{name}: {len(data)} bytes -> {d_comp.numel()} on the device in {dt * 1e3:.2f} ms (call, allocations included)", flush=True)
        comp = d_comp.cpu().numpy().tobytes()
        if what == "kernels":
            members = gz.walk_members(comp)
            for it in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                back = gz.inflate_device("<buffer>", members, dev, lambda _p, _n, _d: d_comp)
                torch.cuda.synchronize()
                print(f"{name}: inflated again in {(time.perf_counter() - t0) * 1e3:.2f} ms", flush=True)
            assert torch.equal(back, d_text)
        else:
            z6 = len(gz.bgzf_compress(data, 6))
            zh = len(gz.bgzf_compress(data, 6, zlib.Z_HUFFMAN_ONLY))
            print(f"{name}: ratio {len(data) / len(comp):.3f}; zlib level 6 {z6} bytes ({len(data) / z6:.3f}), Z_HUFFMAN_ONLY {zh} bytes "
                  f"({len(data) / zh:.3f}); ours / Z_HUFFMAN_ONLY = {len(comp) / zh:.4f}", flush=True)
