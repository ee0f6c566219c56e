"""Where gru_split2_kernel's workgroups spend a launch: reads the clock stamps of the DIAGNOSTIC build (tools/build_split2_stamps.sh ->
build/ab/split2_stamps.so; gru_split2.hip, DGRP_SPLIT2_STAMPS) for one forward + merge launch of the benchmark's model at 50 and at
250 Mbp, once with the static stride (workgroup b walks b, b + G, ...: the launch shape in front of the queue) and once with the queue.

    tools/build_split2_stamps.sh && python tools/split2_stamps.py [MBP ...]

Per launch: the finish-time spread by blockIdx.x % 8 (the XCD of a workgroup) and by workgroup on the constant 100 MHz clock
(s_memrealtime), the clock each XCD held (shader cycles of s_memtime per tick of s_memrealtime), and the share of a pair spent in set-up,
time loop and drain (s_memtime at the four boundaries of every pair; nothing is stamped inside the time loop)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepgrp_amd import _lib                                                                     # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, "build", "ab", "split2_stamps.so")
from deepgrp_amd import synthetic                                                                # noqa: E402
from deepgrp_amd.pipeline import ContigPipeline, DeviceModel, upload_sequence                    # noqa: E402

T, S = 200, 50


def report(tag, st, npairs):
    """st: uint64 [G, 3 + 4 cap]"""
    G = st.shape[0]
    entry, exit_, nrun = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64), st[:, 2].astype(np.int64)
    assert int(nrun.sum()) == npairs, (int(nrun.sum()), npairs)
    cap = (st.shape[1] - 3) // 4
    assert int(nrun.max()) <= cap
    t0 = int(entry.min())
    span = int(exit_.max()) - t0
    us = lambda ticks: ticks / 100.0                                                             # 100 MHz
    fin = exit_ - t0
    idle_tail = (int(exit_.max()) - exit_).astype(np.float64)
    idle_head = (entry - t0).astype(np.float64)
    print(f"{tag}: {G} workgroups, {npairs} pairs ({npairs / G:.2f} rounds), launch {us(span):.1f} us on the device")
    print(f"{tag}: pairs per workgroup min {nrun.min()} max {nrun.max()}; entry spread {us(idle_head.max()):.1f} us; "
          f"finish min {us(fin.min()):.1f} median {us(np.median(fin)):.1f} max {us(fin.max()):.1f} us")
    print(f"{tag}: workgroup-time without a wave: {100 * idle_head.sum() / (G * span):.3f} % in front of the entry, "
          f"{100 * idle_tail.sum() / (G * span):.3f} % behind the exit")
    pp = st[:, 3:].reshape(G, cap, 4).astype(np.int64)
    setup = loop = drain = gap = 0
    clk = np.zeros(G)
    for b in range(G):
        k = int(nrun[b])
        q = pp[b, :k]
        setup += int((q[:, 1] - q[:, 0]).sum())
        loop += int((q[:, 2] - q[:, 1]).sum())
        drain += int((q[:, 3] - q[:, 2]).sum())
        gap += int((q[1:, 0] - q[:-1, 3]).sum())
        clk[b] = (q[-1, 3] - q[0, 0]) / max(1, exit_[b] - entry[b]) * 100.0                    # MHz, weight loads and exit included in the ticks
    tot = setup + loop + drain + gap
    print(f"{tag}: of a pair's {tot / npairs:.0f} shader cycles: set-up {100 * setup / tot:.3f} %, time loop {100 * loop / tot:.3f} %, "
          f"drain {100 * drain / tot:.3f} %, between pairs {100 * gap / tot:.3f} %  "
          f"(cycles per pair: set-up {setup / npairs:.0f}, loop {loop / npairs:.0f}, drain {drain / npairs:.0f})")
    print(f"{tag}: by blockIdx.x % 8:   pairs   clock MHz (min..max)   finish us (min..max)   cycles per pair")
    for x in range(8):
        sel = np.arange(G) % 8 == x
        if not sel.any():
            continue
        cyc = sum(int((pp[b, :nrun[b], 3] - pp[b, :nrun[b], 0]).sum()) for b in np.nonzero(sel)[0]) / max(1, int(nrun[sel].sum()))
        print(f"{tag}:   {x}   {int(nrun[sel].sum()):7d}   {clk[sel].mean():7.1f} ({clk[sel].min():.1f}..{clk[sel].max():.1f})   "
              f"{us(fin[sel].mean()):9.1f} ({us(fin[sel].min()):.1f}..{us(fin[sel].max()):.1f})   {cyc:.0f}")


def main():
    sizes = [float(a) for a in sys.argv[1:]] or [50.0, 250.0]
    L = _lib.lib()
    fn = L.dgrp_split2_stamps
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]
    dev = torch.device("cuda")
    G = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    w = synthetic.trained_weights()
    m = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=T)
    pipe = ContigPipeline(m, S, 256)
    assert m.plan(0, S, handle=pipe.handle).kernel == "split2"
    for mbp in sizes:
        _st, d = upload_sequence(synthetic.synthetic_chromosome(int(mbp * 1e6)))
        nwin = L.dgrp_window_count(d.numel(), T, S)
        npairs = (nwin + 31) // 32
        cap = 2 * ((npairs + G - 1) // G) + 8
        for static_walk in (1, 0, 1, 0):
            fn(None, 0, static_walk)
            for _ in range(3):                                                                   # warm, and at the clock the chip holds under this load
                pipe.merged(d)
            buf = torch.zeros((min(G, npairs), 3 + 4 * cap), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fn(buf.data_ptr(), cap, static_walk)
            pipe.merged(d)
            torch.cuda.synchronize()
            fn(None, 0, 0)
            report(f"{mbp:g} Mbp {'static' if static_walk else 'queue '}", buf.cpu().numpy().view(np.uint64), npairs)
            print(flush=True)
    pipe.close()
    m.close()


if __name__ == "__main__":
    main()
