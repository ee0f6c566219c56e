"""Compressed input: one synthetic record of [Mbp] (default 250) in /dev/shm as .fa, as BGZF (level 6, written
with Python's zlib the way bgzip lays it out) and as plain gzip (level 6, one member).  For each form the end-to-end rate of
bench.py's e2e leg (read_multi_fasta_device -> RecordRunner -> TSV bytes in host memory), then the inflate kernel alone
(dgrp_inflate_batch on the uploaded BGZF file, GB/s of output) and host zlib on the same files.  One JSON line per result.
    python tools/gz_throughput.py [Mbp]"""
import ctypes as C
import json
import os
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import BATCH, MIN_MSS, STEP, T, XDROP, write_fasta  # noqa: E402
from deepgrp_amd import gz, synthetic  # noqa: E402
from deepgrp_amd._lib import check, lib  # noqa: E402
from deepgrp_amd.fasta import _upload_file, read_multi_fasta_device  # noqa: E402
from deepgrp_amd.pipeline import ContigPipeline, DeviceModel, stream_ptr  # noqa: E402
from deepgrp_amd.runner import RecordRunner, rows_text, rows_text_batch  # noqa: E402


def _bgzf_piece(args):
    data, = args
    return gz.bgzf_compress(data, 6, eof=False)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250.0
    n = int(mbp * 1e6)
    torch.cuda.set_device(0)
    raw = synthetic.synthetic_chromosome(n, contig=0)
    w = synthetic.trained_weights()
    model = DeviceModel(w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], w["scale"], vecsize=T)
    pipe = ContigPipeline(model, STEP, BATCH, MIN_MSS, XDROP, use_mss=True)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else "/tmp"
    base = os.path.join(shm, f"dgrp_gz_{os.getpid()}")
    paths = {"fa": base + ".fa", "bgzf": base + ".bgzf.fa.gz", "gzip": base + ".gzip.fa.gz"}
    try:
        write_fasta(paths["fa"], b"chr_bench", raw)
        text = open(paths["fa"], "rb").read()
        t = time.perf_counter()
        step = gz.BGZF_BLOCK * 64                                          # 64 members per worker task, bgzip's member size
        with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            pieces = list(ex.map(_bgzf_piece, [(text[o:o + step],) for o in range(0, len(text), step)]))
        with open(paths["bgzf"], "wb") as fh:
            fh.write(b"".join(pieces) + gz.BGZF_EOF)
        t_bgzf = time.perf_counter() - t
        t = time.perf_counter()
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        with open(paths["gzip"], "wb") as fh:
            fh.write(co.compress(text) + co.flush())
        t_gzip = time.perf_counter() - t
        sizes = {k: os.path.getsize(p) for k, p in paths.items()}
        emit(what="inputs", mbp=mbp, bytes=sizes, ratio_bgzf=round(sizes["fa"] / sizes["bgzf"], 3),
             ratio_gzip=round(sizes["fa"] / sizes["gzip"], 3), write_s={"bgzf": round(t_bgzf, 2), "gzip": round(t_gzip, 2)})

        def file_to_tsv(path):
            runner = RecordRunner(pipe)
            parts = []
            for kind, key, rows in runner.results(read_multi_fasta_device(path)):
                parts.append(rows_text_batch(path, key, rows) if kind == "batch" else rows_text(path, key, rows))
            return "".join(parts).encode()

        tsv = {}
        for form in ("fa", "bgzf", "gzip", "fa"):                        # .fa again last: the same session's drift
            file_to_tsv(paths[form])
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = file_to_tsv(paths[form])
                ts.append(time.perf_counter() - t)
            tsv.setdefault(form, out.replace(paths[form].encode(), b"<file>"))
            emit(what="e2e", form=form, mbp_per_s=round(n / float(np.mean(ts)) / 1e6, 3), ms=round(float(np.mean(ts)) * 1e3, 3),
                 ms_each=[round(x * 1e3, 3) for x in ts], rows=out.count(b"\n"))
        emit(what="tsv identical", bgzf=tsv["bgzf"] == tsv["fa"], gzip=tsv["gzip"] == tsv["fa"])

        # ---- the inflate kernel alone, on the uploaded BGZF file
        dev = torch.device("cuda", 0)
        with open(paths["bgzf"], "rb") as fh:
            comp = fh.read()
        t = time.perf_counter()
        members = gz.walk_members(comp, paths["bgzf"])
        t_walk = time.perf_counter() - t
        L = lib()
        nmem = int(members.start.size)
        out_off = np.zeros(nmem + 1, np.int64)
        np.cumsum(members.isize, out=out_off[1:])
        total = int(out_off[-1])
        t = time.perf_counter()
        d_in = _upload_file(paths["bgzf"], members.size, dev)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t
        d_out = torch.empty(total, dtype=torch.uint8, device=dev)
        wb = int(L.dgrp_inflate_workspace_bytes(nmem))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        bad, reason = C.c_int64(), C.c_int()
        ms = []
        for rep in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(L.dgrp_inflate_batch(d_in.data_ptr(), members.size, nmem, members.data_off.ctypes.data, members.data_len.ctypes.data,
                                       out_off.ctypes.data, d_out.data_ptr(), total, C.byref(bad), C.byref(reason), work.data_ptr(),
                                       wb, stream_ptr()), "dgrp_inflate_batch")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
        assert d_out.cpu().numpy().tobytes() == text
        emit(what="inflate kernel", members=nmem, out_bytes=total, ms=round(float(np.mean(ms)), 3), ms_each=[round(x, 3) for x in ms],
             gb_per_s=round(total / (float(np.mean(ms)) * 1e-3) / 1e9, 2), member_walk_ms=round(t_walk * 1e3, 2),
             upload_ms=round(t_up * 1e3, 2), note="events around the synchronous call: launch, kernel, status read-back")

        # ---- host zlib on the same files (one core)
        for form in ("bgzf", "gzip"):
            with open(paths[form], "rb") as fh:
                comp = fh.read()
            t = time.perf_counter()
            plain = gz.inflate_host(comp, paths[form], 1 << 40)
            dt = time.perf_counter() - t
            assert len(plain) == len(text)
            emit(what="host zlib", form=form, ms=round(dt * 1e3, 1), mb_per_s=round(len(text) / dt / 1e6, 1))
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.unlink(p)


if __name__ == "__main__":
    main()
