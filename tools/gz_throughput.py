"""Compressed input: one synthetic record of [Mbp] (default 250) in /dev/shm as .fa, as BGZF (level 6, written
with Python's zlib the way bgzip lays it out) and as plain gzip (level 6, one member).  For each form the end-to-end rate of
bench.py's e2e leg (read_multi_fasta_device -> RecordRunner -> TSV bytes in host memory), then the inflate kernel alone
(dgrp_inflate_batch on the uploaded BGZF file, GB/s of output) and host zlib on the same files.  The plain-gzip file goes in twice,
through the device path (dgrp_inflate_stream_scan / _write) and through zlib with the device path switched off by
gz.PLAIN_DEVICE_MIN_BYTES; scan and write are timed alone as well, with the chain's statistics.  One JSON line per result.
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

        # three alternating rounds of the four ways in: plain gzip on the device, plain gzip through zlib (the device path switched
        # off by its constant), BGZF, and the text itself
        ways = {"gzip_device": ("gzip", 0), "gzip_host": ("gzip", float("inf")), "bgzf": ("bgzf", None), "fa": ("fa", None)}
        shipped = gz.PLAIN_DEVICE_MIN_BYTES
        tsv, ts = {}, {k: [] for k in ways}

        def run(way):
            form, min_bytes = ways[way]
            gz.PLAIN_DEVICE_MIN_BYTES = shipped if min_bytes is None else min_bytes
            try:
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = file_to_tsv(paths[form])
                return time.perf_counter() - t, out
            finally:
                gz.PLAIN_DEVICE_MIN_BYTES = shipped
        for way in ways:
            run(way)
        for _ in range(3):
            for way in ways:
                dt, out = run(way)
                ts[way].append(dt)
                tsv[way] = out.replace(paths[ways[way][0]].encode(), b"<file>")
        for way in ways:
            emit(what="e2e", form=way, mbp_per_s=round(n / float(np.mean(ts[way])) / 1e6, 3), ms=round(float(np.mean(ts[way])) * 1e3, 3),
                 ms_each=[round(x * 1e3, 3) for x in ts[way]], rows=tsv[way].count(b"\n"))
        emit(what="tsv identical", bgzf=tsv["bgzf"] == tsv["fa"], gzip_device=tsv["gzip_device"] == tsv["fa"],
             gzip_host=tsv["gzip_host"] == tsv["fa"], shipped_min_bytes=str(shipped))

        # ---- scan and write alone, on the uploaded plain gzip file, at the shipped chunk size and at others
        from deepgrp_amd._lib import InflateStreamStats
        dev = torch.device("cuda", 0)
        L = lib()
        size = sizes["gzip"]
        with open(paths["gzip"], "rb") as fh:
            data_off = gz.plain_data_off(fh.read(4096))
        d_in = _upload_file(paths["gzip"], size, dev)
        for chunk in sorted({gz.PLAIN_CHUNK_BYTES, 16 << 10, 32 << 10, 64 << 10, 128 << 10}):
            wb = int(L.dgrp_inflate_stream_workspace_bytes(size, chunk))
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
            total, st, reason, crc, used = C.c_int64(), InflateStreamStats(), C.c_int(), C.c_uint32(), C.c_int64()
            t_scan, t_write = [], []
            for rep in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                check(L.dgrp_inflate_stream_scan(d_in.data_ptr(), size, data_off, chunk, gz.PLAIN_MAX_SPAN_BYTES, gz.PLAIN_MAX_ROUNDS,
                                                 C.byref(total), C.byref(st), C.byref(reason), work.data_ptr(), wb, stream_ptr()), "scan")
                t_scan.append(time.perf_counter() - t)
                d_out = torch.empty(total.value, dtype=torch.uint8, device=dev)
                d_sym = torch.empty(total.value, dtype=torch.int16, device=dev)
                torch.cuda.synchronize()
                t = time.perf_counter()
                check(L.dgrp_inflate_stream_write(d_in.data_ptr(), size, data_off, chunk, d_sym.data_ptr(), d_out.data_ptr(), total.value,
                                                  C.byref(crc), C.byref(used), C.byref(reason), work.data_ptr(), wb, stream_ptr()), "write")
                t_write.append(time.perf_counter() - t)
            same = d_out.cpu().numpy().tobytes() == text and crc.value == zlib.crc32(text) and used.value == size - 8
            emit(what="inflate stream", chunk_bytes=chunk, out_bytes=total.value, bytes_identical=same,
                 scan_ms=[round(x * 1e3, 2) for x in t_scan], write_ms=[round(x * 1e3, 2) for x in t_write], stats=st.as_dict())
            del d_out, d_sym, work

        # ---- the inflate kernel alone, on the uploaded BGZF file
        with open(paths["bgzf"], "rb") as fh:
            comp = fh.read()
        t = time.perf_counter()
        members = gz.walk_members(comp, paths["bgzf"])
        t_walk = time.perf_counter() - t
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
