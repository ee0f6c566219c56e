"""2bit input: the benchmark's synthetic chromosome of [Mbp] (default 250) in /dev/shm as .fa (60-column lines, as
bench.py writes it) and as .2bit (N runs as N blocks, lower case as mask blocks), and both ingests timed in turn in one process:
file bytes in the page cache -> DeviceRecords ready (host clock around read_multi_fasta_device and a device synchronise), then
upload and encode separately between device events.  [warm-up] untimed rounds (default 2), then [runs] timed rounds (default 7),
the two forms alternating; median, smallest and largest of each.  The class indices of the two ingests are compared first.  One
JSON line per result.
    python tools/twobit_throughput.py [Mbp] [runs] [warm-up]"""
import json
import mmap
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import write_fasta  # noqa: E402
from deepgrp_amd import fasta, synthetic, twobit  # noqa: E402
from deepgrp_amd._lib import lib  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def _runs(inside: np.ndarray):
    edge = np.diff(np.concatenate(([0], inside.view(np.int8), [0])))
    start = np.flatnonzero(edge == 1)
    return start, np.flatnonzero(edge == -1) - start


def write_twobit(path, name: bytes, raw: bytes) -> None:
    """One record in the writer's order: N runs as N blocks (T stored under them), lower-case runs as mask blocks."""
    seq = np.frombuffer(raw, np.uint8)
    up = seq & 0xDF
    code = np.zeros(256, np.uint8)
    code[ord("C")], code[ord("A")], code[ord("G")] = 1, 2, 3
    c = code[up]
    c = np.concatenate([c, np.zeros((-c.size) % 4, np.uint8)]).reshape(-1, 4)
    packed = (c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]
    tables = b""
    for inside in (up == ord("N"), seq >= 97):
        start, size = _runs(inside)
        tables += struct.pack("<I", start.size) + start.astype("<u4").tobytes() + size.astype("<u4").tobytes()
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IIII", twobit.SIGNATURE, 0, 1, 0) + bytes([len(name)]) + name + struct.pack("<I", 16 + 1 + len(name) + 4))
        fh.write(struct.pack("<I", seq.size) + tables + struct.pack("<I", 0) + packed.tobytes())


def stages_fasta(L, dev, path):
    """(upload ms, chunk table + encode ms) of the FASTA ingest's two stages, between events."""
    size = os.path.getsize(path)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_COPY) as mm:
        e[0].record()
        d_file = fasta._upload_file(path, size, dev)
        e[1].record()
        for grp in fasta._chunk_groups(L, dev, path, mm, 0, size, 256 << 20, 4096, d_file=d_file):
            del grp
        e[2].record()
        torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def stages_twobit(L, dev, path):
    """(upload ms, encode ms) of the 2bit ingest's two stages (the host parse comes before both and is timed by the caller)."""
    tb = twobit.open_twobit(path)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    dtb = twobit.DeviceTwoBit(tb, dev, fasta._upload_file)
    e[1].record()
    d_idx, _off = dtb.encode(0, tb.nrec)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def ingest(path):
    torch.cuda.synchronize()
    t = time.perf_counter()
    recs = list(fasta.read_multi_fasta_device(path))
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, recs


def spread(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(float(np.min(xs)), 3), max=round(float(np.max(xs)), 3), n=len(xs))


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 250.0
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    n = int(mbp * 1e6)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = lib()
    raw = synthetic.synthetic_chromosome(n, contig=0)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else "/tmp"
    paths = {"fa": os.path.join(shm, f"dgrp_2bit_{os.getpid()}.fa"), "2bit": os.path.join(shm, f"dgrp_2bit_{os.getpid()}.2bit")}
    try:
        write_fasta(paths["fa"], b"chr_bench", raw)
        write_twobit(paths["2bit"], b"chr_bench", raw)
        tb = twobit.open_twobit(paths["2bit"])
        emit(what="inputs", mbp=mbp, device=torch.cuda.get_device_name(0), bytes={k: os.path.getsize(p) for k, p in paths.items()},
             n_blocks=int(len(tb.n_iv)), mask_blocks=int(len(tb.m_iv)))
        (_ms, a), (_ms, b) = ingest(paths["fa"]), ingest(paths["2bit"])
        same = len(a) == len(b) == 1 and a[0][0] == b[0][0] and (a[0][1].startpos, a[0][1].length) == (b[0][1].startpos, b[0][1].length) \
            and bool(torch.equal(a[0][1].d_idx, b[0][1].d_idx))
        emit(what="indices identical", ok=same)
        del a, b
        if not same:
            sys.exit("the two ingests disagree: nothing is timed")
        stage = {"fa": stages_fasta, "2bit": stages_twobit}
        e2e, up, enc, parse = ({"fa": [], "2bit": []} for _ in range(4))
        for rep in range(warm + runs):
            for form in ("fa", "2bit"):
                ms, recs = ingest(paths[form])
                del recs
                u, k = stage[form](L, dev, paths[form])
                t = time.perf_counter()
                if form == "2bit":
                    twobit.open_twobit(paths[form])
                p = (time.perf_counter() - t) * 1e3
                if rep >= warm:
                    e2e[form].append(ms), up[form].append(u), enc[form].append(k), parse[form].append(p)
        for form in ("fa", "2bit"):
            emit(what="ingest", form=form, file_to_records_ms=spread(e2e[form]), upload_ms=spread(up[form]),
                 encode_ms=spread(enc[form]), host_parse_ms=spread(parse[form]),
                 mbp_per_s=round(n / (float(np.median(e2e[form])) * 1e-3) / 1e6, 1),
                 note="encode of fa = chunk table + dgrp_fasta_encode_batch (with its read-back); of 2bit = dgrp_twobit_encode_batch")
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.unlink(p)


if __name__ == "__main__":
    main()
