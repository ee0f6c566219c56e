#!/usr/bin/env python
"""Seeded search for a DEFLATE stream in which the block finder of the plain-gzip path accepts a bit offset that is no block start,
so that the chain has to repair it (dgrp_inflate_stream_stats.false_starts > 0).  Runs on the CPU, on the host entry.

Such offsets are rare, and one matters only when it lies in the chunk the chain lands in, in front of the landing.  So the search
has two steps over level-1 FASTA streams (tests/gzip_stream_cases.fasta_text(seed, nbases)):
  1. at the smallest chunk size (64 bytes) nearly every bit offset of the stream is put to the whole filter; a stream whose finder
     reports more starts than it has blocks holds a false one somewhere;
  2. for such a stream, chunk sizes are swept until the false start falls into a landing chunk in front of the landing.
The seed, size and chunk it prints are what tests/gzip_stream_cases.FALSE_START pins; the bytes are rebuilt from them."""
import argparse
import ctypes as C
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--first", type=int, default=100)
    ap.add_argument("--seeds", type=int, default=400)
    ap.add_argument("--nbases", type=int, default=1_500_000)
    args = ap.parse_args()
    import gzip_stream_cases as gc
    from deepgrp_amd._lib import InflateStreamStats, lib
    L = lib()

    def stats(comp, text, chunk):
        out = (C.c_uint8 * len(text))()
        ol, iu, r, st = C.c_int64(), C.c_int64(), C.c_int(), InflateStreamStats()
        rc = L.dgrp_inflate_stream_host(comp, len(comp), chunk, gc.MAX_SPAN, 1 << 20, out, len(text), C.byref(ol), C.byref(iu), C.byref(st),
                                        C.byref(r))
        assert rc == 0 and bytes(out) == text, (chunk, rc, r.value)
        return st.as_dict()

    t0, bits, hits = time.time(), 0, 0
    for seed in range(args.first, args.first + args.seeds):
        text = gc.fasta_text(seed, args.nbases)
        comp = gc.deflate(text, 1)
        assert zlib.decompress(comp, -15) == text
        bits += 8 * len(comp)
        st = stats(comp, text, 64)
        # every block is a span here: the first one, those the finder reported, and those the chain had to put in
        if 1 + st["candidates"] + st["repaired"] - st["false_starts"] <= st["spans"]:
            continue
        print(f"seed {seed}: a false start somewhere ({st}); {bits / 1e6:.0f} M bit offsets walked, {time.time() - t0:.0f} s", flush=True)
        for chunk in range(1 << 10, 160 << 10, 1 << 10):
            st = stats(comp, text, chunk)
            if st["false_starts"]:
                print(f"FALSE_START seed {seed} nbases {args.nbases} chunk {chunk}: {st}", flush=True)
                hits += 1
                break
    print(f"{hits} found in {bits / 1e6:.0f} M bit offsets of {args.seeds} streams, {time.time() - t0:.0f} s")
    return 0 if hits else 1


if __name__ == "__main__":
    sys.exit(main())
