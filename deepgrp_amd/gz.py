"""Compressed FASTA input (an addition; the reference reads plain text only).

A gzip file is recognised by its magic bytes, not by its name.  A BGZF file (every member carries the `BC` extra subfield with its
compressed size BSIZE, and inflates to at most 64 KiB) is split into its members by a walk over the member headers on the host;
the compressed file is uploaded as it is and the members are inflated side by side on the device (dgrp_inflate_batch), straight
into the buffer the FASTA ingest consumes.  A file of one plain member (as gzip and pigz write it) of at least
PLAIN_DEVICE_MIN_BYTES is uploaded as it is too and its one DEFLATE stream is inflated on the device as many spans
(dgrp_inflate_stream_scan / _write); whenever that path declines -- several members, a stream of stored or fixed blocks, a corrupt
file -- and for any other gzip file (members without `BC`) the file is
inflated on the host with zlib and uploaded.  Corrupt input raises GzipError naming the file and the compressed byte offset of
the first bad member.

The other direction (`predict --mask_dir --mask_gzip`): bgzf_compress_device deflates device bytes into BGZF members on the device
(dgrp_bgzf_compress_level: level 0 writes literals under a per-member Huffman code, level 1 adds matches inside the member);
bgzf_compress_host is the same encoder on the host.  `predict --track_dir --track_gzip` writes its tracks through it as well."""
from __future__ import annotations

import logging
import os
import struct
import zlib
from typing import Optional

import numpy as np

MAGIC = b"\x1f\x8b"
BGZF_MAX_ISIZE = 1 << 16
_LOG = logging.getLogger(__name__)

# DGRP_INFLATE_* (include/deepgrp_hip.h)
REASONS = {1: "input ends inside the DEFLATE stream", 2: "invalid block type", 3: "stored block LEN/NLEN mismatch",
           4: "invalid code lengths", 5: "invalid symbol", 6: "distance too far back", 7: "more output than ISIZE",
           8: "CRC-32 mismatch", 9: "output shorter than ISIZE", 10: "DEFLATE stream ends before the member's trailer",
           11: "a span longer than PLAIN_MAX_SPAN_BYTES (no block starts to find, as in a stream of stored or fixed blocks)",
           12: "the chain of spans is not closed after PLAIN_MAX_ROUNDS rounds"}


class GzipError(ValueError):
    """Corrupt or truncated gzip input: `path` and the compressed byte `offset` of the first bad member."""

    def __init__(self, path, offset: int, what: str):
        super().__init__(f"{path}: corrupt gzip input, member at compressed byte offset {offset}: {what}")
        self.path, self.offset = path, int(offset)


def is_gzip(path) -> bool:
    """The file starts with the gzip magic bytes 1f 8b (False for anything that cannot be opened)."""
    try:
        with open(path, "rb") as fh:
            return fh.read(2) == MAGIC
    except OSError:
        return False


def compressed_inputs(files):
    """The command-line inputs that are gzip files (stdin and the one-hot .npz are never)."""
    return [f for f in files if f != "-" and not f.endswith(".npz") and os.path.isfile(f) and is_gzip(f)]


class Members:
    """Result of the member walk.  kind = "bgzf" or "gzip"; for BGZF, per member: `start` (offset of its header), `data_off` and
    `data_len` (its DEFLATE data), `isize` (its trailer's ISIZE); `size` = compressed file size."""

    __slots__ = ("kind", "start", "data_off", "data_len", "isize", "size")

    def __init__(self, kind, size, start=(), data_off=(), data_len=(), isize=()):
        self.kind, self.size = kind, int(size)
        self.start, self.data_off, self.data_len, self.isize = (np.asarray(a, np.int64) for a in (start, data_off, data_len, isize))


def walk_members(buf, path="<buffer>") -> Members:
    """Classify the gzip bytes `buf` (bytes or a mapping of the file) by a walk over its member headers: "bgzf" when every member
    has FLG = FEXTRA, a `BC` subfield whose BSIZE frames it inside the file, and an ISIZE of at most 64 KiB; "gzip" as soon as a
    member does not (that file goes to zlib, which finds member ends by inflating).  A BGZF member whose header or BSIZE runs past
    the end of the file, or bytes after a BGZF member that are not a gzip member, raise GzipError."""
    n = len(buf)
    pos = 0
    start, doff, dlen, isize = [], [], [], []
    while pos < n:
        if n - pos < 12:
            if pos == 0 or buf[pos:pos + 2] == MAGIC[:n - pos]:
                raise GzipError(path, pos, "truncated member header")
            raise GzipError(path, pos, "not a gzip member")
        id12, cm, flg = buf[pos:pos + 2], buf[pos + 2], buf[pos + 3]
        if id12 != MAGIC:
            raise GzipError(path, pos, "not a gzip member")
        if cm != 8:
            raise GzipError(path, pos, f"compression method {cm} is not DEFLATE")
        if flg != 4:
            return Members("gzip", n)
        xlen = struct.unpack_from("<H", buf, pos + 10)[0]
        hlen = 12 + xlen
        if pos + hlen > n:
            raise GzipError(path, pos, "truncated member header")
        bsize, x = None, pos + 12
        while x + 4 <= pos + hlen:
            si1, si2, slen = buf[x], buf[x + 1], struct.unpack_from("<H", buf, x + 2)[0]
            if si1 == 66 and si2 == 67 and slen == 2 and x + 6 <= pos + hlen:
                bsize = struct.unpack_from("<H", buf, x + 4)[0]
            x += 4 + slen
        if bsize is None:
            return Members("gzip", n)
        end = pos + bsize + 1
        if bsize + 1 < hlen + 8:
            raise GzipError(path, pos, f"BSIZE {bsize} leaves no room for the header and trailer")
        if end > n:
            raise GzipError(path, pos, f"truncated member (BSIZE {bsize} runs past the end of the file at {n})")
        isz = struct.unpack_from("<I", buf, end - 4)[0]
        if isz > BGZF_MAX_ISIZE:
            return Members("gzip", n)
        start.append(pos)
        doff.append(pos + hlen)
        dlen.append(bsize + 1 - hlen - 8)
        isize.append(isz)
        pos = end
    return Members("bgzf", n, start, doff, dlen, isize)


def too_large(path, nbytes: int, limit: int) -> ValueError:
    return ValueError(f"{path}: inflates to more than {limit} bytes (DGRP_FASTA_RESIDENT_BYTES); compressed input is read whole "
                      "into device memory, so decompress this file and give the FASTA instead")


def inflate_host(buf, path, limit: int) -> bytearray:
    """Every member of the gzip bytes `buf` inflated with zlib (CRC-32 and ISIZE checked), concatenated.  Raises GzipError for a
    bad or truncated member and ValueError once the output exceeds `limit` bytes."""
    out = bytearray()
    n = len(buf)
    step = 1 << 20
    pos = 0
    while pos < n:
        d = zlib.decompressobj(31)
        o = pos
        while not d.eof:
            if o >= n:
                raise GzipError(path, pos, "truncated member")
            data = buf[o:o + step]                                   # (a copy: no view of the mapping outlives this call)
            o += len(data)
            while data:
                try:
                    piece = d.decompress(data, limit - len(out) + 1)
                except zlib.error as e:
                    raise GzipError(path, pos, str(e)) from None
                out += piece
                if len(out) > limit:
                    raise too_large(path, len(out), limit)
                data = d.unconsumed_tail
                if d.eof:
                    break
        pos = o - len(d.unused_data)
    return out


def inflate_device(path, members: Members, dev, upload):
    """The BGZF file's members inflated on the device into one buffer (uint8 tensor of sum(ISIZE) bytes).  `upload(path, size,
    dev)` puts the compressed file into HBM (the ingest's pinned-slab uploader)."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    nmem = int(members.start.size)
    out_off = np.zeros(nmem + 1, np.int64)
    np.cumsum(members.isize, out=out_off[1:])
    total = int(out_off[-1])
    d_in = upload(path, members.size, dev)
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    wb = int(L.dgrp_inflate_workspace_bytes(nmem))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    bad, reason = C.c_int64(-1), C.c_int(0)
    rc = L.dgrp_inflate_batch(d_in.data_ptr(), members.size, nmem, members.data_off.ctypes.data, members.data_len.ctypes.data,
                              out_off.ctypes.data, d_out.data_ptr(), total, C.byref(bad), C.byref(reason), work.data_ptr(), wb,
                              stream_ptr())
    if rc == -5:                                                     # DGRP_EDATA
        raise GzipError(path, int(members.start[bad.value]), REASONS.get(reason.value, f"reason {reason.value}"))
    check(rc, "dgrp_inflate_batch")
    return d_out


class DeviceText:
    """The inflated bytes of a BGZF file, resident on the device, as the ingest reads them on the host: `t[i]` and `t[a:b]` like
    the mapping of a plain file.  `prime` fetches every chunk's header line in one gather and one copy; any other slice (the body
    of a chunk that takes the reference loop) is copied when asked for."""

    def __init__(self, d_text):
        self.d = d_text
        self.spans, self.blob = {}, b""

    def prime(self, starts, head_ends) -> None:
        import torch
        st = np.asarray(starts[:len(head_ends)], np.int64)
        ln = np.asarray(head_ends, np.int64) - st
        offs = np.cumsum(ln) - ln
        total = int(ln.sum())
        if total:
            dev = self.d.device
            d_ln = torch.from_numpy(ln).to(dev)
            shift = torch.repeat_interleave(torch.from_numpy(st - offs).to(dev), d_ln, output_size=total)
            self.blob = self.d[torch.arange(total, device=dev) + shift].cpu().numpy().tobytes()
        self.spans = dict(zip(st.tolist(), zip(offs.tolist(), (st + ln).tolist())))

    def __getitem__(self, k):
        if isinstance(k, slice):
            a, b = k.start, k.stop
            hit = self.spans.get(a)
            if hit is not None and hit[1] == b:
                return self.blob[hit[0]:hit[0] + b - a]
            return self.d[a:b].cpu().numpy().tobytes()
        return int(self.d[k])


# ---- plain gzip (one member, one DEFLATE stream) on the device: dgrp_inflate_stream_scan / _write (include/deepgrp_hip.h).
# DESIGN 5d states each value with the run it came from.
PLAIN_CHUNK_BYTES = 16 << 10          # compressed bytes per chunk: one span start is looked for in each (below zlib's blocks of FASTA)
PLAIN_MAX_SPAN_BYTES = 1 << 20        # one wave decodes a span serially: above this it costs what zlib costs for a 70 MB file
PLAIN_MAX_ROUNDS = 16                 # counting rounds of the chain (one more for every start repaired behind a repaired one)
PLAIN_DEVICE_MIN_BYTES = 16 << 20     # compressed size from which the device path is taken (float("inf"): never)


def plain_data_off(buf) -> Optional[int]:
    """Offset of the DEFLATE data of the first gzip member of `buf` (FEXTRA, FNAME, FCOMMENT and FHCRC skipped), or None when the
    header is not one this parser takes or leaves no room for a trailer."""
    n = len(buf)
    if n < 18 or buf[0:2] != MAGIC or buf[2] != 8 or buf[3] & 0xe0:
        return None
    flg, pos = buf[3], 10
    if flg & 4:
        pos += 2 + struct.unpack_from("<H", buf, pos)[0]
    for bit in (8, 16):                                              # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            if pos >= n:
                return None
            end = buf.find(b"\0", pos)
            if end < 0:
                return None
            pos = end + 1
    if flg & 2:
        pos += 2
    return pos if pos <= n - 8 else None


def inflate_stream_device(path, size: int, data_off: int, limit: int, dev, upload):
    """The one-member gzip file `path` inflated on the device.  -> (uint8 device tensor, None) when scan and write succeed, the
    final block ends 8 bytes before the end of the file and CRC-32 and ISIZE match the trailer; (None, why not) otherwise.  Raises
    only the `too_large` error."""
    import ctypes as C

    import torch

    from ._lib import InflateStreamStats, check, lib
    from .pipeline import stream_ptr
    L = lib()
    d_in = upload(path, size, dev)
    wb = int(L.dgrp_inflate_stream_workspace_bytes(size, PLAIN_CHUNK_BYTES))
    if wb <= 0:
        return None, "a size the device entry does not take"
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    total, stats, reason = C.c_int64(0), InflateStreamStats(), C.c_int(0)
    rc = L.dgrp_inflate_stream_scan(d_in.data_ptr(), size, data_off, PLAIN_CHUNK_BYTES, PLAIN_MAX_SPAN_BYTES, PLAIN_MAX_ROUNDS,
                                    C.byref(total), C.byref(stats), C.byref(reason), work.data_ptr(), wb, stream_ptr())
    if rc == -5:                                                     # DGRP_EDATA
        return None, "scan: " + REASONS.get(reason.value, f"reason {reason.value}")
    check(rc, "dgrp_inflate_stream_scan")
    n = int(total.value)
    if n > limit:
        raise too_large(path, n, limit)
    if n == 0:
        return None, "no text"
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    d_sym = torch.empty(n, dtype=torch.int16, device=dev)
    crc, used = C.c_uint32(0), C.c_int64(0)
    rc = L.dgrp_inflate_stream_write(d_in.data_ptr(), size, data_off, PLAIN_CHUNK_BYTES, d_sym.data_ptr(), d_out.data_ptr(), n,
                                     C.byref(crc), C.byref(used), C.byref(reason), work.data_ptr(), wb, stream_ptr())
    if rc == -5:
        return None, "write: " + REASONS.get(reason.value, f"reason {reason.value}")
    check(rc, "dgrp_inflate_stream_write")
    if used.value != size - 8:
        return None, "more than one member" if used.value < size - 8 else "truncated trailer"
    want_crc, isize = struct.unpack("<II", d_in[size - 8:].cpu().numpy().tobytes())
    if crc.value != want_crc or (n & 0xffffffff) != isize:
        return None, "CRC-32 or ISIZE mismatch"
    s = stats.as_dict()
    _LOG.info("%s: gzip but not BGZF, inflated on the device: %d spans of %d chunks (%d starts found, %d repaired, %d false), "
              "%d rounds, longest span %d bytes", path, s["spans"], s["chunks"], s["candidates"], s["repaired"], s["false_starts"],
              s["rounds"], s["longest_span"])
    return d_out, None


def open_inflated(path, limit: int, dev_fn, upload):
    """(host view, device bytes, size) of the gzip file `path`: the member walk, then the device (BGZF; one-member gzip of at least
    PLAIN_DEVICE_MIN_BYTES) or zlib (every other gzip file, and whatever the device path hands back).  Everything that can be
    refused -- corrupt headers, an inflated size above `limit` -- is refused before `dev_fn()` is called, except on the device path
    of a plain gzip file, which needs the device to learn the size."""
    import mmap
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as cm:
        members = walk_members(cm, path)
        text: Optional[bytearray] = None
        if members.kind == "bgzf":
            total = int(members.isize.sum())
            if total > limit:
                raise too_large(path, total, limit)
        else:
            why, dev = None, None
            data_off = plain_data_off(cm)
            if members.size < PLAIN_DEVICE_MIN_BYTES:
                why = f"smaller than {PLAIN_DEVICE_MIN_BYTES} bytes"
            elif data_off is None:
                why = "a member header the device path does not take"
            else:
                try:
                    dev = dev_fn()
                except Exception:                                    # (raised again below, after what zlib refuses)
                    why = "no device"
            if why is None:
                d_text, why = inflate_stream_device(path, members.size, data_off, limit, dev, upload)
                if d_text is not None:
                    return DeviceText(d_text), d_text, int(d_text.numel())
            _LOG.info("%s: gzip but not BGZF, inflated on the host with zlib (%s); `bgzip` would let the GPU inflate it", path, why)
            text = inflate_host(cm, path, limit)
            total = len(text)
    if total == 0:
        return None, None, 0
    dev = dev_fn()
    if text is None:
        d_text = inflate_device(path, members, dev, upload)
        return DeviceText(d_text), d_text, total
    import torch
    return text, torch.frombuffer(text, dtype=torch.uint8).to(dev), total


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the empty member bgzip ends a file with
BGZF_BLOCK = 0xff00                                                                     # input bytes per member, as bgzip takes them


def bgzf_member(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    """One BGZF member of `data` (at most 64 KiB) as bgzip lays it out: FLG = FEXTRA, the `BC` subfield with BSIZE, raw DEFLATE,
    CRC-32 and ISIZE."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = co.compress(data) + co.flush()
    bsize = 18 + len(body) + 8 - 1
    if len(data) > BGZF_MAX_ISIZE or bsize > 0xffff:
        raise ValueError("a BGZF member holds at most 64 KiB and compresses to at most 64 KiB")
    head = MAGIC + bytes([8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<HBBHH", 6, 66, 67, 2, bsize)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf_compress(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, block: int = BGZF_BLOCK,
                  eof: bool = True) -> bytes:
    """`data` as a BGZF file written the way bgzip writes it: members of `block` input bytes, then the EOF member."""
    out = [bgzf_member(data[o:o + block], level, strategy) for o in range(0, len(data), block)]
    return b"".join(out) + (BGZF_EOF if eof else b"")


LEVELS = (0, 1)                                                                         # dgrp_bgzf_compress_level's


def bgzf_compress_host(data, eof: bool = True, level: int = 0) -> bytes:
    """`data` as a BGZF file by the library's own encoder on the host (dgrp_bgzf_compress_host_level: members of BGZF_BLOCK input
    bytes; level 0: literals under a per-member Huffman code or a stored block; level 1: with matches inside the member, never a
    larger member than level 0's): the bytes bgzf_compress_device gives."""
    import ctypes as C

    from ._lib import check, lib
    L = lib()
    data = bytes(data)
    cap = int(L.dgrp_bgzf_bound(len(data), int(eof)))
    out = (C.c_uint8 * max(cap, 1))()
    got = C.c_int64(0)
    check(L.dgrp_bgzf_compress_host_level(data, len(data), out, cap, C.byref(got), int(eof), int(level)), "dgrp_bgzf_compress_host_level")
    return bytes(memoryview(out)[:got.value])


def bgzf_compress_device(d_text, eof: bool = True, level: int = 0):
    """The bytes of the uint8 device tensor `d_text` (contiguous, any alignment) as a BGZF file, deflated on the device
    (dgrp_bgzf_compress_level); -> uint8 device tensor.  One read-back: the size."""
    import ctypes as C

    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    if d_text.dtype != torch.uint8 or not d_text.is_contiguous():
        raise ValueError("bgzf_compress_device takes a contiguous uint8 tensor")
    if level not in LEVELS:
        raise ValueError(f"bgzf_compress_device: level {level} is not one of {LEVELS}")
    n = int(d_text.numel())
    cap = int(L.dgrp_bgzf_bound(n, int(eof)))
    d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=d_text.device)
    wb = int(L.dgrp_bgzf_workspace_bytes_level(n, int(level)))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=d_text.device)
    got = C.c_int64(0)
    check(L.dgrp_bgzf_compress_level(d_text.data_ptr() if n else None, n, d_out.data_ptr(), cap, C.byref(got), int(eof), int(level),
                                     work.data_ptr(), wb, stream_ptr()), "dgrp_bgzf_compress_level")
    return d_out[:got.value]


GZIP_PIECE = 4096 * 0xff00                          # bytes deflated per call (the level-1 workspace is five times the piece)


def bgzf_members_device(d_text, level: int, piece: int = GZIP_PIECE) -> bytes:
    """The BGZF members of the uint8 device tensor `d_text` (no EOF member; b"" for no text), deflated on the device `piece` bytes
    a call (bgzf_compress_device) and read back: members of BGZF_BLOCK text bytes, a short one at the end of every piece."""
    return b"".join(bgzf_compress_device(d_text[o:o + piece], eof=False, level=level).cpu().numpy().tobytes()
                    for o in range(0, int(d_text.numel()), piece))
