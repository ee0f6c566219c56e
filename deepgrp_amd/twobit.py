"""UCSC .2bit input (an addition; the reference reads FASTA text only).  A 2bit file is recognised by its signature, not by its name.

The format, as this module reads it (our statement of it; no UCSC tool has checked it).  Every integer is a uint32 in the writer's
byte order.

  header   signature 0x1A412743 (read as 0x4327411A: every integer of the file is byte-swapped), version (0; version 1 has 64-bit
           index offsets and is refused), sequenceCount, reserved
  index    sequenceCount entries: nameSize (uint8), name (nameSize bytes, no terminator), offset of the record from the file start
  record   dnaSize, nBlockCount, nBlockStarts[nBlockCount], nBlockSizes[nBlockCount], maskBlockCount, maskBlockStarts[],
           maskBlockSizes[], reserved, packedDna (ceil(dnaSize / 4) bytes)
  packing  T=0 C=1 A=2 G=3, the first base of a byte in its two most significant bits; the unused bits of the last byte are
           arbitrary.  Records are byte-aligned: packedDna starts at any address.
  N        bases inside an N block are N whatever their two bits say
  mask     bases inside a mask block are soft-masked (lower case)

The TEXT of a 2bit file is the FASTA `twoBitToFa` is understood to write: per record '>' + name + LF, then the bases 50 per line,
every line LF-terminated (dnaSize 0: the header line only), letters ACGT, N inside N blocks, lower case inside mask blocks.  Every
command gives for a 2bit file what it gives for that text (apart from the file-name column): the ingest below yields the records
the FASTA ingest yields from the text, and `predict --mask_dir` masks the text itself, built on the device.

open_twobit parses and validates on the host (numpy over a mapping of the file, no Python loop over blocks) and merges the blocks
into disjoint ascending intervals; the packed bases are unpacked on the GPU (dgrp_twobit_encode_batch, dgrp_twobit_text_batch).

OUTPUT (`predict --mask_dir DIR --mask_twobit`): the 2bit file of a masked text M, little-endian, version 0, both `reserved` words
0, the index directly behind the header, the records behind it in file order without padding.  Its records are the records the
reference's line loop yields from M (no header or an empty one: no record), named by the first whitespace-delimited word of the
header.  A C G T in either case pack to T=0 C=1 A=2 G=3 (the unused bits of the last byte 0); any other sequence character is N (an
N block, two bits 0); a character 'a'..'z' -- `n` and lower-case IUPAC letters included -- lies in a mask block.  Both tables hold
the maximal runs: ascending, disjoint, never adjacent, never empty.  That fixes every byte of the file.  Plain records are packed
on the device from the bytes dgrp_fasta_mask_batch has just rewritten (dgrp_twobit_pack_batch), the others by `pack_record` from
the host-masked bytes; `write_file` states the header and the index.  Round trip: the text dgrp_twobit_text_batch gives for the
output file is M with three changes -- record names are cut to their first word, sequences are re-wrapped at 50 bases per line,
and every non-ACGT letter becomes `N` or `n`.  No UCSC tool has read these files: they are checked by the tests' own reader and
writer.  `Refused`: duplicate names, a name above 255 bytes, a record above 2^32 - 1 bases, a file that reaches 2^32 bytes, a
record whose sequence lines are not ASCII -- no file is written for that input."""
from __future__ import annotations

import mmap
import os
import struct
from typing import List

import numpy as np

SIGNATURE = 0x1A412743
_MAGIC = {struct.pack("<I", SIGNATURE): "<", struct.pack(">I", SIGNATURE): ">"}
LINE = 50                                                  # bases per line of the text


def is_twobit(path) -> bool:
    """The file starts with the 2bit signature in either byte order (False for anything that cannot be opened)."""
    try:
        with open(path, "rb") as fh:
            return fh.read(4) in _MAGIC
    except OSError:
        return False


def twobit_inputs(files):
    """The command-line inputs that are 2bit files (stdin and the one-hot .npz are never)."""
    return [f for f in files if f != "-" and not f.endswith(".npz") and os.path.isfile(f) and is_twobit(f)]


def too_large(path, limit: int) -> ValueError:
    return ValueError(f"{path}: more than {limit} bytes (DGRP_FASTA_RESIDENT_BYTES); a 2bit file is read whole into device memory, "
                      "so convert this file to FASTA and give that instead")


def _merge(start: np.ndarray, size: np.ndarray) -> np.ndarray:
    """Blocks ascending by start -> disjoint ascending [start, end) intervals (int64 [k, 2]): zero-length blocks dropped, adjacent
    and overlapping ones merged."""
    keep = size > 0
    s, e = start[keep], (start + size)[keep]
    if s.size == 0:
        return np.zeros((0, 2), np.int64)
    reach = np.maximum.accumulate(e)                                    # furthest end up to and including block i
    first = np.flatnonzero(np.concatenate(([True], s[1:] > reach[:-1])))   # blocks that open an interval
    last = np.concatenate((first[1:] - 1, [s.size - 1]))
    return np.stack((s[first], reach[last]), axis=1)


class TwoBit:
    """A parsed 2bit file.  Per record r: `names[r]` (bytes), `name_off[r]` (file offset of the name), `rec_off[r]` (of the record),
    `dna_size[r]`, `packed_off[r]` (file offset of packedDna), its merged N intervals `n_iv[n_off[r]:n_off[r + 1]]` and soft-mask
    intervals `m_iv[m_off[r]:m_off[r + 1]]` ([start, end), int64), `startpos[r]` (leading N) and `kept[r]` (bases from the first to
    the last that is not N; minus dnaSize for a record of N only, as dgrp_fasta_encode_batch reports it), `text_off` (nrec + 1
    offsets of the records in the text of the file).  All offsets int64."""

    __slots__ = ("path", "size", "byteorder", "names", "name_off", "name_len", "rec_off", "dna_size", "packed_off", "n_iv", "n_off",
                 "m_iv", "m_off", "startpos", "kept", "text_off")

    @property
    def nrec(self) -> int:
        return len(self.names)

    @property
    def text_size(self) -> int:
        return int(self.text_off[-1])

    def plain_names(self) -> bool:
        """Every header line of the text is one ASCII line (what the FASTA ingest's device path asks of a header line)."""
        return all(nm.isascii() and b"\n" not in nm and b"\r" not in nm for nm in self.names)

    def header(self, r: int) -> str:
        """The header the FASTA ingest reads from the record's header line of the text (plain_names() only)."""
        return (b">" + self.names[r]).decode("ascii").strip()[1:]


def open_twobit(path) -> TwoBit:
    """Parse and validate the 2bit file `path` on the host.  ValueError naming the file, the record and the field for a version
    other than 0, an index, table or packedDna that runs past the end of the file, blocks that are not ascending by start and a
    block that reaches past dnaSize."""
    size = os.path.getsize(path)
    tb = TwoBit()
    tb.path, tb.size = path, size
    if not is_twobit(path):
        raise ValueError(f"{path}: not a 2bit file (no signature 0x{SIGNATURE:08X})")
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        order = _MAGIC[mm[:4]]
        if size < 16:
            raise ValueError(f"{path}: truncated: the header (signature, version, sequenceCount, reserved) runs past the end of the file")
        dt = np.dtype(order + "u4")
        u32 = struct.Struct(order + "I")
        version, count, _reserved = struct.unpack_from(order + "III", mm, 4)
        if version != 0:
            raise ValueError(f"{path}: 2bit version {version} is not supported (version 0 only; version 1 has 64-bit index offsets)")
        tb.byteorder = order
        names: List[bytes] = []
        name_off, rec_off = np.zeros(count, np.int64), np.zeros(count, np.int64)
        pos = 16
        for i in range(count):
            if pos + 1 > size or pos + 1 + mm[pos] + 4 > size:
                raise ValueError(f"{path}: truncated: index entry {i} of {count} (nameSize, name, offset) runs past the end of the file")
            ns = mm[pos]
            names.append(mm[pos + 1:pos + 1 + ns])
            name_off[i] = pos + 1
            rec_off[i] = u32.unpack_from(mm, pos + 1 + ns)[0]
            pos += 1 + ns + 4
        dna, packed = np.zeros(count, np.int64), np.zeros(count, np.int64)
        n_parts, m_parts = [], []
        n_off, m_off = np.zeros(count + 1, np.int64), np.zeros(count + 1, np.int64)

        def word(p: int, who: str, field: str) -> int:
            if p + 4 > size:
                raise ValueError(f"{path}: truncated: {who}: {field} runs past the end of the file")
            return u32.unpack_from(mm, p)[0]

        def blocks(p: int, who: str, kind: str, n: int):
            """The block table at p -> (merged intervals, position behind it)."""
            cnt = word(p, who, f"{kind}BlockCount")
            p += 4
            if p + 8 * cnt > size:
                field = f"{kind}BlockStarts" if p + 4 * cnt > size else f"{kind}BlockSizes"
                raise ValueError(f"{path}: truncated: {who}: {field} ({cnt} blocks) runs past the end of the file")
            start = np.frombuffer(mm, dtype=dt, count=cnt, offset=p).astype(np.int64)
            length = np.frombuffer(mm, dtype=dt, count=cnt, offset=p + 4 * cnt).astype(np.int64)
            if cnt > 1:
                bad = np.flatnonzero(start[1:] < start[:-1])
                if bad.size:
                    k = int(bad[0]) + 1
                    raise ValueError(f"{path}: {who}: {kind}BlockStarts are not ascending: block {k} starts at {int(start[k])}, "
                                     f"block {k - 1} at {int(start[k - 1])}")
            bad = np.flatnonzero(start + length > n)
            if bad.size:
                k = int(bad[0])
                raise ValueError(f"{path}: {who}: {kind}Block {k} [{int(start[k])}, {int(start[k] + length[k])}) reaches past dnaSize {n}")
            return _merge(start, length), p + 8 * cnt

        for r in range(count):
            who = f"record {r} ({names[r]!r})"
            p = int(rec_off[r])
            n = word(p, who, "dnaSize")
            n_iv, p = blocks(p + 4, who, "n", n)
            m_iv, p = blocks(p, who, "mask", n)
            word(p, who, "reserved")
            p += 4
            if p + (n + 3) // 4 > size:
                raise ValueError(f"{path}: truncated: {who}: packedDna ({(n + 3) // 4} bytes at offset {p}) runs past the end of the file")
            dna[r], packed[r] = n, p
            n_parts.append(n_iv)
            m_parts.append(m_iv)
            n_off[r + 1] = n_off[r] + len(n_iv)
            m_off[r + 1] = m_off[r] + len(m_iv)
    tb.names, tb.name_off, tb.rec_off, tb.dna_size, tb.packed_off = names, name_off, rec_off, dna, packed
    tb.name_len = np.array([len(nm) for nm in names], np.int64)
    empty = np.zeros((0, 2), np.int64)
    tb.n_iv = np.ascontiguousarray(np.concatenate(n_parts)) if n_parts else empty
    tb.m_iv = np.ascontiguousarray(np.concatenate(m_parts)) if m_parts else empty
    tb.n_off, tb.m_off = n_off, m_off
    # leading / trailing N from the merged intervals: the first one when it starts at 0, the last one when it ends at dnaSize
    has = n_off[1:] > n_off[:-1]
    first = tb.n_iv[np.minimum(n_off[:-1], max(len(tb.n_iv) - 1, 0))] if len(tb.n_iv) else np.zeros((count, 2), np.int64)
    last = tb.n_iv[np.maximum(n_off[1:] - 1, 0)] if len(tb.n_iv) else np.zeros((count, 2), np.int64)
    lead = np.where(has & (first[:, 0] == 0), first[:, 1], 0)
    end = np.where(has & (last[:, 1] == dna), last[:, 0], dna)
    tb.startpos = lead.astype(np.int64)
    tb.kept = np.where(end > lead, end - lead, np.where(dna > 0, -dna, 0)).astype(np.int64)
    tb.text_off = np.zeros(count + 1, np.int64)
    np.cumsum(2 + tb.name_len + dna + (dna + LINE - 1) // LINE, out=tb.text_off[1:])
    return tb


def placed_offsets(packed_addr: np.ndarray, dna: np.ndarray, idx_addr: int) -> np.ndarray:
    """Offsets into an index buffer at address `idx_addr` at which dgrp_twobit_encode_batch has both its 4-byte packed loads and
    its 16-byte index stores aligned, for records whose packed bytes lie at `packed_addr` and hold `dna` bases; the buffer takes
    dna.sum() + 32 * nrec + 16 bytes.  Word g of a record whose first index lies `o` bytes into a 16-byte word starts with base
    16 g - o, which is packed byte 4 g - o / 4: that address is a multiple of 4 when o = 4 * (packed_addr mod 4)."""
    phase = (4 * (packed_addr & 3) - idx_addr) & 15                        # idx_addr + out_off = 4 * (packed_addr mod 4) (mod 16)
    slot = (dna + 15 + 16) & ~np.int64(15)                                 # room for any phase
    return np.ascontiguousarray(np.cumsum(slot) - slot + phase, dtype=np.int64)


def _device_intervals(iv: np.ndarray, dev):
    import torch
    return torch.from_numpy(iv).to(dev) if len(iv) else None


def _ptr(t):
    return t.data_ptr() if t is not None else None


class DeviceTwoBit:
    """A parsed 2bit file whose bytes and N intervals are in HBM."""

    def __init__(self, tb: TwoBit, dev, upload):
        self.tb, self.dev = tb, dev
        self.d_file = upload(tb.path, tb.size, dev)
        self.d_n_iv = _device_intervals(tb.n_iv, dev)

    def encode(self, r0: int, r1: int):
        """Class indices of the records [r0, r1) in one dgrp_twobit_encode_batch -> (uint8 device buffer, offset of every record's
        first base in it).  Every record is placed so that its 4-byte packed loads and 16-byte index stores are both aligned."""
        import torch

        from ._lib import check, lib
        from .pipeline import stream_ptr
        L = lib()
        tb, nrec = self.tb, r1 - r0
        dna = np.ascontiguousarray(tb.dna_size[r0:r1])
        packed = np.ascontiguousarray(tb.packed_off[r0:r1])
        d_idx = torch.empty(int(dna.sum()) + 32 * nrec + 16, dtype=torch.uint8, device=self.dev)
        out_off = placed_offsets(self.d_file.data_ptr() + packed, dna, d_idx.data_ptr())
        n_off = np.ascontiguousarray(tb.n_off[r0:r1 + 1])
        wb = int(L.dgrp_twobit_workspace_bytes(nrec))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.dev)
        check(L.dgrp_twobit_encode_batch(self.d_file.data_ptr(), tb.size, nrec, packed.ctypes.data, dna.ctypes.data, _ptr(self.d_n_iv),
                                         n_off.ctypes.data, len(tb.n_iv), out_off.ctypes.data, d_idx.data_ptr(), int(d_idx.numel()),
                                         work.data_ptr(), wb, stream_ptr()), f"dgrp_twobit_encode_batch ({tb.path})")
        return d_idx, out_off

    def text(self):
        """The text of the file as one uint8 device tensor (dgrp_twobit_text_batch over every record)."""
        import torch

        from ._lib import check, lib
        from .pipeline import stream_ptr
        L = lib()
        tb = self.tb
        d_text = torch.empty(tb.text_size, dtype=torch.uint8, device=self.dev)
        if tb.nrec == 0:
            return d_text
        d_m_iv = _device_intervals(tb.m_iv, self.dev)
        wb = int(L.dgrp_twobit_workspace_bytes(tb.nrec))
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.dev)
        check(L.dgrp_twobit_text_batch(self.d_file.data_ptr(), tb.size, tb.nrec, tb.name_off.ctypes.data, tb.name_len.ctypes.data,
                                       tb.packed_off.ctypes.data, tb.dna_size.ctypes.data, _ptr(self.d_n_iv), tb.n_off.ctypes.data,
                                       len(tb.n_iv), _ptr(d_m_iv), tb.m_off.ctypes.data, len(tb.m_iv), tb.text_off.ctypes.data,
                                       d_text.data_ptr(), tb.text_size, work.data_ptr(), wb, stream_ptr()),
              f"dgrp_twobit_text_batch ({tb.path})")
        return d_text


def open_text(path, limit: int, dev_fn, upload):
    """(host view, device bytes, size) of the text of the 2bit file `path`, as gz.open_inflated gives them for a compressed FASTA
    file.  Everything that can be refused -- a file that does not parse, a file or text above `limit` -- is refused before
    `dev_fn()` is called."""
    from .gz import DeviceText
    tb = open_twobit(path)
    if tb.size > limit or tb.text_size > limit:
        raise too_large(path, limit)
    if tb.text_size == 0:
        return None, None, 0
    d_text = DeviceTwoBit(tb, dev_fn(), upload).text()
    return DeviceText(d_text), d_text, tb.text_size


# ---- output: the 2bit file of a masked text

class Refused(ValueError):
    """The input has no 2bit file (the message names the file and the record); nothing is written for it."""


_ENOMEM = -3                                               # DGRP_ENOMEM (include/deepgrp_hip.h)
_CODE = np.full(256, 4, np.uint8)                          # T=0 C=1 A=2 G=3 in either case, 4 = N
for _i, _c in enumerate(b"TCAG"):
    _CODE[_c] = _CODE[_c | 0x20] = _i


def _runs(inside: np.ndarray):
    """(starts, sizes) of the maximal runs of True."""
    edge = np.diff(np.concatenate(([0], inside.view(np.int8), [0])))
    start = np.flatnonzero(edge == 1)
    return start, np.flatnonzero(edge == -1) - start


def pack_record(seq) -> bytes:
    """The record blob (dnaSize, the N block table, the mask block table, reserved, packedDna) of the sequence characters `seq`
    (bytes or uint8 array, no line ends), by the rules of the module docstring -- what dgrp_twobit_pack_batch writes for a plain
    record."""
    b = np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)
    if b.size > 0xFFFFFFFF:
        raise Refused(f"{b.size} bases, a 2bit record holds at most 2^32 - 1")
    code = _CODE[b]
    isn = code == 4
    ns, nz = _runs(isn)
    ms, mz = _runs((b >= 97) & (b <= 122))
    two = np.where(isn, 0, code).astype(np.uint8)
    two = np.concatenate((two, np.zeros((-b.size) % 4, np.uint8))).reshape(-1, 4)
    packed = (two[:, 0] << 6) | (two[:, 1] << 4) | (two[:, 2] << 2) | two[:, 3]
    u = lambda a: np.asarray(a, "<u4").tobytes()
    return b"".join((u([b.size, ns.size]), u(ns), u(nz), u([ms.size]), u(ms), u(mz), u([0]), packed.astype(np.uint8).tobytes()))


def record_name(header: str, encoding: str = "ascii") -> bytes:
    """faToTwoBit's rule: the first whitespace-delimited word of the (stripped) header."""
    words = header.split()
    return words[0].encode(encoding, "surrogateescape") if words else b""


def write_file(names, blobs, out, sizes=None, what=None) -> int:
    """Write the 2bit file of the records `names` (bytes) to the path `out`: header (signature, version 0, count, reserved 0),
    index (nameSize, name, offset of the record), then the record blobs back to back.  `blobs`: one bytes-like per record; with
    `sizes` (bytes per record) any iterable of pieces whose concatenation is the blobs in order (a spool).  Refused, before
    anything is written, with `what` (default `out`) and the record in the message: two records of one name, a name above 255
    bytes, a file that reaches 2^32 bytes.  Returns the file's size."""
    what = str(out) if what is None else what
    names = [bytes(n) for n in names]
    if sizes is None:
        blobs = [memoryview(b).cast("B") for b in blobs]
        sizes = [len(b) for b in blobs]
    if len(sizes) != len(names):
        raise ValueError(f"{what}: {len(names)} names, {len(sizes)} records")
    seen = {}
    for r, nm in enumerate(names):
        if len(nm) > 255:
            raise Refused(f"{what}: record {r} ({nm[:40]!r}...): its name has {len(nm)} bytes, a 2bit index entry holds at most 255")
        if nm in seen:
            raise Refused(f"{what}: records {seen[nm]} and {r} are both named {nm!r} (the first word of their headers); a 2bit file "
                          "names every record once")
        seen[nm] = r
    pos = 16 + sum(5 + len(nm) for nm in names)
    index = []
    for r, (nm, z) in enumerate(zip(names, sizes)):
        if pos + z >= 1 << 32:
            raise Refused(f"{what}: record {r} ({nm!r}): the file reaches 2^32 bytes, beyond the 32-bit offsets of 2bit version 0")
        index.append(bytes([len(nm)]) + nm + struct.pack("<I", pos))
        pos += z
    total = 0
    with open(out, "wb") as fh:
        fh.write(struct.pack("<IIII", SIGNATURE, 0, len(names), 0))
        fh.write(b"".join(index))
        for piece in blobs:
            total += fh.write(piece)
    if total != sum(sizes):
        raise ValueError(f"{what}: {total} bytes of records, the index states {sum(sizes)}")
    return pos


def pack_device(raw_ptr: int, h_off: np.ndarray, h_len: np.ndarray, dev, what: str):
    """dgrp_twobit_pack_batch over the plain record bodies [h_off[r], + h_len[r]) of the 16-byte aligned device buffer at
    `raw_ptr` -> (uint8 device buffer, counts int64 [nrec, 3] = dnaSize, nBlockCount, maskBlockCount, blob offsets int64
    [nrec + 1]): record r's blob is buffer[blob_off[r]:blob_off[r + 1]].  The buffer is sized for few blocks; where the counts ask
    for more the call is repeated once at the size it names."""
    import torch

    from ._lib import check, lib
    from .pipeline import stream_ptr
    L = lib()
    nrec, total = len(h_off), int(h_len.sum())
    counts, blob_off = np.zeros((nrec, 3), np.int64), np.zeros(nrec + 1, np.int64)
    wb = int(L.dgrp_twobit_pack_workspace_bytes(nrec, total))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    cap = 17 * nrec + total // 4 + total // 16 + 4096
    for attempt in (0, 1):
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        rc = L.dgrp_twobit_pack_batch(raw_ptr, nrec, h_off.ctypes.data, h_len.ctypes.data, d_out.data_ptr(), 0, cap, counts.ctypes.data,
                                      blob_off.ctypes.data, work.data_ptr(), wb, stream_ptr())
        if rc == _ENOMEM and attempt == 0 and int(blob_off[-1]) > cap:    # many blocks; the sizes are known now
            cap = int(blob_off[-1])
            continue
        check(rc, what)
        break
    return d_out, counts, blob_off
