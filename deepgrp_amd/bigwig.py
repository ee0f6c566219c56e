"""The bigWig file (`.bw`) of a probability track (`predict --track_dir --track_bigwig`), stated in numpy/Python.

What the file says is what the bedGraph of the same flags says (tracks.reference_text): `reference_items` gives the items of one class
column -- (start, end, q) of every line -- and an item's value is float32(q / 10^digits), the float32 a reader gets from the line's
decimal text.  The device writes the uncompressed sections and zoom records and deflates them (dgrp_track_sections_batch,
dgrp_track_zoom_batch, dgrp_zlib_compress_batch); `BigWigBuilder` puts the container around them as the writes come in.

The layout.  All fields are little-endian and every part is found through an absolute file offset, so data is appended per write and
the header is rewritten at commit.
  1. Header, 64 bytes: magic u32 0x888FFC26, version u16 4, zoomLevels u16, chromosomeTreeOffset u64, fullDataOffset u64,
     fullIndexOffset u64, fieldCount u16 0, definedFieldCount u16 0, autoSqlOffset u64 0, totalSummaryOffset u64, uncompressBufSize
     u32 (the largest uncompressed block of the file, sections and zoom blocks alike), reserved u64 0.
  2. Zoom headers, room for 10, zoomLevels of them valid, 24 bytes each: reductionLevel u32, reserved u32, dataOffset u64,
     indexOffset u64.
  3. Total summary, 40 bytes: basesCovered u64, then minVal, maxVal, sumData, sumSquares as doubles, over the bases with q != 0 (all
     0 with nothing covered).
  4. Data at fullDataOffset: sectionCount u64, then the sections in the order they are produced (file order of the records,
     ascending start inside a record).  A section is up to 1024 items of ONE record; uncompressed: chromId u32, chromStart u32 (its
     first item's start), chromEnd u32 (its last item's end), itemStep u32 0, itemSpan u32 0, type u8 1 (bedGraph), reserved u8,
     itemCount u16, then the items (start u32, end u32, value f32).  Stored as one zlib stream: 78 01, one DEFLATE block, Adler-32.
  5. Data index at fullIndexOffset, a cirTree.  Header, 48 bytes: magic u32 0x2468ACE0, blockSize u32 256, itemCount u64,
     startChromIx, startBase, endChromIx, endBase (u32 each), endFileOffset u64, itemsPerSlot u32 1, reserved u32.  Node: isLeaf u8,
     reserved u8, count u16, then its items.  Leaf item, 32 bytes: startChromIx, startBase, endChromIx, endBase, dataOffset u64,
     dataSize u64.  Inner item, 24 bytes: the four bounds, childOffset u64.  One leaf item per section, 256 per node, bottom-up;
     the levels lie root first.  Without sections: itemCount 0 and one empty leaf.
  6. Zoom levels, each: recordCount u32 at dataOffset, the zoom blocks, a cirTree of the blocks at indexOffset.  A block is up to
     1024 records of ONE write as one zlib stream; a record is 32 bytes: chromId, chromStart, chromEnd, validCount (u32), minVal,
     maxVal, sumData, sumSquares (f32).
  7. Chromosome B+ tree.  Header, 32 bytes: magic u32 0x78CA8C91, blockSize u32 min(256, max(1, count)), keySize u32 (the longest
     name, at least 1), valSize u32 8, itemCount u64, reserved u64.  Node: isLeaf u8, reserved u8, count u16, then room for blockSize
     items.  Leaf item: the key, zero-padded to keySize, chromId u32, chromSize u32.  Inner item: key, childOffset u64.  Keys in
     ascending byte order.  It holds every record that reached the writer, records without items included; chromId is the record's
     ordinal in the input, so file order is (chromId, start) order; chromSize is startpos + n, the end of the predicted span (the
     pipeline does not keep the count of trailing N).
  8. Trailer: magic u32 0x888FFC26.

Zoom ladder.  R_k = 16 * bin * 4^k, k = 0..9; level k is written when R_k is smaller than the largest chromSize of the input and the
level holds a record, else neither it nor the levels above.  Window w of level k of a record is [w * R_k, (w + 1) * R_k); a window
with a covered base gives one record (dgrp_track_zoom_batch in include/deepgrp_hip.h states its fields).

A bigWig cannot hold a record with an empty name, two records of one name, or a record that ends above 2^32 - 1 (`Refused`).

No program of the UCSC tree has read these files: the format above is checked by a reader written for the tests alone."""
from __future__ import annotations

import os
import struct
import tempfile
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAGIC = 0x888FFC26
CIR_MAGIC = 0x2468ACE0
BPT_MAGIC = 0x78CA8C91
MAX_END = (1 << 32) - 1
SECTION_ITEMS = 1024
ZOOM_LEVELS = 10
BLOCK = 0xff00                                      # the largest block of a zlib stream (gz.BGZF_BLOCK)
DATA_OFFSET = 64 + 24 * ZOOM_LEVELS + 40            # header, zoom headers, total summary

SECTION_DTYPE = np.dtype([("off", "<i8"), ("bytes", "<i8"), ("rec", "<i4"), ("start", "<u4"), ("end", "<u4"), ("pad", "<u4")])
ZOOM_BLOCK_DTYPE = np.dtype([("off", "<i8"), ("bytes", "<i8"), ("cls", "<i4"), ("level", "<i4"), ("rec0", "<i4"), ("rec1", "<i4"),
                             ("start", "<u4"), ("end", "<u4")])
TOTALS_DTYPE = np.dtype([("covered", "<u8"), ("qmin", "<u8"), ("qmax", "<u8"), ("sum", "<u8"), ("sumsq", "<u8")])
LEAF_DTYPE = np.dtype([("sc", "<u4"), ("sb", "<u4"), ("ec", "<u4"), ("eb", "<u4"), ("off", "<u8"), ("size", "<u8")])
_INNER_DTYPE = np.dtype([("sc", "<u4"), ("sb", "<u4"), ("ec", "<u4"), ("eb", "<u4"), ("off", "<u8")])


class Refused(ValueError):
    """The input has no bigWig: an empty name, a name that two records share, a record that ends above 2^32 - 1."""


def reduction(level: int, bin: int) -> int:
    return 16 * bin * 4 ** level


def reference_items(column: np.ndarray, startpos: int, digits: int = 2, bin: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The items of one class column (float32 [n]) of one record by tracks.reference_text's rules: -> (start, end, q), int64 each."""
    from .tracks import quantise
    v = np.asarray(column, np.float32)
    n = v.size
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    pos = np.arange(startpos, startpos + n, dtype=np.int64)
    cut = np.flatnonzero(np.diff(pos // bin)) + 1
    first = np.r_[0, cut]
    q = quantise(np.maximum(np.maximum.reduceat(v, first), np.float32(0)), digits)
    lo = pos[first]
    hi = np.r_[pos[cut], startpos + n]
    rs = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    re = np.r_[rs[1:], q.size]
    keep = q[rs] != 0
    return lo[rs[keep]], hi[re[keep] - 1], q[rs[keep]]


def item_values(q: np.ndarray, digits: int) -> np.ndarray:
    """float32(q / 10^digits): the value of an item."""
    return (np.asarray(q, np.float64) / np.float64(10 ** digits)).astype(np.float32)


def section_bytes(chrom: int, start: np.ndarray, end: np.ndarray, q: np.ndarray, digits: int) -> List[bytes]:
    """The uncompressed sections of one record's items."""
    out = []
    val = item_values(q, digits)
    for a in range(0, len(start), SECTION_ITEMS):
        b = min(a + SECTION_ITEMS, len(start))
        items = np.zeros(b - a, np.dtype([("s", "<u4"), ("e", "<u4"), ("v", "<f4")]))
        items["s"], items["e"], items["v"] = start[a:b], end[a:b], val[a:b]
        out.append(struct.pack("<IIIIIBBH", chrom, int(start[a]), int(end[b - 1]), 0, 0, 1, 0, b - a) + items.tobytes())
    return out


def chrom_tree(names: Sequence[bytes], ids: Sequence[int], sizes: Sequence[int], at: int) -> bytes:
    """The chromosome B+ tree as it lies at file offset `at`."""
    n = len(names)
    bs = min(256, max(1, n))
    ks = max([1] + [len(x) for x in names])
    head = struct.pack("<IIIIQQ", BPT_MAGIC, bs, ks, 8, n, 0)
    item = np.dtype([("key", f"S{ks}"), ("val", "<u8")])
    node_size = 4 + bs * item.itemsize
    if n == 0:
        return head + struct.pack("<BBH", 1, 0, 0) + bytes(node_size - 4)
    keys = np.array(list(names), dtype=f"S{ks}")
    order = np.argsort(keys, kind="stable")
    level = np.zeros(n, item)
    level["key"] = keys[order]
    level["val"] = np.asarray(ids, np.uint64)[order] | (np.asarray(sizes, np.uint64)[order] << np.uint64(32))
    levels = [level]                                                # leaves first
    while (len(levels[-1]) + bs - 1) // bs > 1:
        below = levels[-1]
        up = np.zeros((len(below) + bs - 1) // bs, item)
        up["key"] = below["key"][::bs]
        levels.append(up)
    nodes = [(len(lv) + bs - 1) // bs for lv in levels]
    start, pos = [0] * len(levels), at + 32                         # where each level's nodes lie: root level first
    for k in range(len(levels) - 1, -1, -1):
        start[k] = pos
        pos += nodes[k] * node_size
    out = [head]
    for k in range(len(levels) - 1, -1, -1):
        lv = levels[k]
        if k > 0:
            lv["val"] = start[k - 1] + np.arange(len(lv), dtype=np.uint64) * np.uint64(node_size)
        buf = np.zeros((nodes[k], node_size), np.uint8)
        buf[:, 0] = k == 0
        count = np.full(nodes[k], bs, "<u2")
        count[-1] = len(lv) - bs * (nodes[k] - 1)
        buf[:, 2:4] = count.view(np.uint8).reshape(-1, 2)
        padded = np.zeros(nodes[k] * bs, item)
        padded[:len(lv)] = lv
        buf[:, 4:] = padded.view(np.uint8).reshape(nodes[k], -1)
        out.append(buf.tobytes())
    return b"".join(out)


def cir_tree(leaves: np.ndarray, at: int, end_offset: int, items_per_slot: int = 1) -> bytes:
    """The cirTree over `leaves` (LEAF_DTYPE, in (chrom, start) order) as it lies at file offset `at`; items_per_slot is the
    header's field (1 in a bigWig; bigbed.py: the items of a full block)."""
    n = len(leaves)
    bs = 256
    if n == 0:
        return struct.pack("<IIQIIIIQII", CIR_MAGIC, bs, 0, 0, 0, 0, 0, end_offset, items_per_slot, 0) + struct.pack("<BBH", 1, 0, 0)
    ends = (leaves["ec"].astype(np.uint64) << np.uint64(32)) | leaves["eb"].astype(np.uint64)
    top = int(ends.max())
    head = struct.pack("<IIQIIIIQII", CIR_MAGIC, bs, n, int(leaves["sc"][0]), int(leaves["sb"][0]), top >> 32, top & 0xffffffff,
                       end_offset, items_per_slot, 0)
    levels = [(leaves, ends)]
    while len(levels[-1][0]) > bs:
        below, bends = levels[-1]
        first = np.arange(0, len(below), bs)
        up = np.zeros(len(first), _INNER_DTYPE)
        up["sc"], up["sb"] = below["sc"][first], below["sb"][first]
        uends = np.maximum.reduceat(bends, first)
        up["ec"], up["eb"] = (uends >> np.uint64(32)).astype(np.uint32), (uends & np.uint64(0xffffffff)).astype(np.uint32)
        levels.append((up, uends))
    sizes = []                                                      # per level: the byte size of every node
    for lv, _e in levels:
        nn = (len(lv) + bs - 1) // bs
        count = np.full(nn, bs, np.int64)
        count[-1] = len(lv) - bs * (nn - 1)
        sizes.append(4 + count * lv.dtype.itemsize)
    start, pos = [0] * len(levels), at + 48
    for k in range(len(levels) - 1, -1, -1):
        start[k] = pos
        pos += int(sizes[k].sum())
    out = [head]
    for k in range(len(levels) - 1, -1, -1):
        lv = levels[k][0]
        if k > 0:
            lv["off"] = start[k - 1] + np.r_[0, np.cumsum(sizes[k - 1])[:-1]].astype(np.uint64)
        raw = lv.tobytes()
        step = bs * lv.dtype.itemsize
        for j in range(len(sizes[k])):
            part = raw[j * step:(j + 1) * step]
            out.append(struct.pack("<BBH", k == 0, 0, len(part) // lv.dtype.itemsize) + part)
    return b"".join(out)


def zlib_compress_host(data: bytes, offsets: Sequence[int], lengths: Sequence[int], level: int = 1) -> Tuple[bytes, np.ndarray]:
    """The blocks data[offsets[m] : offsets[m] + lengths[m]] as zlib streams back to back, by the library's encoder on the host
    (dgrp_zlib_compress_host: the bytes the device entry gives); -> (streams, their sizes)."""
    import ctypes as C

    from ._lib import check, lib
    L = lib()
    data = bytes(data)
    rows = np.zeros((len(offsets), 2), np.int64)
    rows[:, 0], rows[:, 1] = offsets, lengths
    cap = int(L.dgrp_zlib_bound(len(rows), len(data)))
    out = (C.c_uint8 * max(cap, 1))()
    sizes = np.zeros(max(len(rows), 1), np.int64)
    got = C.c_int64(0)
    check(L.dgrp_zlib_compress_host(data, len(data), rows.ctypes.data, 16, len(rows), int(level), out, cap, sizes.ctypes.data, C.byref(got)),
          "dgrp_zlib_compress_host")
    return bytes(memoryview(out)[:got.value]), sizes[:len(rows)]


class ClassWrite(NamedTuple):
    """One class's part of one write: the compressed sections back to back with the size of each and their table rows
    (SECTION_DTYPE; rec counts inside the write, while the chromId inside a section is the record's ordinal in the input), the same for its zoom blocks (ZOOM_BLOCK_DTYPE), and its integer totals
    (covered, qmin, qmax, sum of q * bases, sum of q^2 * bases)."""
    sections: bytes
    section_sizes: np.ndarray
    section_table: np.ndarray
    zoom: bytes
    zoom_sizes: np.ndarray
    zoom_table: np.ndarray
    totals: Tuple[int, int, int, int, int]


class BigWigBuilder:
    """One `.bw` file on the open binary file `fh` (empty, seekable): `add` appends a write's sections and spools its zoom blocks to a
    temporary file beside it, `finish` writes indexes, zoom levels, chromosome tree and trailer and rewrites the header.  The class
    attributes are what bigbed.BigBedBuilder states differently: the magic, fieldCount and definedFieldCount, the autoSql text behind
    the zoom headers (none: autoSqlOffset 0) and the itemsPerSlot of the data index."""
    magic = MAGIC
    fields = (0, 0)
    autosql = b""
    items_per_slot = 1

    def __init__(self, fh, digits: int, bin: int, spool_dir: Optional[str] = None):
        self.fh, self.digits, self.bin = fh, digits, bin
        self.names: List[bytes] = []
        self.sizes: List[int] = []
        self.leaves: List[np.ndarray] = []
        self.zoom: List[List[np.ndarray]] = [[] for _ in range(ZOOM_LEVELS)]     # per level: LEAF_DTYPE rows with spool offsets
        self.zoom_records = [0] * ZOOM_LEVELS
        self.zoom_buf = [0] * ZOOM_LEVELS                                       # per level: its largest uncompressed block
        self.spool = tempfile.TemporaryFile(dir=spool_dir)
        self.spooled = 0
        self.nsections = 0
        self.buf_size = 0
        self.covered = self.sum = self.sumsq = self.qmax = 0
        self.qmin: Optional[int] = None
        self.summary_at = 64 + 24 * ZOOM_LEVELS + len(self.autosql)
        self.data_at = self.summary_at + 40
        fh.write(bytes(self.data_at + 8))
        self.at = self.data_at + 8

    def add(self, names: Sequence[bytes], sizes: Sequence[int], w: Optional[ClassWrite]) -> None:
        first = len(self.names)
        self.names.extend(names)
        self.sizes.extend(int(s) for s in sizes)
        if w is None:
            return
        t = w.section_table
        if len(t):
            leaf = np.zeros(len(t), LEAF_DTYPE)
            leaf["sc"] = leaf["ec"] = t["rec"].astype(np.int64) + first
            leaf["sb"], leaf["eb"] = t["start"], t["end"]
            leaf["size"] = w.section_sizes
            leaf["off"] = self.at + np.r_[0, np.cumsum(w.section_sizes)[:-1]]
            self.leaves.append(leaf)
            self.fh.write(w.sections)
            self.at += len(w.sections)
            self.nsections += self.counted(t)
            self.buf_size = max(self.buf_size, int(t["bytes"].max()))
        z = w.zoom_table
        if len(z):
            off = self.spooled + np.r_[0, np.cumsum(w.zoom_sizes)[:-1]]
            for k in range(ZOOM_LEVELS):
                sel = np.flatnonzero(z["level"] == k)
                if sel.size == 0:
                    continue
                leaf = np.zeros(sel.size, LEAF_DTYPE)
                leaf["sc"], leaf["ec"] = z["rec0"][sel].astype(np.int64) + first, z["rec1"][sel].astype(np.int64) + first
                leaf["sb"], leaf["eb"] = z["start"][sel], z["end"][sel]
                leaf["off"], leaf["size"] = off[sel], w.zoom_sizes[sel]
                self.zoom[k].append(leaf)
                self.zoom_records[k] += int(z["bytes"][sel].sum()) // 32
                self.zoom_buf[k] = max(self.zoom_buf[k], int(z["bytes"][sel].max()))
            self.spool.write(w.zoom)
            self.spooled += len(w.zoom)
        covered, qmin, qmax, s1, s2 = (int(x) for x in w.totals)
        if covered:
            self.covered += covered
            self.sum += s1
            self.sumsq += s2
            self.qmin = qmin if self.qmin is None else min(self.qmin, qmin)
            self.qmax = max(self.qmax, qmax)

    @staticmethod
    def counted(table: np.ndarray) -> int:
        """What a write's table adds to the count at fullDataOffset: its sections."""
        return len(table)

    def levels(self) -> int:
        """The zoom levels the file gets."""
        longest = max(self.sizes, default=0)
        k = 0
        while k < ZOOM_LEVELS and reduction(k, self.bin) < longest and self.zoom_records[k] > 0:
            k += 1
        return k

    def finish(self) -> None:
        fh = self.fh
        leaves = np.concatenate(self.leaves) if self.leaves else np.zeros(0, LEAF_DTYPE)
        index_at = self.at
        fh.write(cir_tree(leaves, index_at, index_at, self.items_per_slot))
        nlev = self.levels()
        zoom_heads = []
        for k in range(nlev):
            data_at = fh.tell()
            fh.write(struct.pack("<I", self.zoom_records[k]))
            rows = np.concatenate(self.zoom[k])
            pos = data_at + 4
            for row in rows:                                        # (a level's blocks lie apart in the spool: one write in between each)
                self.spool.seek(int(row["off"]))
                fh.write(self.spool.read(int(row["size"])))
            rows = rows.copy()
            rows["off"] = pos + np.r_[0, np.cumsum(rows["size"])[:-1]].astype(np.uint64)
            ix_at = fh.tell()
            fh.write(cir_tree(rows, ix_at, ix_at))
            zoom_heads.append(struct.pack("<IIQQ", reduction(k, self.bin), 0, data_at, ix_at))
        self.spool.close()
        tree_at = fh.tell()
        fh.write(chrom_tree(self.names, range(len(self.names)), self.sizes, tree_at))
        fh.write(struct.pack("<I", self.magic))
        scale = 10 ** self.digits
        summary = struct.pack("<Qdddd", self.covered, (self.qmin or 0) / scale, self.qmax / scale, self.sum / scale, self.sumsq / scale ** 2)
        fh.seek(0)
        fh.write(struct.pack("<IHHQQQHHQQIQ", self.magic, 4, nlev, tree_at, self.data_at, index_at, *self.fields,
                             64 + 24 * ZOOM_LEVELS if self.autosql else 0, self.summary_at, max([self.buf_size] + self.zoom_buf[:nlev]), 0))
        fh.write(b"".join(zoom_heads) + bytes(24 * (ZOOM_LEVELS - nlev)))
        fh.write(self.autosql + summary)
        fh.write(struct.pack("<Q", self.nsections))
        fh.seek(0, os.SEEK_END)

    def close(self) -> None:
        """Drop the spool of a file that is not finished."""
        if not self.spool.closed:
            self.spool.close()
