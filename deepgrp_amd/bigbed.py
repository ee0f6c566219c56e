"""The bigBed file (`.bb`) of the scored repeats (`predict --bed_dir --bed_bigbed`), stated in numpy/Python.

What the file says is what the BED of the same flags says (bed.reference_lines): one item per line, columns 1-3 in binary, columns
4-9 as the line's own text.  The device writes the uncompressed item blocks and the coverage zoom records and deflates them
(dgrp_bed_blocks_batch, dgrp_bed_zoom_batch, dgrp_zlib_compress_batch); `BigBedBuilder` puts the container around them as the
writes come in.  bigBed is the BBI sibling of bigWig: the chromosome B+ tree, the cirTree, the zoom headers and the builder's
spool, leaves and levels are bigwig.py's.

The layout.  All fields are little-endian and every part is found through an absolute file offset.
  1. Header, 64 bytes: magic u32 0x8789F2EB, version u16 4, zoomLevels u16, chromosomeTreeOffset u64, fullDataOffset u64,
     fullIndexOffset u64, fieldCount u16 9, definedFieldCount u16 6, autoSqlOffset u64 304, totalSummaryOffset u64,
     uncompressBufSize u32 (the largest uncompressed block of the file, item blocks and zoom blocks alike), extensionOffset u64 0.
  2. Zoom headers, room for 10, zoomLevels of them valid, 24 bytes each, as in a bigWig.
  3. At offset 304 the autoSql text `AUTOSQL`, zero-terminated: the nine columns and what they mean.
  4. Directly behind the terminating zero the total summary, 40 bytes: basesCovered u64, then minVal 1.0, maxVal 1.0, sumData and
     sumSquares = basesCovered as doubles (all 0 with nothing covered).
  5. Directly behind that, at fullDataOffset, itemCount u64 -- the items, not the blocks -- then the blocks in the order they are
     produced (file order of the records, ascending start inside a record).  An item is chromId u32, chromStart u32, chromEnd u32 and
     `rest`: columns 4-9 of the BED line exactly as dgrp_format_bed_rows prints them, tab-separated, without the line feed, and one
     zero byte: `class3\\t812\\t.\\t0.8123\\t0.4000\\t0.9500\\0`.  A block is up to 512 consecutive items of ONE record, in row
     order, stored as one zlib stream: 78 01, one DEFLATE block, Adler-32.
  6. Data index at fullIndexOffset: bigwig.cir_tree with one leaf per block, blockSize 256, itemsPerSlot 512.
  7. Zoom levels, as in a bigWig (recordCount u32, zoom blocks of up to 1024 records of one write, a cirTree of the blocks): the
     COVERAGE of the items.  R_k = 1024 * 4^k, k = 0..9 (bigwig.reduction(k, 64)); level k is written when R_k is smaller than the
     largest chromSize and the level holds a record.  Window w of level k of a record is [w * R_k, (w + 1) * R_k); a window with a
     covered base gives one 32-byte record: chromId, chromStart = its first covered base, chromEnd = one past its last, validCount =
     its covered bases (u32 each), minVal = maxVal = 1.0f, sumData = sumSquares = (float)validCount.  The rows of one record never
     overlap (dgrp_bed_blocks_batch refuses rows that do), so the depth is 1 wherever a base is covered.
  8. Chromosome B+ tree (bigwig.chrom_tree): every record that reached the writer, records without an emitted item included;
     chromId is the record's ordinal in the input, chromSize is startpos + n, the end of the predicted span.
  9. Trailer: magic u32 0x8789F2EB.

A bigBed cannot hold a record with an empty name, two records of one name, or a record that ends above 2^32 - 1.

No program of the UCSC tree has read these files: the format above is checked by a reader written for the tests alone."""
from __future__ import annotations

import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import bigwig as bw

MAGIC = 0x8789F2EB
BLOCK_ITEMS = 512
ZOOM_BIN = 64                                       # bigwig.reduction(k, 64) = 1024 * 4^k
MAX_END = bw.MAX_END
AUTOSQL = (b'table deepgrpRepeats\n'
           b'"Repeats predicted by DeepGRP with the model\'s confidence in each element"\n'
           b'    (\n'
           b'    string chrom;      "Name of the record: the first word of its header"\n'
           b'    uint   chromStart; "Start of the element, 0-based"\n'
           b'    uint   chromEnd;   "End of the element, exclusive"\n'
           b'    string name;       "class<label>: the predicted repeat class"\n'
           b'    uint   score;      "Mean probability of the class over the element on the scale 0..1000"\n'
           b'    char[1] strand;    "Always ."\n'
           b'    float  mean;       "Mean of the merged probabilities of the class over the bases of the element"\n'
           b'    float  minProb;    "Smallest of those probabilities"\n'
           b'    float  agree;      "Fraction of the bases at which the class is the largest column"\n'
           b'    )\n\0')

BLOCK_DTYPE = np.dtype([("off", "<i8"), ("bytes", "<i8"), ("rec", "<i4"), ("start", "<u4"), ("end", "<u4"), ("items", "<u4")])


class BigBedWrite(NamedTuple):
    """What one write (a record, or a batch) adds to the bigBed file of its input: the records' names and chromSizes (startpos + n)
    and -- unless the input cannot have a bigBed (`refused`) or the write has no row (blocks None) -- the compressed item blocks
    back to back with the size of each and their table rows (BLOCK_DTYPE; rec counts inside the write, while the chromId inside
    an item is the record's ordinal in the input), the same for the zoom blocks (bigwig.ZOOM_BLOCK_DTYPE), the totals (covered, 1,
    1, covered, covered) and the chromId of the first record as the device wrote it."""
    names: List[bytes]
    sizes: List[int]
    refused: Optional[str] = None
    blocks: Optional[bytes] = None
    block_sizes: Optional[np.ndarray] = None
    block_table: Optional[np.ndarray] = None
    zoom: bytes = b""
    zoom_sizes: Optional[np.ndarray] = None
    zoom_table: Optional[np.ndarray] = None
    totals: Tuple[int, int, int, int, int] = (0, 0, 0, 0, 0)
    chrom0: Optional[int] = None


def end_refusal(names: Sequence[bytes], sizes: Sequence[int]) -> Optional[str]:
    """Why these records cannot lie in a bigBed by their ends, or None."""
    for nm, end in zip(names, sizes):
        if end > MAX_END:
            return (f"record {nm.decode('utf-8', 'replace')!r} ends at {end}, above 2^32 - 1 = {MAX_END}, the largest coordinate of "
                    "a bigBed")
    return None


# ---- the statements the kernels and the builder are tested against --------------------------------------------------------------
def reference_items(by_contig: bool, rows, scores, min_score: int = 0, chrom0: int = 0) -> List[Tuple[int, int, int, bytes]]:
    """(record in the call, start, end, the item's bytes) of every emitted row: bed.reference_lines states which rows are emitted
    and the text of `rest`."""
    from .bed import reference_lines
    out = []
    for k in range(len(rows)):
        line = reference_lines([b""], False, rows[k:k + 1], scores[k:k + 1], min_score)
        if not line:
            continue
        rest = line[:-1].split(b"\t", 3)[3]
        r = int(rows[k]["contig"]) if by_contig else 0
        start, end = int(rows[k]["start"]), int(rows[k]["end"])
        out.append((r, start, end, struct.pack("<III", chrom0 + r, start, end) + rest + b"\0"))
    return out


def reference_blocks(by_contig: bool, rows, scores, min_score: int = 0, chrom0: int = 0) -> Tuple[bytes, np.ndarray]:
    """What dgrp_bed_blocks_batch writes: -> (the uncompressed blocks back to back, their table, BLOCK_DTYPE)."""
    items = reference_items(by_contig, rows, scores, min_score, chrom0)
    table, blob, at, a = [], [], 0, 0
    while a < len(items):
        b = a
        while b < len(items) and b - a < BLOCK_ITEMS and items[b][0] == items[a][0]:
            b += 1
        data = b"".join(it[3] for it in items[a:b])
        table.append((at, len(data), items[a][0], items[a][1], items[b - 1][2], b - a))
        blob.append(data)
        at += len(data)
        a = b
    return b"".join(blob), np.array(table, BLOCK_DTYPE) if table else np.zeros(0, BLOCK_DTYPE)


def reference_zoom(by_contig: bool, rows, scores, min_score: int = 0, chrom0: int = 0):
    """What dgrp_bed_zoom_batch writes: -> (the 32-byte records of the ten levels back to back, record offsets [11], the block
    table (bigwig.ZOOM_BLOCK_DTYPE), block offsets [11]).  Every level is computed from the items themselves."""
    items = reference_items(by_contig, rows, scores, min_score, chrom0)
    rec_dtype = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid", "<u4"), ("min", "<f4"), ("max", "<f4"),
                          ("sum", "<f4"), ("sumsq", "<f4")])
    blob, table, roff, boff = [], [], [0], [0]
    for k in range(bw.ZOOM_LEVELS):
        R = bw.reduction(k, ZOOM_BIN)
        wins: dict = {}                                             # (record, window) -> [first, last, covered]; insertion order is file order
        for r, start, end, _b in items:
            for w in range(start // R, (end - 1) // R + 1):
                a, b = max(start, w * R), min(end, (w + 1) * R)
                have = wins.setdefault((r, w), [a, b, 0])
                have[1] = b
                have[2] += b - a
        recs = np.zeros(len(wins), rec_dtype)
        for i, ((r, _w), (a, b, n)) in enumerate(wins.items()):
            recs[i] = (chrom0 + r, a, b, n, 1.0, 1.0, np.float32(n), np.float32(n))
        keys = list(wins)
        for a in range(0, len(recs), bw.SECTION_ITEMS):
            b = min(a + bw.SECTION_ITEMS, len(recs))
            table.append((32 * (roff[-1] + a), 32 * (b - a), 0, k, keys[a][0], keys[b - 1][0], int(recs["start"][a]), int(recs["end"][b - 1])))
        blob.append(recs.tobytes())
        roff.append(roff[-1] + len(recs))
        boff.append(len(table))
    return (b"".join(blob), np.array(roff, np.int64), np.array(table, bw.ZOOM_BLOCK_DTYPE) if table else np.zeros(0, bw.ZOOM_BLOCK_DTYPE),
            np.array(boff, np.int64))


def reference_totals(by_contig: bool, rows, scores, min_score: int = 0) -> Tuple[int, int, int, int, int]:
    """(covered, 1, 1, covered, covered) of the emitted rows, zeros when nothing is covered."""
    covered = sum(end - start for _r, start, end, _b in reference_items(by_contig, rows, scores, min_score))
    return (covered, 1, 1, covered, covered) if covered else (0, 0, 0, 0, 0)


class BigBedBuilder(bw.BigWigBuilder):
    """One `.bb` file on the open binary file `fh` (empty, seekable): bigwig.BigWigBuilder with bigBed's header fields, the autoSql
    text, the item count at fullDataOffset and itemsPerSlot 512; `add` takes a BigBedWrite."""
    magic = MAGIC
    fields = (9, 6)
    autosql = AUTOSQL
    items_per_slot = BLOCK_ITEMS

    def __init__(self, fh, spool_dir: Optional[str] = None):
        super().__init__(fh, 0, ZOOM_BIN, spool_dir)                 # (digits 0: the totals are counts of bases, the values 1)

    @staticmethod
    def counted(table: np.ndarray) -> int:
        return int(table["items"].sum())

    def add(self, names: Sequence[bytes], sizes: Sequence[int], w: Optional[BigBedWrite] = None) -> None:
        if w is None or w.blocks is None:
            return super().add(names, sizes, None)
        empty = np.zeros(0, np.int64)
        super().add(names, sizes, bw.ClassWrite(w.blocks, w.block_sizes, w.block_table, w.zoom,
                                                empty if w.zoom_sizes is None else w.zoom_sizes,
                                                np.zeros(0, bw.ZOOM_BLOCK_DTYPE) if w.zoom_table is None else w.zoom_table, w.totals))
