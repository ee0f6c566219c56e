"""The tabix index (`.tbi`) of a BGZF bedGraph track (`predict --track_dir --track_gzip --track_index`), stated in numpy/Python.
The index of a scored BED (`predict --bed_dir --bed_gzip --bed_index`) is the same statement: `reference_index` reads nothing but
name, start and end of every line, so the `.tbi` of a `.bed.gz` is `reference_index` of that file; its lines vary in width, may
be nested and may span many 16 kb windows, which is what the running maximum in the linear index's rule is for.

`reference_index` computes the index's payload from a finished `.gz` file alone and is the statement every other path is held to;
`IndexBuilder` puts the same payload together from what the track writer knows (chunks and linear index in text offsets from
dgrp_track_index_batch, the compressed size of every member written); `read_index` and `query` are a small reader that works as
tabix does.  The `.tbi` file is the payload as BGZF (`index_file`).

The format.  Bins are the standard scheme with min_shift 14 and depth 5 (`reg2bin`), so coordinates end at or below 2^29.  The
virtual offset of text byte u is (file offset of the BGZF member that holds u) << 16 | (offset of u inside that member); for u = the
text's length it is (offset of the EOF member) << 16, so the end of a line is always the virtual offset of the byte behind it.
Reference sequences are the distinct names in order of first appearance.  A chunk (the rule of htslib's hts_idx_push) is a maximal
run of consecutive lines with the same name and the same bin, from its first line's begin to its last line's end; there is no
further merging and no pseudo-bin 37450.  The linear index of a sequence has n_intv = ((end of its last line - 1) >> 14) + 1 entries,
ioff[w] = the begin of its first line whose end is greater than w << 14.  Bytes: `TBI\\1`, n_ref, format 0x10000 (generic, zero-based
half-open: htslib's `bed` preset), col_seq 1, col_beg 2, col_end 3, meta `#`, skip 0, l_nm, the names with a NUL each; per sequence
n_bin, the bins in ascending number (bin, n_chunk, (beg, end)... in file order), n_intv, ioff...; n_no_coor = 0 as uint64.

A GFF3 file (`predict --bed_gff3`, gff.py) has the same index under htslib's `gff` preset (PRESET_GFF: format 0, col_seq 1, col_beg
4, col_end 5, one-based closed columns): `payload`, `reference_index`, `read_index`, `query` and `IndexBuilder` take the preset as
an optional last argument and do for PRESET_BED, the default, what they did without it.

The CSI index (`.csi`, `predict --index_format csi`), version 1, not yet read by an htslib tool.  A `.tbi` ends at 2^29; a CSI index
has the same chunks under a binning scheme of configurable depth and, in place of the linear index, one `loffset` per bin.  With
min_shift 14 and depth D the levels are 0..D; level l starts at bin ((1 << 3l) - 1) / 7 and has shift 14 + 3 (D - l).  For D = 6
(CSI_DEPTH) the first bins are 0, 1, 9, 73, 585, 4681, 37449, there are 299 593 bins and the largest coordinate is 2^32, the limit
of 2bit, bigWig and bigBed.  `csi_reg2bin(beg, end, depth)` searches from level D upwards and returns first(l) + (beg >> shift(l)) at
the first level where beg >> shift == (end - 1) >> shift, 0 otherwise; at depth 5 it is `reg2bin`, and below 2^29 a `.tbi` bin
first5(l) + o is the depth-6 bin first6(l + 1) + o.  The chunk rule is unchanged: a maximal run of consecutive lines of one name and
one bin, no merging, no pseudo-bin.  A bin at level l with offset o inside its level has the bottom window o << 3 (D - l), the first
16 kb window it covers; its loffset is ioff[bottom window], ioff[w] by the rule of the linear index stated above: the begin of the
sequence's first line, in file order, whose end is greater than w << 14.  That line exists for the bottom window of every bin that
holds a line: the window is at or below (the line's begin) >> 14, and the line ends above its begin.  So no bin gets the 0 that
stands for "no line".  Where the starts of a sequence ascend -- always inside one record -- the sequence's last line starts at or
behind every earlier line, every such window lies inside n_intv = ((that line's end - 1) >> 14) + 1, and ioff is the `.tbi`'s own
array.  Consecutive records of one name are one sequence whose starts begin again at 0: a bin of the first record may then have its
bottom window at or behind n_intv, where a `.tbi` has no entry; the rule still names a line there, and a CSI index has room for it.
ioff does not descend with w (the lines that end above w << 14 get fewer), whatever the order of the starts, which is what
`csi_query` rests on: every line that overlaps a region ends above its begin, so it lies at or behind ioff[w] for every w at or
below begin >> 14, and the loffset of any bin in front of the region's begin is at or below ioff[begin >> 14].  Bytes: `CSI\1`, min_shift i32 = 14, depth i32, l_aux i32 = 28 + l_nm; aux =
the seven int32 of the `.tbi` header behind n_ref (format, col_seq, col_beg, col_end, meta `#`, skip 0, l_nm) and the names with a NUL
each; n_ref i32; per sequence n_bin i32 and the bins in ascending number (bin u32, loffset u64, n_chunk i32, (beg, end) u64 pairs in
file order); n_no_coor u64 = 0.  The `.csi` file is that payload as BGZF (`index_file`).  `csi_reference_index` states it from the
finished `.gz` alone, `IndexBuilder(fmt="csi")` puts it together from the writer's pieces (chunks with depth-D bins from
dgrp_track_csi_batch and its kin, the same 16 kb linear arrays), `read_csi` and `csi_query` read it as htslib does."""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MIN_SHIFT = 14
MAX_END = 1 << 29
CSI_DEPTH = 6                                       # of a `.csi` written here: coordinates up to 2^32
FORMAT_BED = 0x10000
PRESET_BED = (FORMAT_BED, 1, 2, 3)                  # (format, col_seq, col_beg, col_end), columns counted from 1
PRESET_GFF = (0, 1, 4, 5)                           # generic, one-based closed: htslib's `gff` preset
_LEVELS = ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1))
BLOCK = 0xff00                                      # text bytes per member of a write (gz.BGZF_BLOCK)

CHUNK_DTYPE = np.dtype([("beg", "<i8"), ("end", "<i8"), ("rec", "<i4"), ("bin", "<u4")])     # struct dgrp_track_chunk


class IndexRefused(ValueError):
    """The file has no tabix index: coordinates above 2^29, a name that reappears after another name, an empty name."""


def reg2bin(beg: int, end: int) -> int:
    """The bin of [beg, end) (end exclusive, 0 <= beg < end <= 2^29)."""
    if not 0 <= beg < end <= MAX_END:
        raise IndexRefused(f"[{beg}, {end}) is not a span inside [0, 2^29]")
    end -= 1
    for shift, first in _LEVELS:
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def csi_max_end(depth: int) -> int:
    """The largest coordinate of an index with min_shift 14 and `depth` levels below the root: 2^29 at 5, 2^32 at 6."""
    return 1 << (MIN_SHIFT + 3 * depth)


def end_refusal(ends, names: Optional[Sequence[bytes]] = None, depth: int = 5) -> Optional[str]:
    """Why records that end at `ends` cannot have an index (the first that ends above 2^29, by its name or, without names, by its
    ordinal), or None.  With another depth: above 2^(14 + 3 depth), the limit of a CSI index of that depth."""
    top, power = csi_max_end(depth), f"2^{MIN_SHIFT + 3 * depth}"
    what = "a tabix index" if depth == 5 else f"a CSI index of depth {depth}"
    for i, end in enumerate(np.asarray(ends, np.int64).tolist()):
        if end > top:
            who, limit = (i, power) if names is None else (repr(names[i].decode("utf-8", "replace")), f"{power} = {top}")
            return f"record {who} ends at {end}, above {limit}, the largest coordinate of {what}"
    return None


def window_prefix(ends, depth: int = 5) -> np.ndarray:
    """wpref [records + 1] of records that end at `ends`: record r has the ((end - 1) >> MIN_SHIFT) + 1 windows of 16 kb up to its
    end, at [wpref[r], wpref[r + 1]) of a linear index.  A record that ends above 2^29 (2^(14 + 3 depth) with a depth) raises
    IndexRefused (end_refusal's text)."""
    if end_refusal(ends, None, depth) is not None:
        raise IndexRefused(end_refusal(ends, None, depth))
    return np.r_[np.int64(0), np.cumsum(((np.asarray(ends, np.int64) - 1) >> MIN_SHIFT) + 1, dtype=np.int64)]


def reg2bins(beg: int, end: int) -> List[int]:
    """Every bin that can hold a line overlapping [beg, end)."""
    end = min(end, MAX_END) - 1
    out = [0]
    for shift, first in reversed(_LEVELS):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def _csi_first(level: int) -> int:
    return ((1 << 3 * level) - 1) // 7


def csi_reg2bin(beg: int, end: int, depth: int = CSI_DEPTH) -> int:
    """The bin of [beg, end) (end exclusive, 0 <= beg < end <= 2^(14 + 3 depth)) in the scheme of `depth` levels below the root."""
    if not 0 <= beg < end <= csi_max_end(depth):
        raise IndexRefused(f"[{beg}, {end}) is not a span inside [0, 2^{MIN_SHIFT + 3 * depth}]")
    end -= 1
    for level in range(depth, 0, -1):
        shift = MIN_SHIFT + 3 * (depth - level)
        if beg >> shift == end >> shift:
            return _csi_first(level) + (beg >> shift)
    return 0


def csi_reg2bins(beg: int, end: int, depth: int = CSI_DEPTH) -> List[int]:
    """Every bin of that scheme that can hold a line overlapping [beg, end)."""
    end = min(end, csi_max_end(depth)) - 1
    out = [0]
    for level in range(1, depth + 1):
        shift = MIN_SHIFT + 3 * (depth - level)
        out.extend(range(_csi_first(level) + (beg >> shift), _csi_first(level) + (end >> shift) + 1))
    return out


def csi_bottom_window(b: int, depth: int = CSI_DEPTH) -> int:
    """The first 16 kb window that bin `b` covers: o << 3 (depth - l) for the bin at offset o of level l."""
    level = 0
    while level < depth and b >= _csi_first(level + 1):
        level += 1
    return (b - _csi_first(level)) << 3 * (depth - level)


def csi_payload(names: Sequence[bytes], bins: Sequence[Dict[int, List[Tuple[int, int]]]], loffsets: Sequence[Dict[int, int]],
                preset: Tuple[int, int, int, int] = PRESET_BED, depth: int = CSI_DEPTH) -> bytes:
    """The CSI index's bytes from its parts: per sequence its name, bin -> [(beg, end), ...] in file order, and bin -> loffset."""
    blob = b"".join(nm + b"\0" for nm in names)
    out = [b"CSI\1", struct.pack("<3i", MIN_SHIFT, depth, 28 + len(blob)), struct.pack("<7i", *preset, ord("#"), 0, len(blob)), blob,
           struct.pack("<i", len(names))]
    for b, lo in zip(bins, loffsets):
        out.append(struct.pack("<i", len(b)))
        for k in sorted(b):
            out.append(struct.pack("<IQi", k, lo[k], len(b[k])))
            out.append(np.asarray(b[k], "<u8").tobytes())
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def _csi_loffsets(bins: Dict[int, list], lin, depth: int) -> Dict[int, int]:
    """loffset of every bin of one sequence from `lin`, its linear index with an entry for every window a line of it ends above
    (not cut to n_intv: a bin's bottom window may lie behind the last line's)."""
    return {k: int(lin[csi_bottom_window(k, depth)]) for k in bins}


def payload(names: Sequence[bytes], bins: Sequence[Dict[int, List[Tuple[int, int]]]], linear: Sequence[Sequence[int]],
            preset: Tuple[int, int, int, int] = PRESET_BED) -> bytes:
    """The index's bytes from its parts: per sequence its name, bin -> [(beg, end), ...] in file order, and ioff."""
    blob = b"".join(nm + b"\0" for nm in names)
    out = [b"TBI\1", struct.pack("<8i", len(names), *preset, ord("#"), 0, len(blob)), blob]
    for b, lin in zip(bins, linear):
        out.append(struct.pack("<i", len(b)))
        for k in sorted(b):
            out.append(struct.pack("<Ii", k, len(b[k])))
            out.append(np.asarray(b[k], "<u8").tobytes())
        out.append(struct.pack("<i", len(lin)))
        out.append(np.asarray(lin, "<u8").tobytes())
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def index_file(pl: bytes) -> bytes:
    """The `.tbi` file of a payload: BGZF from the host, EOF member included."""
    from .gz import bgzf_compress
    return bgzf_compress(pl)


def _member_size(gz_bytes, off: int) -> int:
    if gz_bytes[off:off + 4] != b"\x1f\x8b\x08\x04" or gz_bytes[off + 12:off + 16] != b"BC\x02\x00":
        raise ValueError(f"no BGZF member at byte {off}")
    return struct.unpack_from("<H", gz_bytes, off + 16)[0] + 1


def _inflate_member(gz_bytes, off: int) -> Tuple[bytes, int]:
    size = _member_size(gz_bytes, off)
    return zlib.decompress(bytes(gz_bytes[off:off + size]), 31), size


def _interval(f: List[bytes], preset) -> Tuple[bytes, int, int]:
    """(sequence, beg, end), zero-based half-open, of a line's columns under a preset."""
    beg = int(f[preset[2] - 1])
    return f[preset[1] - 1], beg if preset[0] & FORMAT_BED else beg - 1, int(f[preset[3] - 1])


def reference_index(gz_bytes: bytes, preset: Tuple[int, int, int, int] = PRESET_BED) -> bytes:
    """The payload of the index of the BGZF bedGraph file `gz_bytes`, from the file alone: a walk over its members, zlib, the lines.
    Under PRESET_GFF the lines that start with the meta character `#` are skipped, as tabix skips them."""
    names, bins, linear, last_end = _reference_parts(gz_bytes, preset, reg2bin)
    return payload(names, bins, [lin[:((e - 1) >> MIN_SHIFT) + 1] for lin, e in zip(linear, last_end)], preset)


def csi_reference_index(gz_bytes: bytes, preset: Tuple[int, int, int, int] = PRESET_BED, depth: int = CSI_DEPTH) -> bytes:
    """The payload of the CSI index of that file, from the file alone: the same walk with the bins of `depth` levels, and every
    bin's loffset read from the linear index the `.tbi` statement defines."""
    names, bins, linear, _last = _reference_parts(gz_bytes, preset, lambda beg, end: csi_reg2bin(beg, end, depth))
    return csi_payload(names, bins, [_csi_loffsets(b, lin, depth) for b, lin in zip(bins, linear)], preset, depth)


def _reference_parts(gz_bytes: bytes, preset, bin_of):
    """(names, bins, linear, last_end) of the file, the bin of a line's interval given by bin_of(beg, end): per sequence
    bin -> chunks, ioff for every window a line ends above, and the end of its last line (which cuts a `.tbi`'s linear index)."""
    starts, tstarts, parts = [], [], []
    off = total = 0
    while off < len(gz_bytes):
        text, size = _inflate_member(gz_bytes, off)
        starts.append(off)
        tstarts.append(total)
        parts.append(text)
        total += len(text)
        off += size
    text = b"".join(parts)
    tstarts = np.asarray(tstarts, np.int64)

    def voff(u: int) -> int:
        m = int(np.searchsorted(tstarts, u, "right")) - 1               # the last member that starts at or in front of u
        return starts[m] << 16 | (u - int(tstarts[m]))

    names: List[bytes] = []
    bins: List[Dict[int, List[Tuple[int, int]]]] = []
    linear: List[List[int]] = []
    last_end: List[int] = []
    run = None                                                          # the open chunk: [sequence, bin, begin, end] in text offsets
    u = 0
    lines = text.split(b"\n")
    if not lines[-1]:
        lines.pop()
    for line in lines:
        v = u + len(line) + 1
        if preset != PRESET_BED and line.startswith(b"#"):
            u = v
            continue
        name, beg, end = _interval(line.split(b"\t"), preset)
        if not name:
            raise IndexRefused("a line with an empty name")
        if not names or names[-1] != name:
            if name in names:
                raise IndexRefused(f"the name {name!r} reappears after another name")
            names.append(name)
            bins.append({})
            linear.append([])
            last_end.append(0)
        s = len(names) - 1
        b = bin_of(beg, end)
        if run is not None and run[0] == s and run[1] == b:
            run[3] = v
        else:
            if run is not None:
                bins[run[0]].setdefault(run[1], []).append((voff(run[2]), voff(run[3])))
            run = [s, b, u, v]
        lin = linear[s]
        if (end - 1) >> MIN_SHIFT >= len(lin):                          # the first line whose end is greater than w << 14
            lin.extend([voff(u)] * (((end - 1) >> MIN_SHIFT) + 1 - len(lin)))
        last_end[s] = end
        u = v
    if run is not None:
        bins[run[0]].setdefault(run[1], []).append((voff(run[2]), voff(run[3])))
    return names, bins, linear, last_end


def read_index(pl: bytes, preset: Tuple[int, int, int, int] = PRESET_BED) -> dict:
    """The payload's parts: {"names": [...], "bins": [{bin: [(beg, end), ...]}, ...], "linear": [uint64 array, ...]}."""
    if pl[:4] != b"TBI\1":
        raise ValueError("not a tabix index")
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", pl, 4)
    if (fmt, col_seq, col_beg, col_end) != tuple(preset):
        raise ValueError("not an index of the bed preset" if preset == PRESET_BED else f"not an index of the preset {preset}")
    p = 36
    names = pl[p:p + l_nm].split(b"\0")[:-1]
    p += l_nm
    bins, linear = [], []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", pl, p)
        p += 4
        b = {}
        for _k in range(n_bin):
            k, n_chunk = struct.unpack_from("<Ii", pl, p)
            p += 8
            c = np.frombuffer(pl, "<u8", 2 * n_chunk, p).reshape(-1, 2)
            p += 16 * n_chunk
            b[k] = [(int(x), int(y)) for x, y in c]
        n_intv, = struct.unpack_from("<i", pl, p)
        p += 4
        linear.append(np.frombuffer(pl, "<u8", n_intv, p))
        p += 8 * n_intv
        bins.append(b)
    if len(names) != n_ref or p + 8 > len(pl):
        raise ValueError("truncated tabix index")
    return {"names": names, "bins": bins, "linear": linear}


def query(index: dict, gz_bytes: bytes, name: bytes, beg: int, end: int, preset: Tuple[int, int, int, int] = PRESET_BED) -> List[bytes]:
    """The lines of sequence `name` that overlap [beg, end), in file order, as tabix finds them: the bins of the region, their
    chunks that end above ioff[beg >> 14], only the members those chunks touch, and an overlap filter on the lines."""
    if name not in index["names"] or beg >= end:
        return []
    s = index["names"].index(name)
    lin = index["linear"][s]
    w = beg >> MIN_SHIFT
    min_off = int(lin[w]) if w < len(lin) else (int(lin[-1]) if len(lin) else 0)
    chunks = sorted(c for b in reg2bins(beg, end) for c in index["bins"][s].get(b, ()) if c[1] > min_off)
    out = []
    for cb, ce in chunks:
        off, parts = cb >> 16, []
        while off < ce >> 16 or (off == ce >> 16 and ce & 0xffff):
            text, size = _inflate_member(gz_bytes, off)
            parts.append(text if off < ce >> 16 else text[:ce & 0xffff])
            off += size
        for line in b"".join(parts)[cb & 0xffff:].split(b"\n")[:-1]:
            if preset != PRESET_BED and line.startswith(b"#"):
                continue
            seq, lb, le = _interval(line.split(b"\t"), preset)
            if seq == name and lb < end and le > beg:
                out.append(line)
    return out


def _chunk_lines(gz_bytes: bytes, chunks) -> List[bytes]:
    """The lines of the chunks (virtual-offset pairs), reading only the members they touch."""
    out = []
    for cb, ce in chunks:
        off, parts = cb >> 16, []
        while off < ce >> 16 or (off == ce >> 16 and ce & 0xffff):
            text, size = _inflate_member(gz_bytes, off)
            parts.append(text if off < ce >> 16 else text[:ce & 0xffff])
            off += size
        out.extend(b"".join(parts)[cb & 0xffff:].split(b"\n")[:-1])
    return out


def read_csi(pl: bytes) -> dict:
    """The CSI payload's parts: {"names": [...], "depth": D, "preset": (format, col_seq, col_beg, col_end), "bins": [{bin: (loffset,
    [(beg, end), ...])}, ...]}."""
    if pl[:4] != b"CSI\1":
        raise ValueError("not a CSI index")
    min_shift, depth, l_aux = struct.unpack_from("<3i", pl, 4)
    if min_shift != MIN_SHIFT or depth < 1 or l_aux < 28:
        raise ValueError(f"a CSI index with min_shift {min_shift}, depth {depth}, {l_aux} bytes of aux")
    fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<7i", pl, 16)
    if l_aux != 28 + l_nm:
        raise ValueError("the aux block of the CSI index is not a tabix header")
    p = 44
    names = pl[p:p + l_nm].split(b"\0")[:-1]
    p += l_nm
    n_ref, = struct.unpack_from("<i", pl, p)
    p += 4
    bins = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", pl, p)
        p += 4
        b = {}
        for _k in range(n_bin):
            k, loff, n_chunk = struct.unpack_from("<IQi", pl, p)
            p += 16
            c = np.frombuffer(pl, "<u8", 2 * n_chunk, p).reshape(-1, 2)
            p += 16 * n_chunk
            b[k] = (loff, [(int(x), int(y)) for x, y in c])
        bins.append(b)
    if len(names) != n_ref or p + 8 > len(pl):
        raise ValueError("truncated CSI index")
    return {"names": names, "depth": depth, "preset": (fmt, col_seq, col_beg, col_end), "bins": bins}


def csi_min_off(bins: Dict[int, tuple], beg: int, depth: int) -> int:
    """The offset in front of which no line of the sequence overlaps a region that begins at `beg`, as htslib finds it: start at the
    bottom-level bin of beg; while that bin is absent step to the previous sibling, at a first child to the parent, up to bin 0;
    the loffset of the bin found, or 0."""
    b = _csi_first(depth) + (min(beg, csi_max_end(depth) - 1) >> MIN_SHIFT)
    while b and b not in bins:
        parent = (b - 1) >> 3
        b = b - 1 if b > (parent << 3) + 1 else parent
    return bins[b][0] if b in bins else 0


def csi_query(index: dict, gz_bytes: bytes, name: bytes, beg: int, end: int, use_loffset: bool = True) -> List[bytes]:
    """The lines of sequence `name` that overlap [beg, end), in file order, as htslib finds them in a CSI index (`read_csi`): the
    bins of the region, their chunks that end above min_off (csi_min_off; 0 without use_loffset: the bins alone), only the members
    those chunks touch, and an overlap filter on the lines."""
    if name not in index["names"] or beg >= end:
        return []
    preset, depth = tuple(index["preset"]), index["depth"]
    bins = index["bins"][index["names"].index(name)]
    min_off = csi_min_off(bins, beg, depth) if use_loffset else 0
    chunks = sorted(c for b in csi_reg2bins(beg, end, depth) if b in bins for c in bins[b][1] if c[1] > min_off)
    out = []
    for line in _chunk_lines(gz_bytes, chunks):
        if preset != PRESET_BED and line.startswith(b"#"):
            continue
        seq, lb, le = _interval(line.split(b"\t"), preset)
        if seq == name and lb < end and le > beg:
            out.append(line)
    return out


def member_sizes(members: bytes) -> Tuple[np.ndarray, int]:
    """(the compressed size of every BGZF member of `members`, the text bytes they hold), from their BSIZE and ISIZE fields."""
    out, off, text_len = [], 0, 0
    while off < len(members):
        out.append(_member_size(members, off))
        off += out[-1]
        text_len += struct.unpack_from("<I", members, off - 4)[0]
    return np.asarray(out, np.int64), text_len


class IndexBuilder:
    """The index of one track file from its writes.  A write is the BGZF members of one text (one record, or one class of a batch)
    appended at a file offset; every write starts a member and its members hold BLOCK text bytes each but the last, so text offset u
    of a write lies in member u // BLOCK of it."""

    def __init__(self, preset: Tuple[int, int, int, int] = PRESET_BED, fmt: str = "tbi", depth: int = 5):
        """fmt "csi": the same `add` calls with chunks that carry the bins of `depth` levels; the linear arrays come in 16 kb windows
        as for a `.tbi` and are kept, merged per sequence, only to read every bin's loffset from; `payload` gives the CSI bytes."""
        if fmt not in ("tbi", "csi") or (fmt == "tbi" and depth != 5):
            raise ValueError(f"no index of format {fmt!r} and depth {depth}")
        self.preset, self.fmt, self.depth = preset, fmt, depth
        self.names: List[bytes] = []
        self.bins: List[Dict[int, List[List[int]]]] = []
        self.linear: List[np.ndarray] = []
        self.n_intv: List[int] = []
        self.last_bin = -1                                              # the bin of the last chunk of the last sequence

    def add(self, file_off: int, sizes: np.ndarray, text_len: int, rec_names: Sequence[bytes], chunks: np.ndarray, linear: np.ndarray,
            wpref: np.ndarray, last_end=None) -> None:
        """One write of `text_len` text bytes in members of `sizes` compressed bytes at `file_off`: its chunks (CHUNK_DTYPE, text
        offsets, `rec` an index into rec_names) and its linear index (record r at linear[wpref[r]:wpref[r + 1]], -1: no line).
        last_end[r], where given, is the end of record r's last line: a BED's ends need not ascend, and the sequence's linear index
        ends with its last line, not with its longest (a track's ends ascend: both are one)."""
        mstart = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum(sizes, out=mstart[1:])
        if len(sizes) != (text_len + BLOCK - 1) // BLOCK:
            raise ValueError(f"{len(sizes)} members for {text_len} bytes of text")

        def voff(u):
            u = np.asarray(u, np.int64)
            m = u // BLOCK
            v = (file_off + mstart[np.minimum(m, len(sizes))]) << 16 | (u - m * BLOCK)
            return np.where(u >= text_len, (file_off + int(mstart[-1])) << 16, v)

        cb, ce = voff(chunks["beg"]).tolist(), voff(chunks["end"]).tolist()
        for rec, b, vb, ve in zip(chunks["rec"].tolist(), chunks["bin"].tolist(), cb, ce):
            name = rec_names[rec]
            if not self.names or self.names[-1] != name:
                if name in self.names or not name:
                    raise IndexRefused(f"the name {name!r} reappears after another name" if name else "an empty name")
                self.names.append(name)
                self.bins.append({})
                self.linear.append(np.zeros(0, np.int64))
                self.n_intv.append(0)
                self.last_bin = -1
            if b == self.last_bin:                                      # consecutive records of one name: the run goes on
                self.bins[-1][b][-1][1] = ve
            else:
                self.bins[-1].setdefault(b, []).append([vb, ve])
                self.last_bin = b
        for r in np.unique(chunks["rec"]).tolist():                     # the records with a line, in order
            lin = linear[wpref[r]:wpref[r + 1]]
            lin = voff(lin[:int(np.flatnonzero(lin >= 0)[-1]) + 1])
            s = self.names.index(rec_names[r])
            have = self.linear[s]                                       # an earlier record's line comes first in the file
            self.linear[s] = np.concatenate([have, lin[len(have):]])
            # ... but the sequence ends with its last line
            self.n_intv[s] = len(lin) if last_end is None else ((int(last_end[r]) - 1) >> MIN_SHIFT) + 1

    def payload(self) -> bytes:
        if self.fmt == "csi":                                          # (loffset reads the whole merged array, not its first n_intv)
            return csi_payload(self.names, self.bins, [_csi_loffsets(b, lin, self.depth) for b, lin in zip(self.bins, self.linear)],
                               self.preset, self.depth)
        return payload(self.names, self.bins, [lin[:n] for lin, n in zip(self.linear, self.n_intv)], self.preset)
