"""An independent bigBed reader for the tests (not a test): `struct` and `zlib.decompress` only, no code of deepgrp_amd.  It reads the
file the way a browser does -- header, autoSql, zoom headers, total summary, chromosome B+ tree, the items through the R-tree (a full
walk and range queries) and every zoom level -- and asserts the container's invariants on the way.  The walkers of the chromosome
tree and of a zoom level are bigwig_reader's, unchanged."""
import struct

from bigwig_reader import CIR_MAGIC, BigWig

MAGIC = 0x8789F2EB
BLOCK_ITEMS = 512


class BigBed(BigWig):
    def __init__(self, data: bytes):
        self.d = data
        (magic, self.version, self.nzoom, self.chrom_at, self.data_at, self.index_at, self.field_count, self.defined_fields, self.autosql_at,
         self.summary_at, self.buf_size, extension) = struct.unpack_from("<IHHQQQHHQQIQ", data, 0)
        assert magic == MAGIC and self.version == 4 and extension == 0
        assert struct.unpack_from("<I", data, len(data) - 4)[0] == MAGIC, "trailer"
        assert 0 <= self.nzoom <= 10
        self.zoom_heads = [struct.unpack_from("<IIQQ", data, 64 + 24 * k) for k in range(self.nzoom)]
        assert data[64 + 24 * self.nzoom:64 + 240] == bytes(24 * (10 - self.nzoom))
        assert self.autosql_at == 304
        stop = data.index(b"\0", self.autosql_at)
        self.autosql = data[self.autosql_at:stop]
        assert self.summary_at == stop + 1 and self.data_at == self.summary_at + 40, "autoSql, summary and data lie back to back"
        self.summary = struct.unpack_from("<Qdddd", data, self.summary_at)
        self.chroms = self._walk_chroms()                       # [(key, id, size)] in key order
        self.item_count = struct.unpack_from("<Q", data, self.data_at)[0]
        self.inflated_max = 0

    def _data_leaves(self, query=None):
        """The leaf items (sc, sb, ec, eb, off, size) of the data index in tree order; with query = (chrom, beg, end) only those that
        overlap.  (bigwig_reader's walk, for a tree of itemsPerSlot 512.)"""
        at = self.index_at
        magic, bs, n, sc, sb, ec, eb, end_off, per_slot, res = struct.unpack_from("<IIQIIIIQII", self.d, at)
        assert magic == CIR_MAGIC and bs == 256 and per_slot == BLOCK_ITEMS and res == 0 and end_off == self.index_at
        out = []

        def overlaps(b):
            if query is None:
                return True
            c, beg, end = query
            return (b[0], b[1]) < (c, end) and (b[2], b[3]) > (c, beg)

        def node(p, bounds):
            leaf, _r, count = struct.unpack_from("<BBH", self.d, p)
            assert count <= bs
            for i in range(count):
                it = struct.unpack_from("<IIIIQQ", self.d, p + 4 + 32 * i) if leaf else struct.unpack_from("<IIIIQ", self.d, p + 4 + 24 * i)
                if bounds is not None:
                    assert (it[0], it[1]) >= (bounds[0], bounds[1]) and (it[2], it[3]) <= (bounds[2], bounds[3]), "a node's bounds contain its children's"
                if not overlaps(it):
                    continue
                if leaf:
                    out.append(it)
                else:
                    node(it[4], it)
        node(at + 48, (sc, sb, ec, eb) if n else None)
        if query is None:
            assert len(out) == n
        return out, n

    @staticmethod
    def _block(raw):
        """[(chromId, start, end, rest)] of one inflated block."""
        items, p = [], 0
        while p < len(raw):
            cid, start, end = struct.unpack_from("<III", raw, p)
            stop = raw.index(b"\0", p + 12)
            items.append((cid, start, end, raw[p + 12:stop]))
            p = stop + 1
        assert 1 <= len(items) <= BLOCK_ITEMS and len({it[0] for it in items}) == 1, "a block holds 1..512 items of one chromosome"
        assert all(s < e for _c, s, e, _r in items) and all(a[2] <= b[1] for a, b in zip(items, items[1:]))
        return items

    def blocks(self, query=None):
        leaves, _n = self._data_leaves(query)
        if query is None:
            assert all((a[2], a[3]) <= (b[0], b[1]) for a, b in zip(leaves, leaves[1:])), "(chromId, start) order, no overlap"
            at = self.data_at + 8
            for it in leaves:                                    # back to back behind itemCount
                assert it[4] == at
                at += it[5]
            assert at == self.index_at
        out = []
        for sc, sb, ec, eb, off, size in leaves:
            items = self._block(self._inflate(off, size))
            assert (sc, sb, ec, eb) == (items[0][0], items[0][1], items[0][0], items[-1][2])
            out.append(items)
        return out

    def items(self):
        """[(chromId, start, end, rest)] of the whole file."""
        out = [it for block in self.blocks() for it in block]
        assert len(out) == self.item_count
        return out

    def query(self, chrom_id, beg, end):
        return [it for block in self.blocks((chrom_id, beg, end)) for it in block if it[1] < end and it[2] > beg]

    def lines(self):
        """The items as BED text: the chromosome's name, start, end and `rest`."""
        name = {cid: key for key, cid, _size in self.chroms}
        return b"".join(b"%s\t%d\t%d\t%s\n" % (name[c], s, e, rest) for c, s, e, rest in self.items())

    def check_all(self):
        """Everything once: -> (items, [zoom levels]); every zoom level is recomputed from the items, and so is the summary."""
        items = self.items()
        zooms = [self.zoom(k) for k in range(self.nzoom)]
        assert self.buf_size == self.inflated_max, "uncompressBufSize is the largest block"
        sizes = {cid: size for _key, cid, size in self.chroms}
        assert all(c in sizes and e <= sizes[c] for c, _s, e, _r in items)
        covered = sum(e - s for _c, s, e, _r in items)
        assert self.summary == ((covered, 1.0, 1.0, float(covered), float(covered)) if covered else (0, 0.0, 0.0, 0.0, 0.0))
        longest = max(sizes.values(), default=0)
        want_levels = 0
        while want_levels < 10 and items and 1024 * 4 ** want_levels < longest:
            want_levels += 1
        assert self.nzoom == want_levels
        for k, (red, recs) in enumerate(zooms):
            assert red == 1024 * 4 ** k
            wins = {}
            for c, s, e, _r in items:
                for w in range(s // red, (e - 1) // red + 1):
                    a, b = max(s, w * red), min(e, (w + 1) * red)
                    have = wins.setdefault((c, w), [a, b, 0])
                    have[1] = b
                    have[2] += b - a
            want = [(c, a, b, n, 1.0, 1.0, struct.unpack("<f", struct.pack("<f", n))[0], struct.unpack("<f", struct.pack("<f", n))[0])
                    for (c, _w), (a, b, n) in wins.items()]
            assert recs == want, f"zoom level {k}"
        return items, zooms
