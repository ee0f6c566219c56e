"""An independent bigWig reader for the tests (not a test): `struct` and `zlib.decompress` only, no code of deepgrp_amd.  It reads the
file the way a browser does -- header, zoom headers, total summary, chromosome B+ tree (walked, and by key lookup), the data through
the cirTree (a full walk and range queries), every section and every zoom level -- and asserts the container's invariants on the way."""
import struct
import zlib

MAGIC, CIR_MAGIC, BPT_MAGIC = 0x888FFC26, 0x2468ACE0, 0x78CA8C91


class BigWig:
    def __init__(self, data: bytes):
        self.d = data
        (magic, self.version, self.nzoom, self.chrom_at, self.data_at, self.index_at, fc, dfc, autosql, self.summary_at, self.buf_size,
         reserved) = struct.unpack_from("<IHHQQQHHQQIQ", data, 0)
        assert magic == MAGIC and self.version == 4 and fc == 0 and dfc == 0 and autosql == 0 and reserved == 0
        assert struct.unpack_from("<I", data, len(data) - 4)[0] == MAGIC, "trailer"
        assert 0 <= self.nzoom <= 10
        self.zoom_heads = [struct.unpack_from("<IIQQ", data, 64 + 24 * k) for k in range(self.nzoom)]
        assert data[64 + 24 * self.nzoom:64 + 240] == bytes(24 * (10 - self.nzoom))
        self.summary = struct.unpack_from("<Qdddd", data, self.summary_at)
        self.chroms = self._walk_chroms()                       # [(key, id, size)] in key order
        self.section_count = struct.unpack_from("<Q", data, self.data_at)[0]
        self.inflated_max = 0

    # ---- chromosome tree
    def _bpt_head(self):
        magic, bs, ks, vs, n, res = struct.unpack_from("<IIIIQQ", self.d, self.chrom_at)
        assert magic == BPT_MAGIC and vs == 8 and res == 0 and 1 <= bs <= 256 and ks >= 1
        return bs, ks, n

    def _walk_chroms(self):
        bs, ks, n = self._bpt_head()
        out = []

        def node(at, lo):
            leaf, _r, count = struct.unpack_from("<BBH", self.d, at)
            assert count <= bs
            first = None
            for i in range(count):
                p = at + 4 + i * (ks + 8)
                key = self.d[p:p + ks]
                if i == 0:
                    first = key
                if leaf:
                    cid, size = struct.unpack_from("<II", self.d, p + ks)
                    out.append((key.rstrip(b"\0"), cid, size))
                else:
                    child = struct.unpack_from("<Q", self.d, p + ks)[0]
                    assert node(child, key) == key, "an inner key is its child's first key"
            return first
        node(self.chrom_at + 32, None)
        assert len(out) == n
        keys = [k for k, _i, _s in out]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), "sorted, distinct keys"
        assert sorted(i for _k, i, _s in out) == list(range(n))
        return out

    def find_chrom(self, name: bytes):
        """(id, size) by descending the tree, None if absent."""
        bs, ks, _n = self._bpt_head()
        key = name.ljust(ks, b"\0")
        at = self.chrom_at + 32
        while True:
            leaf, _r, count = struct.unpack_from("<BBH", self.d, at)
            items = [(self.d[at + 4 + i * (ks + 8):at + 4 + i * (ks + 8) + ks], at + 4 + i * (ks + 8) + ks) for i in range(count)]
            if leaf:
                for k, p in items:
                    if k == key:
                        return struct.unpack_from("<II", self.d, p)
                return None
            below = [p for k, p in items if k <= key]
            if not below:
                return None
            at = struct.unpack_from("<Q", self.d, below[-1])[0]

    # ---- cirTree
    def _cir_leaves(self, at, query=None):
        """The leaf items (sc, sb, ec, eb, off, size) in tree order; with query = (chrom, beg, end) only those that overlap."""
        magic, bs, n, sc, sb, ec, eb, end_off, per_slot, res = struct.unpack_from("<IIQIIIIQII", self.d, at)
        assert magic == CIR_MAGIC and bs == 256 and per_slot == 1 and res == 0
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
                if leaf:
                    it = struct.unpack_from("<IIIIQQ", self.d, p + 4 + 32 * i)
                else:
                    it = struct.unpack_from("<IIIIQ", self.d, p + 4 + 24 * i)
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

    def _inflate(self, off, size):
        raw = zlib.decompress(self.d[off:off + size])            # (zlib checks the Adler-32)
        assert self.d[off:off + 2] == b"\x78\x01"
        assert len(raw) <= self.buf_size, "uncompressBufSize"
        self.inflated_max = max(self.inflated_max, len(raw))
        return raw

    # ---- data
    @staticmethod
    def _section(raw):
        cid, start, end, step, span, typ, res, count = struct.unpack_from("<IIIIIBBH", raw, 0)
        assert step == 0 and span == 0 and typ == 1 and 1 <= count <= 1024 and len(raw) == 24 + 12 * count
        items = [struct.unpack_from("<IIf", raw, 24 + 12 * i) for i in range(count)]
        assert items[0][0] == start and items[-1][1] == end
        assert all(a[1] <= b[0] for a, b in zip(items, items[1:])) and all(s < e for s, e, _v in items)
        return cid, start, end, items

    def sections(self, query=None):
        leaves, n = self._cir_leaves(self.index_at, query)
        if query is None:
            assert n == self.section_count
            assert all((a[2], a[3]) <= (b[0], b[1]) for a, b in zip(leaves, leaves[1:])), "(chromId, start) order, no overlap"
            at = self.data_at + 8
            for it in leaves:                                    # back to back behind sectionCount
                assert it[4] == at
                at += it[5]
        out = []
        for sc, sb, ec, eb, off, size in leaves:
            cid, start, end, items = self._section(self._inflate(off, size))
            assert (sc, sb, ec, eb) == (cid, start, cid, end)
            out.append((cid, items))
        return out

    def items(self):
        """[(chromId, start, end, value)] of the whole file."""
        return [(cid, s, e, v) for cid, items in self.sections() for s, e, v in items]

    def query(self, chrom_id, beg, end):
        return [(cid, s, e, v) for cid, items in self.sections((chrom_id, beg, end)) for s, e, v in items if s < end and e > beg]

    def zoom(self, k):
        """(reduction, [(chromId, start, end, valid, min, max, sum, sumsq)]) of zoom level k."""
        red, res, data_at, index_at = self.zoom_heads[k]
        assert res == 0
        count = struct.unpack_from("<I", self.d, data_at)[0]
        leaves, _n = self._cir_leaves(index_at)
        out = []
        at = data_at + 4
        for sc, sb, ec, eb, off, size in leaves:
            assert off == at
            at += size
            raw = self._inflate(off, size)
            assert len(raw) % 32 == 0 and 1 <= len(raw) // 32 <= 1024
            recs = [struct.unpack_from("<IIIIffff", raw, 32 * i) for i in range(len(raw) // 32)]
            assert (sc, sb) == recs[0][:2] and (ec, eb) == (recs[-1][0], recs[-1][2])
            out.extend(recs)
        assert at == index_at and len(out) == count
        assert all((a[0], a[2]) <= (b[0], b[1]) for a, b in zip(out, out[1:]))
        return red, out

    def check_all(self):
        """Everything once: -> (items, [zoom levels])."""
        items = self.items()
        zooms = [self.zoom(k) for k in range(self.nzoom)]
        assert self.buf_size == self.inflated_max, "uncompressBufSize is the largest block"
        return items, zooms
