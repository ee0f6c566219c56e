"""The three device entries of --track_bigwig, bit for bit: dgrp_track_sections_batch against bigwig.reference_items, dgrp_track_zoom_batch
against a numpy restatement of the zoom rule, dgrp_zlib_compress_batch against the host entry and zlib.decompress; the capacity
protocol with guards behind the buffers; the stream contract of the three (stream_harness.py)."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import FILLS, Harness, i64ptr      # noqa: E402

NCLASS, DIGITS, CHROM0 = 5, 2, 7
CLASSES = (1, 3, 4, 2)                                  # column 4 is zero everywhere: a class without a section or a zoom record
LEVELS = 10


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def pipe_dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _case(width):
    """Records where the chain can go wrong, for one bin width: (lengths, start positions, row0, probs [rows, 5])."""
    b = width
    n = np.array([1, 777, 1024 * b, 1025 * b, 300, 18_000 * b], np.int64)   # (the last: more than 1024 windows of 16 bins)
    spos = np.array([0, 13, 3 * b, 0, 5, 2 * b + (b > 1)], np.int64)
    row0 = np.r_[0, np.cumsum((n[:-1] + 63) // 64 * 64)].astype(np.int64)
    rng = np.random.default_rng(width)
    p = (rng.integers(0, 5, (int(row0[-1] + n[-1]), NCLASS)) / 4).astype(np.float32)
    p[:, 4] = 0
    for r in (2, 3):                                    # every bin an item of its own: exactly 1024 and 1025 items in class 1
        bins = np.arange(n[r]) // b
        p[row0[r]:row0[r] + n[r], 1] = np.where(bins % 2 == 0, 0.25, 0.5)
    p[row0[4]:row0[4] + n[4], :] = 0                    # a record without an item
    a = row0[5]
    p[a:a + n[5], 3] = 0
    p[a + 100 * b:a + 4500 * b, 3] = 0.5                # one item across a 2048-bin tile border and many R_0 and R_1 windows
    p[a + 4600 * b, 3] = 1.0
    return n, spos, row0, p


def _bins(col, sp, width):
    """Per bin of one record's class column: (q, lo, hi)."""
    from deepgrp_amd.tracks import quantise
    pos = np.arange(sp, sp + col.size, dtype=np.int64)
    cut = np.flatnonzero(np.diff(pos // width)) + 1
    first = np.r_[0, cut]
    q = quantise(np.maximum(np.maximum.reduceat(col, first), np.float32(0)), DIGITS)
    return q, pos[first], np.r_[pos[cut], sp + col.size]


def _zoom_reference(col, sp, width, chrom):
    """The zoom rule in numpy: per level the records of one record's class column, and its integer totals."""
    q, lo, hi = _bins(col, sp, width)
    keep = q != 0
    q, lo, hi = q[keep], lo[keep], hi[keep]
    bases = hi - lo
    scale = np.float64(10 ** DIGITS)
    out = []
    rec = np.dtype([("c", "<u4"), ("s", "<u4"), ("e", "<u4"), ("n", "<u4"), ("min", "<f4"), ("max", "<f4"), ("sum", "<f4"), ("sq", "<f4")])
    for k in range(LEVELS):
        win = lo // (16 * width * 4 ** k)                                  # (ascending: the bins are)
        a = np.flatnonzero(np.r_[True, np.diff(win) != 0]) if q.size else np.zeros(0, np.int64)
        z = np.zeros(a.size, rec)
        if a.size:
            last = np.r_[a[1:], q.size] - 1
            f = lambda x, d=scale: (x.astype(np.float64) / d).astype(np.float32)
            z["c"], z["s"], z["e"], z["n"] = chrom, lo[a], hi[last], np.add.reduceat(bases, a)
            z["min"], z["max"] = f(np.minimum.reduceat(q, a)), f(np.maximum.reduceat(q, a))
            z["sum"], z["sq"] = f(np.add.reduceat(q * bases, a)), f(np.add.reduceat(q * q * bases, a), scale * scale)
        out.append([z[i:i + 1].tobytes() for i in range(a.size)])
    tot = (int(bases.sum()), int(q.min()) if q.size else 0, int(q.max()) if q.size else 0, int((q * bases).sum()), int((q * q * bases).sum()))
    return out, tot


@pytest.fixture(scope="module", params=[1, 50, 65], ids=lambda w: f"bin{w}")
def case(request, pipe_dev):
    """One bin width: the inputs, the device results of both track entries, and their references (computed once)."""
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd.pipeline import ContigPipeline
    width = request.param
    n, spos, row0, p = _case(width)
    d_p = torch.from_numpy(p).to(pipe_dev)
    args = (d_p, row0, n, spos, CLASSES, DIGITS, width, CHROM0)
    sec = ContigPipeline.track_sections_batch_device(None, *args)
    zoom = ContigPipeline.track_zoom_batch_device(None, *args)
    want_sec, want_rows = [], []
    for c in CLASSES:
        blocks, rows = [], []
        for r in range(len(n)):
            s, e, q = bw.reference_items(p[row0[r]:row0[r] + n[r], c], int(spos[r]), DIGITS, width)
            for a, raw in zip(range(0, len(s), 1024), bw.section_bytes(CHROM0 + r, s, e, q, DIGITS)):
                blocks.append(raw)
                rows.append((len(raw), r, int(s[a]), int(e[min(a + 1024, len(s)) - 1])))
        want_sec.append(blocks)
        want_rows.append(rows)
    return dict(width=width, n=n, spos=spos, row0=row0, p=p, d_p=d_p, sec=sec, zoom=zoom, want_sec=want_sec, want_rows=want_rows)


def test_sections_are_the_reference_items_bit_for_bit(case):
    from deepgrp_amd import bigwig as bw
    d_out, off, d_tab, soff = case["sec"]
    out, tab = d_out.cpu().numpy().tobytes(), d_tab.cpu().numpy().view(bw.SECTION_DTYPE)
    for k, (blocks, rows) in enumerate(zip(case["want_sec"], case["want_rows"])):
        assert out[off[k]:off[k + 1]] == b"".join(blocks), (case["width"], CLASSES[k])
        t = tab[soff[k]:soff[k + 1]]
        assert len(t) == len(rows)
        at = int(off[k])
        for row, (nbytes, r, s, e) in zip(t, rows):
            assert (row["off"], row["bytes"], row["rec"], row["start"], row["end"], row["pad"]) == (at, nbytes, r, s, e, 0)
            at += nbytes
    k1 = CLASSES.index(1)
    counts = [[struct.unpack_from("<H", b, 22)[0] for b in case["want_sec"][k1] if struct.unpack_from("<I", b, 0)[0] == CHROM0 + r] for r in (2, 3)]
    assert counts == [[1024], [1024, 1]]                                   # the section cut
    assert off[CLASSES.index(4)] == off[CLASSES.index(4) + 1] and case["want_sec"][CLASSES.index(4)] == []
    assert all(CHROM0 + 4 not in {struct.unpack_from("<I", b, 0)[0] for b in blocks} for blocks in case["want_sec"])
    b, r = case["width"], 5                                                # the long run is ONE item, tiles and windows notwithstanding
    s, e, _q = bw.reference_items(case["p"][case["row0"][r]:case["row0"][r] + case["n"][r], 3], int(case["spos"][r]), DIGITS, b)
    assert ((e - s) >= 4400 * b).sum() == 1 and (e - s).max() // b > 2048


def test_zoom_records_are_the_numpy_rule_bit_for_bit(case):
    from deepgrp_amd import bigwig as bw
    d_out, roff, d_tab, boff, totals = case["zoom"]
    out, tab = d_out.cpu().numpy().tobytes(), d_tab.cpu().numpy().view(bw.ZOOM_BLOCK_DTYPE)
    n, spos, row0, p, width = (case[x] for x in ("n", "spos", "row0", "p", "width"))
    seen_levels = 0
    for k, c in enumerate(CLASSES):
        per = [_zoom_reference(p[row0[r]:row0[r] + n[r], c], int(spos[r]), width, CHROM0 + r) for r in range(len(n))]
        tots = [t for _z, t in per if t[0]]
        want_tot = (sum(t[0] for t in tots), min([t[1] for t in tots], default=0), max([t[2] for t in tots], default=0),
                    sum(t[3] for t in tots), sum(t[4] for t in tots))
        assert tuple(int(x) for x in totals[k]) == want_tot, (width, c)
        for lv in range(LEVELS):
            s = k * LEVELS + lv
            recs = [x for z, _t in per for x in z[lv]]
            assert out[32 * roff[s]:32 * roff[s + 1]] == b"".join(recs), (width, c, lv)
            t = tab[boff[s]:boff[s + 1]]
            assert len(t) == (len(recs) + 1023) // 1024
            for j, row in enumerate(t):
                blk = recs[1024 * j:1024 * (j + 1)]
                f, l = struct.unpack_from("<III", blk[0], 0), struct.unpack_from("<III", blk[-1], 0)
                assert (row["off"], row["bytes"], row["cls"], row["level"]) == (32 * (roff[s] + 1024 * j), 32 * len(blk), k, lv)
                assert (row["rec0"], row["start"], row["rec1"], row["end"]) == (f[0] - CHROM0, f[1], l[0] - CHROM0, l[2])
            seen_levels += len(recs) > 0
    assert seen_levels == 3 * LEVELS and roff[CLASSES.index(4) * LEVELS] == roff[(CLASSES.index(4) + 1) * LEVELS]
    if width == 1:
        assert boff[1] - boff[0] > 1                                        # more than one block in a level


def _raw_call(L, entry, case, cap, tcap, out, table, work):
    n, spos, row0 = case["n"], case["spos"], case["row0"]
    cl = np.array(CLASSES, np.int32)
    nseg = len(CLASSES) * (LEVELS if entry == "zoom" else 1)
    a, b = np.full(nseg + 1, -1, np.int64), np.full(nseg + 1, -1, np.int64)
    common = (case["d_p"].data_ptr(), NCLASS, len(n), row0.ctypes.data, n.ctypes.data, spos.ctypes.data, cl.ctypes.data, len(cl), DIGITS, case["width"],
              CHROM0, out.data_ptr(), cap, a.ctypes.data, table.data_ptr(), tcap, b.ctypes.data)
    if entry == "sections":
        rc = L.dgrp_track_sections_batch(*common, work.data_ptr(), work.numel(), None)
    else:
        tot = np.zeros(5 * len(cl), np.uint64)
        rc = L.dgrp_track_zoom_batch(*common, tot.ctypes.data, work.data_ptr(), work.numel(), None)
    torch.cuda.synchronize()
    return rc, a, b


@pytest.mark.parametrize("entry", ["sections", "zoom"])
def test_capacity_protocol_with_guards(L, case, pipe_dev, entry):
    """Too little room for the bytes, or for the table: the offsets are filled in full and nothing is written; exactly enough: the
    bytes behind both buffers stay as they were."""
    from deepgrp_amd import bigwig as bw
    if entry == "sections":
        d_out, off, d_tab, toff = case["sec"]
        row, need = bw.SECTION_DTYPE.itemsize, int(off[-1])
        query = L.dgrp_track_sections_workspace_bytes
    else:
        d_out, roff, d_tab, toff, _tot = case["zoom"]
        off, row, need = roff, bw.ZOOM_BLOCK_DTYPE.itemsize, 32 * int(roff[-1])
        query = L.dgrp_track_zoom_workspace_bytes
    nrows, guard = int(toff[-1]), 4096
    n, spos = case["n"], case["spos"]
    wb = query(len(n), n.ctypes.data, spos.ctypes.data, case["width"], len(CLASSES))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=pipe_dev)
    for cap, tcap, written in ((need - 1, nrows, False), (need, nrows - 1, False), (0, 0, False), (need, nrows, True)):
        out = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=pipe_dev)
        table = torch.full((nrows * row + guard,), 0x5A, dtype=torch.uint8, device=pipe_dev)
        rc, a, b = _raw_call(L, entry, case, cap, tcap, out, table, work)
        assert rc == 0 and a.tolist() == list(off) and b.tolist() == list(toff)
        got, gtab = out.cpu().numpy(), table.cpu().numpy()
        if written:
            assert got[:need].tobytes() == d_out.cpu().numpy().tobytes() and gtab[:nrows * row].tobytes() == d_tab.cpu().numpy().tobytes()
            assert (got[need:] == 0x5A).all() and (gtab[nrows * row:] == 0x5A).all()
        else:
            assert (got == 0x5A).all() and (gtab == 0x5A).all()
    small = torch.empty(wb - 1, dtype=torch.uint8, device=pipe_dev)
    rc, _a, _b = _raw_call(L, entry, case, need, nrows, out, table, small)
    assert rc == -3


@pytest.mark.parametrize("level", [0, 1])
def test_zlib_device_bytes_are_the_host_bytes(case, level):
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd.pipeline import ContigPipeline
    for d_in, d_tab, dt in ((case["sec"][0], case["sec"][2], bw.SECTION_DTYPE), (case["zoom"][0], case["zoom"][2], bw.ZOOM_BLOCK_DTYPE)):
        tab = d_tab.cpu().numpy().view(dt)
        data = d_in.cpu().numpy().tobytes()
        d_out, d_sizes = ContigPipeline.zlib_compress_device(d_in, d_tab, dt.itemsize, level)
        blob, sizes = d_out.cpu().numpy().tobytes(), d_sizes.cpu().numpy()
        want, want_sizes = bw.zlib_compress_host(data, tab["off"], tab["bytes"], level)
        assert sizes.tolist() == want_sizes.tolist() and blob == want
        at = 0
        for o, nb, s in zip(tab["off"], tab["bytes"], sizes):
            assert zlib.decompress(blob[at:at + s]) == data[o:o + nb] and s <= nb + 11
            at += s
        assert len(tab) > 3


def test_zlib_device_edge_blocks_and_a_refused_row(L, pipe_dev):
    """Blocks of 0, 1 and 0xff00 bytes, all 0xff (the byte sum passes 65521 many times), overlapping and unaligned; a row outside
    the input is refused and nothing is written."""
    from deepgrp_amd import bigwig as bw
    from deepgrp_amd.pipeline import ContigPipeline
    rng = np.random.default_rng(3)
    data = np.r_[np.full(0xff00, 0xff, np.uint8), rng.integers(0, 256, 70_000).astype(np.uint8), np.zeros(0xff00, np.uint8)]
    rows = np.array([[0, 0xff00], [5, 0], [0xff00 + 3, 1], [0xff00 + 1, 0xff00], [len(data) - 0xff00, 0xff00], [1, 0xfeff], [0xff00 - 7, 33]], np.int64)
    d_in, d_rows = torch.from_numpy(data).to(pipe_dev), torch.from_numpy(rows).to(pipe_dev).view(torch.uint8).reshape(-1)
    for level in (0, 1):
        d_out, d_sizes = ContigPipeline.zlib_compress_device(d_in, d_rows, 16, level)
        blob, sizes = d_out.cpu().numpy().tobytes(), d_sizes.cpu().numpy()
        want, want_sizes = bw.zlib_compress_host(data.tobytes(), rows[:, 0], rows[:, 1], level)
        assert blob == want and sizes.tolist() == want_sizes.tolist()
        at = 0
        for (o, nb), s in zip(rows, sizes):
            assert zlib.decompress(blob[at:at + s]) == data[o:o + nb].tobytes()
            at += s
    bad = rows.copy()
    bad[2] = (len(data) - 3, 4)
    d_bad = torch.from_numpy(bad).to(pipe_dev).view(torch.uint8).reshape(-1)
    out = torch.full((1 << 18,), 0x5A, dtype=torch.uint8, device=pipe_dev)
    sizes = torch.full((len(bad),), -5, dtype=torch.int64, device=pipe_dev)
    wb = L.dgrp_zlib_workspace_bytes(len(bad), 1)
    work = torch.empty(wb, dtype=torch.uint8, device=pipe_dev)
    got = C.c_int64(-1)
    rc = L.dgrp_zlib_compress_batch(d_in.data_ptr(), len(data), d_bad.data_ptr(), 16, len(bad), 1, out.data_ptr(), 1 << 18, sizes.data_ptr(), C.byref(got),
                                    work.data_ptr(), wb, None)
    assert rc == -1 and b"1 rows do not lie in the input" in L.dgrp_last_error()
    assert (out.cpu().numpy() == 0x5A).all() and (sizes.cpu().numpy() == -5).all()
    rc = L.dgrp_zlib_compress_batch(d_in.data_ptr(), len(data), d_rows.data_ptr(), 16, len(rows), 1, out.data_ptr(), 100, sizes.data_ptr(), C.byref(got),
                                    work.data_ptr(), wb, None)
    assert rc == -3 and got.value > 100 and (out.cpu().numpy() == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def H(L, pipe_dev):
    h = Harness(pipe_dev)
    h.choose_side(L)
    return h


@pytest.mark.parametrize("entry", ["sections", "zoom"])
@pytest.mark.parametrize("fill", FILLS[:2], ids=lambda f: f"fill{f:02X}")
def test_sync_track_entries_honour_the_stream(H, L, entry, fill):
    from deepgrp_amd import bigwig as bw
    width = 7
    n = np.array([1, 65, 4097], np.int64)
    spos = np.array([0, 3, 123], np.int64)
    row0 = np.r_[0, np.cumsum((n[:-1] + 63) // 64 * 64)].astype(np.int64)
    rows = int(row0[-1] + n[-1])
    cls = np.array([0, 3], np.int32)
    rng = np.random.default_rng(11)
    real, poison = ((rng.integers(0, 5, (rows, NCLASS)) / 4).astype(np.float32) for _ in range(2))
    cap, tcap = 1 << 17, 64
    row = (bw.SECTION_DTYPE if entry == "sections" else bw.ZOOM_BLOCK_DTYPE).itemsize
    nseg = len(cls) * (LEVELS if entry == "zoom" else 1)
    q = L.dgrp_track_sections_workspace_bytes if entry == "sections" else L.dgrp_track_zoom_workspace_bytes
    wb = q(len(n), n.ctypes.data, spos.ctypes.data, width, len(cls))

    def call(b, wk, st, t):
        a, c = np.full(nseg + 1, -1, np.int64), np.full(nseg + 1, -1, np.int64)
        common = (b["p"].data_ptr(), NCLASS, len(n), i64ptr(t["row0"]), i64ptr(t["n"]), i64ptr(t["spos"]), t["cls"].ctypes.data, len(cls), DIGITS, width, 0,
                  b["out"].data_ptr(), cap, a.ctypes.data, b["table"].data_ptr(), tcap, c.ctypes.data)
        if entry == "sections":
            rc = L.dgrp_track_sections_batch(*common, wk.data_ptr(), wb, st)
            return rc, (a.tolist(), c.tolist())
        tot = np.zeros(5 * len(cls), np.uint64)
        rc = L.dgrp_track_zoom_batch(*common, tot.ctypes.data, wk.data_ptr(), wb, st)
        return rc, (a.tolist(), c.tolist(), tot.tolist())
    late, host, _idle, host_idle = H.run(call, {"p": (real, poison)}, {"out": np.full(cap, 0x5A, np.uint8), "table": np.full(tcap * row, 0x5A, np.uint8)},
                                         work_bytes=wb, fill=fill, sync=True, tables={"row0": row0, "n": n.copy(), "spos": spos, "cls": cls})
    assert host == host_idle
    if entry == "sections":
        want = b"".join(raw for c in cls for r in range(len(n))
                        for raw in bw.section_bytes(r, *bw.reference_items(real[row0[r]:row0[r] + n[r], c], int(spos[r]), DIGITS, width), DIGITS))
        assert host[0][-1] == len(want) > 1000 and late["out"][:len(want)].tobytes() == want and (late["out"][len(want):] == 0x5A).all()
    else:
        want = b"".join(x for c in cls for lv in range(LEVELS) for r in range(len(n))
                        for x in _zoom_reference(real[row0[r]:row0[r] + n[r], c], int(spos[r]), width, r)[0][lv])
        assert 32 * host[0][-1] == len(want) > 1000 and late["out"][:len(want)].tobytes() == want and (late["out"][len(want):] == 0x5A).all()


@pytest.mark.parametrize("level", [0, 1])
def test_sync_zlib_compress_honours_the_stream(H, L, level):
    from deepgrp_amd import bigwig as bw
    rng = np.random.default_rng(5)
    real = np.repeat(rng.integers(0, 8, 40_000), 5).astype(np.uint8)
    poison = rng.integers(0, 256, real.size).astype(np.uint8)
    rows = np.array([[0, 0xff00], [0xff00, 12_345], [100_000, 0], [150_000, 50_000]], np.int64)
    prow = np.array([[7, 100], [0, 0], [5, 5], [9, 1000]], np.int64)
    cap = int(L.dgrp_zlib_bound(len(rows), real.size))
    wb = int(L.dgrp_zlib_workspace_bytes(len(rows), level))

    def call(b, wk, st, t):
        got = C.c_int64(-1)
        rc = L.dgrp_zlib_compress_batch(b["in"].data_ptr(), real.size, b["rows"].data_ptr(), 16, len(rows), level, b["out"].data_ptr(), cap,
                                        b["sizes"].data_ptr(), C.byref(got), wk.data_ptr(), wb, st)
        return rc, got.value
    late, total, _idle, total_idle = H.run(call, {"in": (real, poison), "rows": (rows, prow)},
                                           {"out": np.full(cap, 0x5A, np.uint8), "sizes": np.full(len(rows), -3, np.int64)}, work_bytes=wb,
                                           fill=FILLS[level], sync=True)
    want, sizes = bw.zlib_compress_host(real.tobytes(), rows[:, 0], rows[:, 1], level)
    assert total == total_idle == len(want) and late["out"][:total].tobytes() == want and (late["out"][total:] == 0x5A).all()
    assert late["sizes"].tolist() == sizes.tolist()
