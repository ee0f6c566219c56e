"""Plain gzip on the GPU: dgrp_inflate_stream_scan / _write against zlib over the corpus of test_inflate_stream_host.py, with the
statistics of the host entry (the chain is the same code, so they are equal, not close), sentinels around every buffer, a
non-default stream; then the ingest on one-member gzip files with the device path switched on, and the files it must hand to zlib."""
import ctypes as C
import gzip
import logging
import os
import struct
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_stream_cases as gc                          # noqa: E402
import inflate_cases as ic                              # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 512
HEAD = b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"            # what stands in front of the stream in a gzip member
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")


def _guarded(nbytes, dev, fill=0xa5):
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + GUARD


def _intact(buf, nbytes, fill=0xa5):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + nbytes:] == fill).all())


def host_stats(comp, chunk, cap, max_span, max_rounds):
    from deepgrp_amd._lib import InflateStreamStats, lib
    out = (C.c_uint8 * max(cap, 1))()
    ol, iu, r, st = C.c_int64(), C.c_int64(), C.c_int(), InflateStreamStats()
    rc = lib().dgrp_inflate_stream_host(comp, len(comp), chunk, max_span, max_rounds, out, cap, C.byref(ol), C.byref(iu), C.byref(st), C.byref(r))
    return rc, r.value, st.as_dict()


def device_inflate(comp, chunk, max_span=gc.MAX_SPAN, max_rounds=gc.MAX_ROUNDS, stream=None, tail=b"\xee" * 8):
    """scan and write on `HEAD + comp + tail` (8 trailer bytes) -> (rc, reason, text, crc, in_used, statistics); every buffer
    between sentinels that must survive"""
    from deepgrp_amd._lib import InflateStreamStats, lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    file = HEAD + comp + tail
    d_in = torch.frombuffer(bytearray(file), dtype=torch.uint8).to(dev)
    wb = int(L.dgrp_inflate_stream_workspace_bytes(len(file), chunk))
    assert wb > 0 and wb % 256 == 0
    work, p_work = _guarded(wb, dev)
    total, st, reason = C.c_int64(-1), InflateStreamStats(), C.c_int(-1)
    sp = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
    rc = L.dgrp_inflate_stream_scan(d_in.data_ptr(), len(file), len(HEAD), chunk, max_span, max_rounds, C.byref(total), C.byref(st),
                                    C.byref(reason), p_work, wb, sp)
    assert _intact(work, wb)
    if rc != 0:
        return rc, reason.value, None, None, None, st.as_dict()
    n = int(total.value)
    out, p_out = _guarded(n, dev)
    sym, p_sym = _guarded(2 * n, dev, 0x5a)
    crc, used = C.c_uint32(0), C.c_int64(-1)
    rc = L.dgrp_inflate_stream_write(d_in.data_ptr(), len(file), len(HEAD), chunk, p_sym, p_out, n, C.byref(crc), C.byref(used), C.byref(reason),
                                     p_work, wb, sp)
    assert _intact(work, wb) and _intact(out, n) and _intact(sym, 2 * n, 0x5a)
    assert bytes(d_in.cpu().numpy()) == file
    text = out[GUARD:GUARD + n].cpu().numpy().tobytes() if rc == 0 else None
    return rc, reason.value, text, crc.value, used.value, st.as_dict()


@pytest.mark.parametrize("chunk", [4 << 10, 32 << 10])
@pytest.mark.parametrize("name", sorted(gc.corpus()))
def test_scan_and_write_equal_zlib_and_the_host_entry(name, chunk):
    comp, want = gc.corpus()[name]
    rc, reason, got, crc, used, st = device_inflate(comp, chunk)
    assert (rc, reason) == (0, 0)
    assert got == want and crc == zlib.crc32(want) and used == len(HEAD) + len(comp)
    hrc, hreason, hst = host_stats(comp, chunk, len(want), gc.MAX_SPAN, gc.MAX_ROUNDS)
    assert (hrc, hreason) == (0, 0) and st == hst
    if chunk == 4 << 10 and len(comp) > 4 * chunk and hst["candidates"]:
        assert st["spans"] > 1


def test_the_false_start_is_repaired_on_the_device_too():
    fs = gc.FALSE_START
    text = gc.fasta_text(fs["seed"], fs["nbases"])
    comp = gc.deflate(text, 1)
    rc, reason, got, crc, used, st = device_inflate(comp, fs["chunk"])
    assert (rc, reason) == (0, 0) and got == text and st["false_starts"] >= 1
    assert st == host_stats(comp, fs["chunk"], len(text), gc.MAX_SPAN, gc.MAX_ROUNDS)[2]


def test_refusals_carry_the_reason_of_the_host_entry():
    data = gc.texts()["fasta"][:200_000]
    for comp, kw in ((gc.deflate(data, 6, zlib.Z_FIXED), dict(max_span=4096)), (gc.corpus()["half-l6"][0], dict(max_rounds=3)),
                     (gc.corpus()["fasta-l6"][0][:200_000], {})):
        rc, reason, _, _, _, st = device_inflate(comp, 4 << 10, **kw)
        hrc, hreason, hst = host_stats(comp, 4 << 10, 4_000_000, kw.get("max_span", gc.MAX_SPAN), kw.get("max_rounds", gc.MAX_ROUNDS))
        assert (rc, reason) == (hrc, hreason) and rc == -5 and reason in (1, 11, 12)


CORE_CASES = [c for c in ic.CORRUPT if c[0] not in ("stored_over_cap", "output_over_cap")]


@pytest.mark.parametrize("chunk", [64, 1024])
@pytest.mark.parametrize("name,comp", [c[:2] for c in CORE_CASES], ids=[c[0] for c in CORE_CASES])
def test_corrupt_corpus_of_the_decode_core_equals_the_host_entry(name, comp, chunk):
    """The corrupt corpus of the decode core (tests/inflate_cases.py: the fixed-reason cases whose reason needs no output cap, the
    flipped and the random streams) as a stream that ends where the file ends: scan and write give the return code and reason of
    dgrp_inflate_stream_host, and its text and input bytes used where it decodes.  The yardstick is the stream host entry, not
    dgrp_inflate_raw_host: both refuse the same streams, but on inflate_cases.HOST_ENTRIES_DIFFER (five random streams, at both
    chunk sizes) with different reasons -- the span path's counting pass decodes the whole stream and meets a later error before
    the window walk can report the bad distance the serial decoder stops at (test_inflate_cases_host.py holds that list to the
    two host entries)."""
    hrc, hreason, htext, hused = ic.stream_host(comp, chunk, 1 << 20, gc.MAX_SPAN, gc.MAX_ROUNDS)
    assert (hrc, hreason) != (-5, ic.EOUTPUT)                                # the cap of the host entry plays no part
    rc, reason, text, crc, used, _st = device_inflate(comp, chunk, tail=b"")
    assert (rc, reason) == (hrc, hreason)
    if hrc == 0:
        assert ic.zlib_says(comp) == (htext, hused)
        assert text == htext and used == len(HEAD) + hused and crc == zlib.crc32(htext)
    else:
        assert rc == -5 and reason > 0 and text is None


def test_write_refuses_a_workspace_without_the_chain():
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp, want = gc.corpus()["hand_run"]
    d_in = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    wb = int(L.dgrp_inflate_stream_workspace_bytes(len(comp), 4096))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    out = torch.full((len(want),), 7, dtype=torch.uint8, device=dev)
    sym = torch.zeros(len(want), dtype=torch.int16, device=dev)
    crc, used, reason = C.c_uint32(), C.c_int64(), C.c_int()
    sp = torch.cuda.current_stream().cuda_stream
    assert L.dgrp_inflate_stream_write(d_in.data_ptr(), len(comp), 0, 4096, sym.data_ptr(), out.data_ptr(), len(want), C.byref(crc),
                                       C.byref(used), C.byref(reason), work.data_ptr(), wb, sp) == -1
    assert "no chain" in L.dgrp_last_error().decode() and bool((out == 7).all())


def test_eight_megabytes_at_the_shipped_constants_on_a_side_stream():
    from deepgrp_amd import gz
    text = gc.fasta_text(5, 8_000_000)
    comp = gc.deflate(text, 6)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc, reason, got, crc, used, st = device_inflate(comp, gz.PLAIN_CHUNK_BYTES, gz.PLAIN_MAX_SPAN_BYTES, gz.PLAIN_MAX_ROUNDS, stream=side)
    assert (rc, reason) == (0, 0) and got == text and crc == zlib.crc32(text)
    assert st == host_stats(comp, gz.PLAIN_CHUNK_BYTES, len(text), gz.PLAIN_MAX_SPAN_BYTES, gz.PLAIN_MAX_ROUNDS)[2]
    assert st["spans"] > 20


def test_text_beyond_two_gib():
    """2.3 GB of text from a 5 MB stream (a run: every symbol behind the first span is a marker): output offsets, symbol and byte
    indices above 2^31.  The text stays on the device; it is all `N`, and its CRC-32 is zlib's."""
    from deepgrp_amd import gz
    from deepgrp_amd._lib import InflateStreamStats, lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    comp, n = gc.hand_big_run(1120)
    assert n > (1 << 31) + (1 << 27)
    d_in = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    wb = int(L.dgrp_inflate_stream_workspace_bytes(len(comp), gz.PLAIN_CHUNK_BYTES))
    work, p_work = _guarded(wb, dev)
    total, st, reason = C.c_int64(-1), InflateStreamStats(), C.c_int(-1)
    sp = torch.cuda.current_stream().cuda_stream
    assert L.dgrp_inflate_stream_scan(d_in.data_ptr(), len(comp), 0, gz.PLAIN_CHUNK_BYTES, gz.PLAIN_MAX_SPAN_BYTES, gz.PLAIN_MAX_ROUNDS,
                                      C.byref(total), C.byref(st), C.byref(reason), p_work, wb, sp) == 0
    assert total.value == n and st.spans > 300
    out, p_out = _guarded(n, dev)
    sym, p_sym = _guarded(2 * n, dev, 0x5a)
    crc, used = C.c_uint32(0), C.c_int64(-1)
    assert L.dgrp_inflate_stream_write(d_in.data_ptr(), len(comp), 0, gz.PLAIN_CHUNK_BYTES, p_sym, p_out, n, C.byref(crc), C.byref(used),
                                       C.byref(reason), p_work, wb, sp) == 0
    assert _intact(work, wb) and _intact(out, n) and _intact(sym, 2 * n, 0x5a)
    text = out[GUARD:GUARD + n]
    assert int(text.min()) == ord("N") == int(text.max()) and used.value == len(comp)
    want, block = 0, b"N" * (1 << 26)
    for o in range(0, n, len(block)):
        want = zlib.crc32(block[:min(len(block), n - o)], want)
    assert crc.value == want


# ------------------------------------------------------------------------------------------------------------------ ingest
def _cli_fasta(rng) -> bytes:
    seq = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    parts = []
    for k, n in enumerate((50_000, 40, 25_000, 80_000)):
        s = "NN" + seq(n) + "N"
        parts.append(b">chr%d\n" % (k + 1) + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode() + b"\n")
    return b"".join(parts)


def _member(data: bytes, name: bytes = b"x.fa", level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    """One gzip member with FNAME and an mtime, as `gzip x.fa` writes it."""
    head = b"\x1f\x8b\x08\x08" + struct.pack("<I", 1_700_000_000) + b"\x00\x03" + name + b"\0"
    return head + gc.deflate(data, level, strategy) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def _records(path):
    from deepgrp_amd.fasta import DeviceRecord, read_multi_fasta_device
    out = []
    for header, rec in read_multi_fasta_device(str(path)):
        if isinstance(rec, DeviceRecord):
            out.append((header, "dev", rec.startpos, rec.length, rec.d_idx.cpu().numpy().tobytes() if rec.length > 0 else b""))
        else:
            out.append((header, "str", rec))
    return out


@pytest.fixture
def device_path(monkeypatch):
    from deepgrp_amd import gz
    monkeypatch.setattr(gz, "PLAIN_DEVICE_MIN_BYTES", 0)
    monkeypatch.setattr(gz, "PLAIN_CHUNK_BYTES", 4 << 10)              # several spans in files of this size
    return gz


def _log_lines(caplog):
    return [r.getMessage() for r in caplog.records if r.name == "deepgrp_amd.gz"]


def test_read_multi_fasta_device_on_plain_gzip(tmp_path, device_path, caplog):
    data = _cli_fasta(np.random.default_rng(8)) + gc.texts()["fasta"][:300_000]
    fa, fz = tmp_path / "x.fa", tmp_path / "x.fa.gz"
    fa.write_bytes(data)
    fz.write_bytes(gzip.compress(data, 6, mtime=1_700_000_000))
    fn = tmp_path / "named.fa.gz"
    fn.write_bytes(_member(data))
    want = _records(fa)
    with caplog.at_level(logging.INFO, logger="deepgrp_amd.gz"):
        assert _records(fz) == want and _records(fn) == want
    lines = _log_lines(caplog)
    assert len(lines) == 2 and all("inflated on the device" in l and "spans" in l for l in lines)


def test_predict_and_mask_gzip_on_plain_gzip(tmp_path, device_path, caplog):
    from deepgrp_amd.__main__ import main
    data = _cli_fasta(np.random.default_rng(3))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    fa, fz = tmp_path / "a" / "in.fa", tmp_path / "b" / "in.fa.gz"
    fa.write_bytes(data)
    fz.write_bytes(_member(data, b"in.fa"))
    flags = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
    main(flags + ["predict", MODEL, str(fa), "--output", str(tmp_path / "plain.tsv"), "--mask_dir", str(tmp_path / "ma"), "--mask_gzip"])
    with caplog.at_level(logging.INFO, logger="deepgrp_amd.gz"):
        main(flags + ["predict", MODEL, str(fz), "--output", str(tmp_path / "gz.tsv"), "--mask_dir", str(tmp_path / "mb"), "--mask_gzip"])
    plain = (tmp_path / "plain.tsv").read_text()
    assert plain.count("\n") > 3 and (tmp_path / "gz.tsv").read_text().replace(str(fz), str(fa)) == plain
    masked = gzip.decompress((tmp_path / "ma" / "in.fa.gz").read_bytes())
    assert masked != data and masked.upper() == data.upper()
    assert gzip.decompress((tmp_path / "mb" / "in.fa.gz").read_bytes()) == masked
    lines = _log_lines(caplog)
    assert len(lines) >= 2 and all("inflated on the device" in l for l in lines)          # the ingest and the second walk


@pytest.mark.parametrize("form,why", [("two_members", "more than one member"), ("fixed", "scan: a span longer than")])
def test_fallbacks_take_the_host_path_and_say_why(tmp_path, device_path, monkeypatch, caplog, form, why):
    data = _cli_fasta(np.random.default_rng(5))
    fa, fz = tmp_path / "x.fa", tmp_path / "x.fa.gz"
    fa.write_bytes(data)
    if form == "two_members":
        fz.write_bytes(_member(data[:100_000]) + _member(data[100_000:]))
    else:
        monkeypatch.setattr(device_path, "PLAIN_MAX_SPAN_BYTES", 16 << 10)   # one span of 45 KB: one wave's serial work
        fz.write_bytes(_member(data, strategy=zlib.Z_FIXED))
    with caplog.at_level(logging.INFO, logger="deepgrp_amd.gz"):
        assert _records(fz) == _records(fa)
    lines = _log_lines(caplog)
    assert len(lines) == 1 and "inflated on the host with zlib" in lines[0] and why in lines[0]


def test_flipped_crc_raises_todays_error_then_predict_succeeds(tmp_path, device_path, caplog):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.fasta import read_multi_fasta_device
    data = _cli_fasta(np.random.default_rng(4))
    good = _member(data)
    bad = bytearray(good)
    bad[-6] ^= 0x40                                                        # a byte of the trailer's CRC-32
    fb, fg, fa = tmp_path / "bad.fa.gz", tmp_path / "good.fa.gz", tmp_path / "good.fa"
    fb.write_bytes(bytes(bad))
    fg.write_bytes(good)
    fa.write_bytes(data)
    with caplog.at_level(logging.INFO, logger="deepgrp_amd.gz"):
        with pytest.raises(gz.GzipError) as e:
            list(read_multi_fasta_device(str(fb)))
    assert e.value.offset == 0 and str(fb) in str(e.value) and "incorrect data check" in str(e.value)      # zlib's words
    with pytest.raises(gz.GzipError) as host:
        gz.inflate_host(bytes(bad), str(fb), 1 << 30)
    assert str(host.value) == str(e.value)                                 # today's error: the fallback raised it
    assert any("CRC-32 or ISIZE mismatch" in l for l in _log_lines(caplog))
    main(["predict", MODEL, str(fg), "--output", str(tmp_path / "good.tsv")])
    main(["predict", MODEL, str(fa), "--output", str(tmp_path / "plain.tsv")])
    assert (tmp_path / "good.tsv").read_text().replace(str(fg), str(fa)) == (tmp_path / "plain.tsv").read_text()
    assert (tmp_path / "plain.tsv").read_text().count("\n") > 3
