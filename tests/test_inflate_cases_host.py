"""The corpus of tests/inflate_cases.py without a GPU: its grids are what they claim under zlib and under dgrp_inflate_raw_host, the
fuzz streams split into enough accepted and enough refused ones for the device test to mean something, and the two host entries
differ in their reason on exactly the streams the device tests are told about."""
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_cases as ic                              # noqa: E402
from deepgrp_amd import gz                              # noqa: E402

EDATA = -5
raw_host, stream_host = ic.raw_host, ic.stream_host


def test_grids_decode_under_zlib_and_the_host_entry():
    grids = {"copy": ic.copy_grid(), "stored": ic.stored_grid(), "size": ic.size_grid()}
    assert len(grids["copy"]) == len(ic.COPY_DIST) * len(ic.COPY_LEN) == 198
    assert len(grids["stored"]) == 2 * len(ic.STORED_LEN) and len(grids["size"]) == len(ic.SIZES)
    for grid in grids.values():
        assert len({name for name, _, _ in grid}) == len(grid)
        for name, stream, text in grid:
            assert zlib.decompress(stream, -15) == text, name
            assert len(text) <= gz.BGZF_MAX_ISIZE, name
            assert raw_host(stream, len(text)) == (0, 0, text, len(stream)), name
    for name, stream, text in grids["copy"]:                          # the last symbol writes the last byte: one short is refused
        assert raw_host(stream, len(text) - 1)[:2] == (EDATA, ic.EOUTPUT), name
    assert [len(t) for _, _, t in grids["size"]] == list(ic.SIZES)
    # a stored block behind 18 bits of a fixed block starts inside a byte
    assert all(s[0] & 7 == 2 for n, s, _ in grids["stored"] if n.startswith("fixed_then"))


def test_member_and_bgzf_wrap():
    text = ic.GOOD_TEXT
    data, trailer, cap = ic.member(ic.GOOD)
    assert (data, cap) == (ic.GOOD, len(text)) and trailer == zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little")
    assert ic.member(ic.GOOD, crc=1, isize=2, cap=3)[1:] == (b"\x01\0\0\0\x02\0\0\0", 3)
    assert ic.member(b"\x07", crc=0, isize=0, cap=100) == (b"\x07", b"\0" * 8, 100)          # a stream zlib refuses
    assert ic.bgzf_wrap(data, trailer) == gz.bgzf_member(text, 6)
    crafted = ic.bgzf_wrap(*ic.member(ic.FIXED["distance_too_far"][1], crc=0, isize=100, cap=100)[:2])
    m = gz.walk_members(ic.bgzf_wrap(data, trailer) + crafted + gz.BGZF_EOF)
    assert m.kind == "bgzf" and m.isize.tolist() == [len(text), 100, 0]
    assert m.data_len.tolist() == [len(data), len(ic.FIXED["distance_too_far"][1]), 2]
    assert m.start.tolist() == [0, 26 + len(data), 26 + len(data) + len(crafted)]


def test_fuzz_split_and_corpus_shape():
    assert set(ic.FIXED) == set(ic.PINNED) and len(ic.FIXED) == 21 and len(ic.FUZZ) == 60 and len(ic.TRUNCATED) == 6
    accepted = refused = 0
    for name, stream, cap, _ in ic.FUZZ:
        rc, reason, _out, _used = raw_host(stream, cap)
        assert (rc == 0 and reason == 0) or (rc == EDATA and reason > 0), name
        accepted += rc == 0
        refused += rc != 0
    print("fuzz: accepted", accepted, "refused", refused)
    assert accepted >= 15 and refused >= 15


def test_host_entries_differ_in_reason_on_five_streams_only():
    """dgrp_inflate_raw_host and dgrp_inflate_stream_host agree on refusal or acceptance everywhere, on the text and the bytes used
    where they accept, and on the reason except for HOST_ENTRIES_DIFFER, where the counting pass of the span path meets a later
    error before the window walk can report the bad distance."""
    for chunk in (64, 1024):
        differ = []
        for name, stream, cap, _ in ic.CORRUPT:
            raw, span = raw_host(stream, cap), stream_host(stream, chunk, cap)
            assert raw[0] == span[0], name
            if raw[0] == 0:
                assert raw == span, name
            elif raw[1] != span[1]:
                differ.append(name)
        assert sorted(differ) == sorted(ic.HOST_ENTRIES_DIFFER), chunk
