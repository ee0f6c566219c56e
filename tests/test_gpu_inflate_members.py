"""The member kernel (dgrp_inflate_batch, inflate_member_kernel) on crafted members: the lane-split match and stored copies at
distances and lengths around 64, the per-lane CRC-32 at sizes around 64, every refusal of the decode core and of the trailer check
with its reason, the order of those checks, the lowest failing member, and the refusals as read_multi_fasta_device reports them.

Every call goes through `run`: the compressed bytes stand at an offset inside one device tensor with PAD bytes of filler on both
sides, the output inside a tensor of sentinels with PAD sentinels on both sides, the workspace between guards.  PAD = 128 KiB is
more than anything a wrong copy could reach (a match 32 768 back and 258 forward, a stored block 65 535 forward, the bit reader 4
bytes), so a violation of "no read or write leaves the member's slices" lands in our own allocation and fails an assertion.  The
expected text is zlib's; the expected reason is the host entry's on the same bytes (dgrp_inflate_raw_host, the core without the
trailer) or, for the trailer, the table of test_trailer_reasons_and_their_order -- never what the device says."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_cases as ic                              # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EDATA = -5
PAD = 128 << 10
GUARD = 512
SENTINEL, WORK_FILL = 0xa5, 0x3c
TEXTS = {ic.ECRC: "CRC-32 mismatch", ic.EISIZE: "output shorter than ISIZE", ic.ETRAIL: "stream ends before the trailer"}
_FILLER = np.random.default_rng(128).integers(0, 256, size=2 * PAD + 8, dtype=np.uint8).tobytes()


class Result:
    def __init__(self, rc, bad, reason, slices, error, raw):
        self.rc, self.bad, self.reason, self.slices, self.error, self.raw = rc, bad, reason, slices, error, raw

    @property
    def status(self):
        return self.rc, self.bad, self.reason


def run(members, shift=0):
    """dgrp_inflate_batch on `members`: (data, trailer, output slice length) or (data, trailer, slice length, in_len) where the
    member is said to be shorter than the bytes that stand in the buffer.  Members and output slices are adjacent.  `shift`: the
    first member's offset from a 256-byte boundary.  Asserts that nothing but the output slices changed."""
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    blobs = [m[0] + m[1] for m in members]
    in_len = np.array([m[3] if len(m) > 3 else len(m[0]) for m in members], np.int64)
    in_off = PAD + shift + np.cumsum([0] + [len(b) for b in blobs[:-1]]).astype(np.int64)
    host_in = _FILLER[:PAD + shift] + b"".join(blobs) + _FILLER[PAD + shift:2 * PAD + shift]
    out_off = np.zeros(len(members) + 1, np.int64)
    np.cumsum([m[2] for m in members], out=out_off[1:])
    total = int(out_off[-1])
    d_in = torch.frombuffer(bytearray(host_in), dtype=torch.uint8).to(dev)
    d_out = torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    wb = int(L.dgrp_inflate_workspace_bytes(len(members)))
    assert wb > 0 and wb % 256 == 0
    work = torch.full((wb + 2 * GUARD,), WORK_FILL, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0 and work.data_ptr() % 256 == 0
    bad, reason = C.c_int64(-7), C.c_int(-7)
    rc = L.dgrp_inflate_batch(d_in.data_ptr(), len(host_in), len(members), in_off.ctypes.data, in_len.ctypes.data, out_off.ctypes.data,
                              d_out.data_ptr() + PAD, total, C.byref(bad), C.byref(reason), work.data_ptr() + GUARD, wb,
                              torch.cuda.current_stream().cuda_stream)
    error = L.dgrp_last_error().decode() if rc != 0 else ""
    got = d_out.cpu().numpy()
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + total:] == SENTINEL).all(), "wrote outside the output slices"
    guards = work.cpu().numpy()
    assert (guards[:GUARD] == WORK_FILL).all() and (guards[GUARD + wb:] == WORK_FILL).all(), "wrote outside the workspace"
    assert d_in.cpu().numpy().tobytes() == host_in, "the input changed"
    body = got[PAD:PAD + total].tobytes()
    slices = [body[out_off[m]:out_off[m + 1]] for m in range(len(members))]
    return Result(rc, bad.value, reason.value, slices, error, body)


def members_of(grid):
    return [ic.member(stream) for _name, stream, _text in grid]


def assert_all_equal_zlib(res, grid):
    assert res.status == (0, -1, 0)
    for (name, _stream, text), got in zip(grid, res.slices):
        assert got == text, name


GOOD_A = ic.member(ic.GOOD)
GOOD_B = ic.member(ic.copy_grid()[ic.COPY_LEN.index(129) + len(ic.COPY_LEN) * ic.COPY_DIST.index(65)][1])
TEXT_A, TEXT_B = ic.GOOD_TEXT, zlib.decompress(GOOD_B[0], -15)


def run_between_good(case):
    """`case` as member 1 of [good, case, good]: both neighbours must be whole whatever the case does"""
    res = run([GOOD_A, case, GOOD_B])
    assert res.slices[0] == TEXT_A and res.slices[2] == TEXT_B, "a member beside the case is not zlib's text"
    return res


# ---------------------------------------------------------------------------------------------------------- a. valid grids
@pytest.mark.parametrize("shift", [0, 1, 7])
def test_copy_grid_equals_zlib(shift):
    grid = ic.copy_grid()
    assert_all_equal_zlib(run(members_of(grid), shift), grid)


@pytest.mark.parametrize("grid", ["stored_grid", "size_grid"])
def test_stored_and_size_grids_equal_zlib(grid):
    grid = getattr(ic, grid)()
    assert_all_equal_zlib(run(members_of(grid)), grid)


# ---------------------------------------------------------------------------------------------------------- b. stream reasons
@pytest.mark.parametrize("name", sorted(ic.PINNED))
def test_every_stream_reason_alone_and_between_good_members(name):
    _, stream, cap, reason = ic.FIXED[name]
    assert reason == ic.PINNED[name][1]
    case = ic.member(stream, crc=0x12345678, isize=cap, cap=cap)
    assert run([case]).status == (EDATA, 0, reason)
    assert run_between_good(case).status == (EDATA, 1, reason)


# ---------------------------------------------------------------------------------------------------------- c. input slice
@pytest.mark.parametrize("name", [c[0] for c in ic.TRUNCATED])
def test_the_reader_stops_at_in_len(name):
    """The truncated streams once more, but behind in_len the buffer goes on with the rest of the stream (and the trailer is read
    from stream bytes): a reader that runs past in_len decodes on and gives another reason than EINPUT, or none."""
    _, stream, cap, reason = ic.FIXED[name]
    assert reason == ic.EINPUT and ic.GOOD[:len(stream)] == stream and len(stream) < len(ic.GOOD)
    case = GOOD_A + (len(stream),)
    assert run([case]).status == (EDATA, 0, ic.EINPUT)
    assert run_between_good(case).status == (EDATA, 1, ic.EINPUT)


# ---------------------------------------------------------------------------------------------------------- d. fuzz
def test_fuzz_split_is_not_vacuous():
    accepted = sum(ic.raw_host(stream, cap)[0] == 0 for _, stream, cap, _ in ic.FUZZ)
    assert accepted >= 15 and len(ic.FUZZ) - accepted >= 15


@pytest.mark.parametrize("name,stream,cap", [c[:3] for c in ic.FUZZ], ids=[c[0] for c in ic.FUZZ])
def test_fuzzed_member_between_good_members(name, stream, cap):
    """What the device must say follows from the host entry on the same bytes: its reason where it refuses; ETRAIL where it accepts
    a stream that ends before in_len; and where it accepts the whole, a trailer made for its output (zlib's, too) is accepted."""
    hrc, hreason, hout, hused = ic.raw_host(stream, cap)
    if hrc != 0:
        res = run_between_good(ic.member(stream, crc=0, isize=cap, cap=cap))
        assert hrc == EDATA and hreason > 0 and res.status == (EDATA, 1, hreason)
    elif hused < len(stream):
        res = run_between_good(ic.member(stream, crc=zlib.crc32(hout), isize=len(hout), cap=cap))
        assert res.status == (EDATA, 1, ic.ETRAIL)
    else:
        assert ic.zlib_says(stream) == (hout, len(stream))
        res = run_between_good(ic.member(stream, crc=zlib.crc32(hout), isize=len(hout), cap=cap))
        assert res.status == (0, -1, 0) and res.slices[1][:len(hout)] == hout


# ---------------------------------------------------------------------------------------------------------- e. trailer reasons
def _trailer_cases():
    n, crc = len(ic.GOOD_TEXT), zlib.crc32(ic.GOOD_TEXT)
    hello = bytes([0x01, 5, 0, 0xFA, 0xFF]) + b"hello"
    far = ic.FIXED["distance_too_far"][1]
    return {
        "crc_low_bit": (ic.member(ic.GOOD, crc=crc ^ 1), ic.ECRC),
        "crc_high_bit": (ic.member(ic.GOOD, crc=crc ^ 0x80000000), ic.ECRC),
        "isize_plus_1_slice_plus_1": (ic.member(ic.GOOD, isize=n + 1, cap=n + 1), ic.EISIZE),
        "isize_minus_1_slice_as_it_is": (ic.member(ic.GOOD, isize=n - 1), ic.EOUTPUT),                # from the trailer check
        "isize_minus_1_slice_minus_1": (ic.member(ic.GOOD, isize=n - 1, cap=n - 1), ic.EOUTPUT),      # from the core
        "zero_byte_before_the_trailer": (ic.member(ic.GOOD + b"\0", crc=crc, isize=n, cap=n), ic.ETRAIL),
        "stored_block_behind_the_final_one": (ic.member(hello + hello, crc=zlib.crc32(b"hello"), isize=5, cap=5), ic.ETRAIL),
        # the order: stream reason, then ETRAIL, then EISIZE / EOUTPUT, then ECRC
        "junk_isize_crc": (ic.member(ic.GOOD + b"\0", crc=crc ^ 1, isize=n + 1, cap=n + 1), ic.ETRAIL),
        "isize_crc": (ic.member(ic.GOOD, crc=crc ^ 1, isize=n + 1, cap=n + 1), ic.EISIZE),
        "isize_low_crc": (ic.member(ic.GOOD, crc=crc ^ 1, isize=n - 1), ic.EOUTPUT),
        "bad_stream_fitting_trailer": (ic.member(far, crc=zlib.crc32(b"A"), isize=1, cap=1), ic.EDIST),
        "bad_stream_junk_fitting_trailer": (ic.member(far + b"\0", crc=zlib.crc32(b"A"), isize=1, cap=1), ic.EDIST),
    }


@pytest.mark.parametrize("name", sorted(_trailer_cases()))
def test_trailer_reasons_and_their_order(name):
    from deepgrp_amd import gz
    case, reason = _trailer_cases()[name]
    for k, res in ((0, run([case])), (1, run_between_good(case))):
        assert res.status == (EDATA, k, reason)
        if reason in TEXTS:
            assert res.error == f"dgrp_inflate_batch: member {k}: {TEXTS[reason]} (reason {reason})"
            assert reason in gz.REASONS


def test_trailer_cases_cover_reasons_8_9_10():
    assert {ic.ECRC, ic.EISIZE, ic.ETRAIL} <= {r for _, r in _trailer_cases().values()}
    assert ic.raw_host(ic.GOOD + b"\0", len(ic.GOOD_TEXT))[::3] == (0, len(ic.GOOD))            # the core accepts it and stops early
    for name, ((data, _trailer, cap), reason) in _trailer_cases().items():                      # the stream reasons are the host's
        if name.startswith("bad_stream"):
            assert ic.raw_host(data, cap)[:3] == (EDATA, reason, b"A")


# ---------------------------------------------------------------------------------------------------------- f. CRC at the size edges
@pytest.mark.parametrize("name,stream,text", ic.size_grid(), ids=[c[0] for c in ic.size_grid()])
def test_crc_sees_the_first_and_the_last_byte(name, stream, text):
    """The trailer holds the CRC-32 of the text with one byte changed: a CRC that left out a lane's piece would accept it."""
    res = run([ic.member(stream)])
    assert res.status == (0, -1, 0) and res.slices[0] == text
    if not text:
        return
    for at in (0, len(text) - 1):
        other = bytearray(text)
        other[at] ^= 0x04
        assert run([ic.member(stream, crc=zlib.crc32(bytes(other)))]).status == (EDATA, 0, ic.ECRC), at


# ---------------------------------------------------------------------------------------------------------- g. lowest failing member
def test_the_lowest_failing_member_is_reported():
    grid = ic.size_grid()
    texts = [grid[k % len(grid)][2] for k in range(200)]
    good = [ic.member(grid[k % len(grid)][1]) for k in range(200)]
    members = list(good)
    n, crc = len(texts[131]), zlib.crc32(texts[131])
    members[131] = ic.member(good[131][0], crc=crc ^ 0x100)
    members[64] = ic.member(good[64][0], isize=len(texts[64]) + 1, cap=len(texts[64]) + 1)
    members[7] = ic.member(ic.FIXED["distance_too_far"][1], crc=0, isize=100, cap=100)
    assert n > 0
    for fix, want in ((None, (EDATA, 7, ic.EDIST)), (7, (EDATA, 64, ic.EISIZE)), (64, (EDATA, 131, ic.ECRC)), (131, (0, -1, 0))):
        if fix is not None:
            members[fix] = good[fix]
        res = run(members)
        assert res.status == want
        for k in range(200):                                                 # every member but the failing ones is whole
            if members[k] is good[k]:
                assert res.slices[k] == texts[k], k


# ---------------------------------------------------------------------------------------------------------- h. the same call twice
def test_the_same_call_twice_gives_the_same_bytes():
    members = members_of(ic.copy_grid())
    first, second = run(members), run(members)
    assert first.status == second.status == (0, -1, 0) and first.raw == second.raw


# ---------------------------------------------------------------------------------------------------------- i. through Python
def _crafted_for_python():
    n, crc = len(ic.GOOD_TEXT), zlib.crc32(ic.GOOD_TEXT)
    return {
        "trail": (ic.member(ic.GOOD + b"\0", crc=crc, isize=n, cap=n), ic.ETRAIL),
        "isize": (ic.member(ic.GOOD, isize=n + 1, cap=n + 1), ic.EISIZE),
        "output": (ic.member(ic.GOOD, isize=n - 1, cap=n - 1), ic.EOUTPUT),
        "dist": (ic.member(ic.FIXED["distance_too_far"][1], crc=0, isize=100, cap=100), ic.EDIST),
        "input": (ic.member(ic.FIXED["truncated_3247"][1], crc=crc, isize=n, cap=n), ic.EINPUT),
    }


@pytest.mark.parametrize("name", sorted(_crafted_for_python()))
def test_read_multi_fasta_device_names_the_member_and_the_reason(tmp_path, name):
    from deepgrp_amd import gz
    from deepgrp_amd.fasta import read_multi_fasta_device
    (data, trailer, cap), reason = _crafted_for_python()[name]
    assert struct.unpack("<I", trailer[4:])[0] == cap                        # the ingest takes the slice from ISIZE
    second = b">chr2\n" + ic.INPUTS["fasta"][20_000:30_000]
    comp = ic.bgzf_wrap(*GOOD_A[:2]) + ic.bgzf_wrap(data, trailer) + gz.bgzf_member(second) + gz.BGZF_EOF
    path = tmp_path / f"{name}.fa.gz"
    path.write_bytes(comp)
    members = gz.walk_members(comp, str(path))
    assert members.kind == "bgzf" and members.start.size == 4 and members.start[1] == 26 + len(ic.GOOD)
    with pytest.raises(gz.GzipError) as e:
        list(read_multi_fasta_device(str(path)))
    assert e.value.offset == int(members.start[1]) and gz.REASONS[reason] in str(e.value) and str(path) in str(e.value)
