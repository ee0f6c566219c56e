"""BGZF output with matches on the GPU: dgrp_bgzf_compress_level at level 1 byte for byte against its host twin (which
test_deflate_lz_host.py holds against zlib), level 0 through the new entry against the old one, the round trip through the device's
own inflate (distance codes the level-0 files never gave it), and mask_fasta(compress=True, level=1)."""
import ctypes as C
import gzip

import numpy as np
import pytest

from deflate_corpus import BLOCK, ENOMEM, check_file, compress_host
from deflate_lz_corpus import all_texts, compress_host_level
from test_gpu_deflate import SEG, _inflate_on_device, _mixed, _mixed_file, _random_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def texts():
    return all_texts()


def _device(data: bytes, eof: bool = True, offset: int = 0, level: int = 1) -> bytes:
    """dgrp_bgzf_compress_level of `data` held at `offset` bytes behind a 16-byte aligned device address."""
    from deepgrp_amd import gz
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device=dev)
    shift = (-buf.data_ptr()) % 16 + offset
    view = buf[shift:shift + len(data)]
    if data:
        view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert view.data_ptr() % 16 == offset % 16
    return gz.bgzf_compress_device(view, eof=eof, level=level).cpu().numpy().tobytes()


def test_device_equals_host_on_the_corpus(texts):
    for name in sorted(texts):
        data = texts[name]
        for eof in (True, False):
            got = _device(data, eof)
            assert got == compress_host_level(data, eof, 1), (name, eof)
        if data:
            assert _inflate_on_device(got) == data, name


def test_level_0_is_the_old_entry(texts):
    from deepgrp_amd import gz
    dev = torch.device("cuda", torch.cuda.current_device())
    for name in sorted(texts):
        data = texts[name]
        d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev) if data else torch.empty(0, dtype=torch.uint8, device=dev)
        old = gz.bgzf_compress_device(d).cpu().numpy().tobytes()
        assert _device(data, True, level=0) == old == compress_host(data, True), name


def test_many_members_equal_host_and_round_trip():
    from deepgrp_amd import gz
    data = _mixed(np.random.default_rng(23))
    got = _device(data, True)
    assert gz.walk_members(got).start.size >= 640
    assert got == compress_host_level(data, True, 1)
    assert _inflate_on_device(got) == data
    assert gzip.decompress(got) == data
    check_file(got, data, True)


@pytest.mark.parametrize("offset", list(range(1, 16)))
def test_input_at_any_alignment(texts, offset):
    for name in ("soft", "bedgraph_d2_bin1", "len_block_plus_1", "n_run", "bytes_1"):
        data = texts[name][:3 * BLOCK + 333]
        assert _device(data, True, offset) == compress_host_level(data, True, 1), name


@pytest.mark.parametrize("name", ["soft", "bedgraph_d3_bin1_long_name", "random"])
def test_capacity_one_byte_short_writes_nothing(texts, name):
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    data = texts[name][:4 * BLOCK + 99]
    want = compress_host_level(data, True, 1)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    cap = len(want) - 1
    d_out = torch.full((cap + 256,), 0xA5, dtype=torch.uint8, device=dev)
    wb = int(L.dgrp_bgzf_workspace_bytes_level(len(data), 1))
    assert wb > int(L.dgrp_bgzf_workspace_bytes(len(data))) == int(L.dgrp_bgzf_workspace_bytes_level(len(data), 0))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    got = C.c_int64(-1)
    stream = torch.cuda.current_stream().cuda_stream
    args = (d_in.data_ptr(), len(data), d_out.data_ptr())
    rc = L.dgrp_bgzf_compress_level(*args, cap, C.byref(got), 1, 1, work.data_ptr(), wb, stream)
    assert rc == ENOMEM and got.value == len(want)
    assert (d_out.cpu().numpy() == 0xA5).all()                        # nothing written, before or behind the capacity
    rc = L.dgrp_bgzf_compress_level(*args, cap + 1, C.byref(got), 1, 1, work.data_ptr(), wb, stream)
    assert rc == 0 and got.value == len(want)
    host = d_out.cpu().numpy()
    assert host[:cap + 1].tobytes() == want and (host[cap + 1:] == 0xA5).all()
    rc = L.dgrp_bgzf_compress_level(*args, cap + 1, C.byref(got), 1, 1, work.data_ptr(), wb - 1, stream)
    assert rc == ENOMEM
    rc = L.dgrp_bgzf_compress_level(*args, cap + 1, C.byref(got), 1, 2, work.data_ptr(), wb, stream)
    assert rc == -1 and b"level" in L.dgrp_last_error()


def test_empty_input_on_the_device():
    from deepgrp_amd import gz
    assert _device(b"", True) == gz.BGZF_EOF
    assert _device(b"", False) == b""


def test_mask_fasta_level_1_equals_the_plain_copy(tmp_path):
    from deepgrp_amd import gz
    from deepgrp_amd.masking import mask_fasta, sequence_byte_offsets
    rng = np.random.default_rng(31)
    data = _mixed_file(rng)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    lengths = [10 if offs is None else offs.size for _header, offs in sequence_byte_offsets(data[data.index(b">"):])]
    rows = np.array([(st, en, lab, k) for k, n in enumerate(lengths) for st, en, lab in _random_rows(rng, n)], SEG)
    for mode, classes in (("soft", None), ("hard", (2, 4))):
        want = tmp_path / f"want_{mode}.fa"
        mask_fasta(str(fa), str(want), rows, mode=mode, classes=classes)
        sizes = {}
        for level in (0, 1):
            for group_bytes in (256 << 20, 30_000):
                out = tmp_path / f"out_{mode}_{level}_{group_bytes}.gz"
                mask_fasta(str(fa), str(out), rows, mode=mode, classes=classes, compress=True, level=level, group_bytes=group_bytes)
                comp = out.read_bytes()
                assert gzip.decompress(comp) == want.read_bytes()
                assert gz.walk_members(comp).kind == "bgzf" and comp.endswith(gz.BGZF_EOF)
                sizes[level, group_bytes] = len(comp)
        assert sizes[1, 256 << 20] <= sizes[0, 256 << 20] and sizes[1, 30_000] <= sizes[0, 30_000]
