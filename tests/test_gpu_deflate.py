"""BGZF output on the GPU: dgrp_bgzf_compress byte for byte against its host twin (dgrp_bgzf_compress_host, which
test_deflate_host.py holds against zlib), the round trip through the device's own inflate, mask_fasta(compress=True), and the
command line's --mask_gzip on plain, BGZF and plain-gzip inputs."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN
from deflate_corpus import BLOCK, ENOMEM, check_file, compress_host, corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


@pytest.fixture(scope="module")
def texts():
    return corpus()


def _device(data: bytes, eof: bool = True, offset: int = 0) -> bytes:
    """dgrp_bgzf_compress of `data` held at `offset` bytes behind a 16-byte aligned device address."""
    from deepgrp_amd import gz
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device=dev)
    shift = (-buf.data_ptr()) % 16 + offset
    view = buf[shift:shift + len(data)]
    if data:
        view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    assert view.data_ptr() % 16 == offset % 16
    return gz.bgzf_compress_device(view, eof=eof).cpu().numpy().tobytes()


def _inflate_on_device(comp: bytes) -> bytes:
    from deepgrp_amd import gz
    dev = torch.device("cuda", torch.cuda.current_device())
    members = gz.walk_members(comp)
    assert members.kind == "bgzf"
    d_comp = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(dev)
    return gz.inflate_device("<buffer>", members, dev, lambda _p, _n, _d: d_comp).cpu().numpy().tobytes()


def test_device_equals_host_on_the_corpus(texts):
    for name in sorted(texts):
        data = texts[name]
        for eof in (True, False):
            got = _device(data, eof)
            assert got == compress_host(data, eof), (name, eof)
        if data:
            assert _inflate_on_device(got) == data, name


def _mixed(rng, nmem=640) -> bytes:
    """`nmem` members' worth of mixed content: FASTA text of either case, N runs, random bytes, single lines repeated, headers."""
    parts, n = [], 0
    k = 0
    while n < nmem * BLOCK - 4321:
        ln = int(rng.integers(1, 3 * BLOCK))
        kind = k % 6
        if kind == 0:
            body = rng.choice(list(b"ACGT\n"), size=ln, p=[.246, .246, .246, .246, .016]).astype(np.uint8).tobytes()
        elif kind == 1:
            body = b"N" * ln
        elif kind == 2:
            body = rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
        elif kind == 3:
            body = rng.choice(list(b"ACGTacgtNn\n"), size=ln).astype(np.uint8).tobytes()
        elif kind == 4:
            line = rng.choice(list(b"ACGTacgtN"), size=60).astype(np.uint8).tobytes() + b"\n"
            body = (line * (ln // len(line) + 1))[:ln]
        else:
            body = (b">chr%d some header | with = rare ~ bytes %d\n" % (k, k * 7919) + rng.integers(32, 127, size=ln, dtype=np.uint8).tobytes())[:ln]
        parts.append(body)
        n += len(body)
        k += 1
    return b"".join(parts)[:nmem * BLOCK - 4321]


def test_many_members_equal_host_and_round_trip():
    from deepgrp_amd import gz
    data = _mixed(np.random.default_rng(23))
    got = _device(data, True)
    assert gz.walk_members(got).start.size >= 640
    assert got == compress_host(data, True)
    assert _inflate_on_device(got) == data
    assert gzip.decompress(got) == data
    check_file(got[:len(got)], data, True)


@pytest.mark.parametrize("offset", [1, 7, 15])
def test_input_at_any_alignment(texts, offset):
    for name in ("soft", "random", "len_block_plus_1", "records_10k", "one_byte"):
        data = texts[name][:5 * BLOCK + 333]
        assert _device(data, True, offset) == compress_host(data, True), name


@pytest.mark.parametrize("name", ["soft", "random"])
def test_capacity_one_byte_short_writes_nothing(texts, name):
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    data = texts[name][:4 * BLOCK + 99]
    want = compress_host(data, True)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    cap = len(want) - 1
    d_out = torch.full((cap + 256,), 0xA5, dtype=torch.uint8, device=dev)
    wb = int(L.dgrp_bgzf_workspace_bytes(len(data)))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    got = C.c_int64(-1)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.dgrp_bgzf_compress(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, C.byref(got), 1, work.data_ptr(), wb, stream)
    assert rc == ENOMEM and got.value == len(want)
    assert (d_out.cpu().numpy() == 0xA5).all()                        # nothing written, before or behind the capacity
    rc = L.dgrp_bgzf_compress(d_in.data_ptr(), len(data), d_out.data_ptr(), cap + 1, C.byref(got), 1, work.data_ptr(), wb, stream)
    assert rc == 0 and got.value == len(want)
    host = d_out.cpu().numpy()
    assert host[:cap + 1].tobytes() == want and (host[cap + 1:] == 0xA5).all()
    rc = L.dgrp_bgzf_compress(d_in.data_ptr(), len(data), d_out.data_ptr(), cap + 1, C.byref(got), 1, work.data_ptr(), wb - 1, stream)
    assert rc == ENOMEM


def test_empty_input_on_the_device():
    from deepgrp_amd import gz
    assert _device(b"", True) == gz.BGZF_EOF
    assert _device(b"", False) == b""


@pytest.mark.parametrize("level", [0, 1])
def test_members_of_a_text_deflated_in_pieces(level):
    """gz.bgzf_members_device: the members of every piece one after the other, no EOF member; an empty text, one byte, exactly
    one piece, and pieces with a rest that is no multiple of a member."""
    from deepgrp_amd import gz
    dev = torch.device("cuda", torch.cuda.current_device())
    piece = 2 * BLOCK
    rng = np.random.default_rng(31 + level)
    alphabet = np.frombuffer(b"chr1\t0.25\n", np.uint8)
    for n in (0, 1, piece, 5 * BLOCK + 17):
        text = alphabet[rng.integers(0, len(alphabet), n)]
        d_text = torch.from_numpy(text).to(dev)
        got = gz.bgzf_members_device(d_text, level, piece)
        want = b"".join(gz.bgzf_compress_device(d_text[o:o + piece], eof=False, level=level).cpu().numpy().tobytes()
                        for o in range(0, n, piece))
        assert isinstance(got, bytes) and got == want, n
        assert gzip.decompress(got) == text.tobytes(), n
        assert (got == b"") == (n == 0)
        assert len(gz.walk_members(got).isize) == sum(-(-min(piece, n - o) // BLOCK) for o in range(0, n, piece)), n
    assert gz.GZIP_PIECE % BLOCK == 0                                                   # the default piece: whole members
    assert gz.bgzf_members_device(d_text, level) == gz.bgzf_compress_device(d_text, eof=False, level=level).cpu().numpy().tobytes()


# ---------------------------------------------------------------- mask_fasta(compress=True)
def _body(rng, n, width, crlf, final_nl=True):
    seq = rng.choice(list(b"ACGTNacgtnRY*"), size=n).astype(np.uint8).tobytes()
    nl = b"\r\n" if crlf else b"\n"
    body = nl.join(seq[i:i + width] for i in range(0, n, width))
    return body + (nl if final_nl else b"")


def _mixed_file(rng) -> bytes:
    """Text before the first header, plain and CRLF records, records that take the reference's line loop (blanks around the lines,
    a sequence line that is not ASCII, lone carriage returns), an empty header, many short records, no final line end."""
    parts = [b"text before the first header\n"]
    parts.append(b">plain one\n" + _body(rng, 5000, 60, False))
    parts.append(b">crlf\r\n" + _body(rng, 3000, 70, True))
    parts.append(b">spaces\n" + b"\n".join(b"  " + _body(rng, 50, 50, False, False) + b" \t" for _ in range(30)) + b"\n")
    parts.append(b">\n" + _body(rng, 300, 60, False))
    parts.append(b">nonascii\nACGT\xc3\xa9ACGT\nACGT\n")
    for k in range(300):
        parts.append(b">s%d\n" % k + _body(rng, int(rng.integers(1, 200)), 60, False))
    parts.append(b">long\n" + _body(rng, 150_000, 60, False))
    parts.append(b">lone cr\rACGTACGT\rACGT\n")
    parts.append(b">last\n" + _body(rng, 20_000, 80, False, False))
    return b"".join(parts)


def _random_rows(rng, n):
    rows, p = [], 0
    while n and p < n:
        p += int(rng.integers(0, 400))
        if p >= n:
            break
        ln = int(rng.integers(1, 300))
        rows.append((p, min(p + ln, n), int(rng.integers(0, 5))))
        p = min(p + ln, n)
    return rows


@pytest.mark.parametrize("source", ["plain", "bgzf", "gzip"])
def test_mask_fasta_compress_equals_the_plain_copy(tmp_path, source):
    from deepgrp_amd import gz
    from deepgrp_amd.masking import mask_fasta, sequence_byte_offsets
    rng = np.random.default_rng(31)
    data = _mixed_file(rng)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    lengths = []
    start = data.index(b">")
    for _header, offs in sequence_byte_offsets(data[start:]):
        lengths.append(10 if offs is None else offs.size)
    assert len(lengths) == 307
    rows = np.array([(st, en, lab, k) for k, n in enumerate(lengths) for st, en, lab in _random_rows(rng, n)], SEG)
    src = fa
    if source != "plain":
        src = tmp_path / "in.fa.gz"
        src.write_bytes(gz.bgzf_compress(data, block=5000) if source == "bgzf" else gzip.compress(data))
    for mode, classes in (("soft", None), ("hard", (2, 4))):
        want = tmp_path / f"want_{mode}.fa"
        assert mask_fasta(str(fa), str(want), rows, mode=mode, classes=classes) == 307
        assert want.read_bytes() != data
        for group_bytes in (256 << 20, 30_000):                       # one group, and several with host-masked records among them
            out = tmp_path / f"out_{mode}_{group_bytes}.gz"
            assert mask_fasta(str(src), str(out), rows, mode=mode, classes=classes, compress=True, group_bytes=group_bytes) == 307
            comp = out.read_bytes()
            assert gzip.decompress(comp) == want.read_bytes()
            m = gz.walk_members(comp)
            assert m.kind == "bgzf" and comp.endswith(gz.BGZF_EOF)
            if group_bytes == 30_000:
                assert (m.isize[:-1] < BLOCK).sum() > 3                # group boundaries: short members
        if source != "plain":                                          # a compressed source, plain copy
            out = tmp_path / f"plain_{mode}.fa"
            assert mask_fasta(str(src), str(out), rows, mode=mode, classes=classes, group_bytes=30_000) == 307
            assert out.read_bytes() == want.read_bytes()


# ---------------------------------------------------------------- the command line
def _cli_file(rng) -> bytes:
    seq = lambda n, alpha="ACGT": "".join(rng.choice(list(alpha), size=n))
    parts = [b"lines before the first header\n"]
    for k, n in enumerate((5000, 40, 2500, 8000)):
        s = "NN" + seq(n) + "N"
        parts.append(b">chr%d some description\n" % (k + 1) + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode() + b"\n")
    s = seq(1500, "acgtn").strip("n")
    parts.append(b">crlf\r\n" + "\r\n".join(s[i:i + 70] for i in range(0, len(s), 70)).encode() + b"\r\n")
    s = seq(2500)
    parts.append(b">odd\n" + "\n".join(" " + s[i:i + 50] + "\t" for i in range(0, len(s), 50)).encode() + b"\n")
    s = seq(3000)
    parts.append(b">tail\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode())
    return b"".join(parts)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_cli_mask_gzip(tmp_path, mode):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    rng = np.random.default_rng(41)
    data = _cli_file(rng)
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    flags = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
    inputs = {}
    for form, comp in (("plain", data), ("bgzf", gz.bgzf_compress(data, block=3000)), ("gzip", gzip.compress(data))):
        d = tmp_path / form
        d.mkdir()
        inputs[form] = d / ("in.fa" if form == "plain" else "in.fa.gz")
        inputs[form].write_bytes(comp)
    fa = inputs["plain"]
    main(flags + ["predict", model, str(fa), "--output", str(tmp_path / "ref.tsv"), "--mask_dir", str(tmp_path / "ref"), "--mask", mode])
    want, want_tsv = (tmp_path / "ref" / "in.fa").read_bytes(), (tmp_path / "ref.tsv").read_text()
    assert want != data and want_tsv.count("\n") > 3
    for form, path in inputs.items():
        mdir, tsv = tmp_path / f"masked_{form}", tmp_path / f"{form}.tsv"
        argv = flags + ["predict", model, str(path), "--output", str(tsv), "--mask_dir", str(mdir), "--mask", mode, "--mask_gzip"]
        if form == "bgzf":                                             # README form, the flags in front
            argv = ["--mask_gzip", "--mask_dir", str(mdir), "--mask", mode] + flags + [model, str(path), "--output", str(tsv)]
        main(argv)
        assert os.listdir(mdir) == ["in.fa.gz"]
        comp = (mdir / "in.fa.gz").read_bytes()
        assert gz.walk_members(comp).kind == "bgzf" and comp.endswith(gz.BGZF_EOF)
        assert gzip.decompress(comp) == want
        assert tsv.read_text().replace(str(path), str(fa)) == want_tsv
        if mode == "soft":
            # the masked copy is an input like any other: the same rows under its own name (letter case does not reach the model;
            # a hard mask's N do, so only the soft copy can be asked for the same rows)
            back = tmp_path / f"back_{form}.tsv"
            main(flags + ["predict", model, str(mdir / "in.fa.gz"), "--output", str(back)])
            assert back.read_text().replace(str(mdir / "in.fa.gz"), str(fa)) == want_tsv
    # a.fa and a.fa.gz collide only once .gz is appended: refused before the model is loaded
    a, az = tmp_path / "a.fa", tmp_path / "a.fa.gz"
    a.write_bytes(data)
    az.write_bytes(gz.bgzf_compress(data))
    import deepgrp_amd.model as dgmodel
    loaded = []
    orig = dgmodel.load_model, dgmodel.device_model
    dgmodel.load_model = lambda *x, **k: loaded.append(1) or orig[0](*x, **k)
    dgmodel.device_model = lambda *x, **k: loaded.append(1) or orig[1](*x, **k)
    try:
        with pytest.raises(SystemExit) as e:
            main(["predict", model, str(a), str(az), "--mask_dir", str(tmp_path / "clash"), "--mask_gzip", "--output", str(tmp_path / "c.tsv")])
    finally:
        dgmodel.load_model, dgmodel.device_model = orig
    assert "same file name" in str(e.value.code) and not loaded and not (tmp_path / "clash").exists()
