"""Compressed FASTA input on the GPU: dgrp_inflate_batch against zlib, read_multi_fasta_device on .fa.gz (BGZF, plain gzip,
multi-member) against the same file uncompressed, the command line on compressed inputs, and a corrupt member."""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY, zlib.Z_FILTERED)


def _mixed_bgzf(rng, nmem=640):
    """A BGZF file of `nmem` members (+ the EOF member) of mixed content, levels and strategies, full 64 KiB members among them and
    a ragged last member; -> (compressed bytes, inflated bytes)."""
    from deepgrp_amd import gz
    members, plain = [], []
    for m in range(nmem):
        kind = m % 5
        n = 65536 if m % 97 == 3 else int(rng.integers(1, 6000))
        if m == nmem - 1:
            n = 777                                                            # ragged last member
        if kind == 0:
            body = rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
        elif kind == 1:
            body = b"N" * n
        elif kind == 2:
            body = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        elif kind == 3:
            line = rng.choice(list(b"ACGTacgtN"), size=60).astype(np.uint8).tobytes() + b"\n"
            body = (line * (n // len(line) + 1))[:n]
        else:
            body = (b">chr%d header\n" % m + b"ACGTTGCA" * n)[:n]
        level = (0, 1, 6, 9)[m % 4]
        if n == 65536:                                                         # a full member: compressible content
            body, level = rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes(), 6
        members.append(gz.bgzf_member(body, level, STRATEGIES[(m // 4) % 5]))
        plain.append(body)
    return b"".join(members) + gz.BGZF_EOF, b"".join(plain)


def test_inflate_batch_matches_zlib(tmp_path):
    from deepgrp_amd import gz
    from deepgrp_amd.fasta import _upload_file
    rng = np.random.default_rng(5)
    comp, want = _mixed_bgzf(rng)
    assert gzip.decompress(comp) == want
    path = tmp_path / "mixed.bin.gz"
    path.write_bytes(comp)
    members = gz.walk_members(comp, str(path))
    assert members.kind == "bgzf" and members.start.size >= 600
    dev = torch.device("cuda", torch.cuda.current_device())
    got = gz.inflate_device(str(path), members, dev, _upload_file)
    assert got.numel() == len(want)
    assert got.cpu().numpy().tobytes() == want


def _odd_fasta(rng) -> bytes:
    """The odd-record fixture: headerless start, an empty record, an all-N record, CRLF, lower case, a record that takes the
    reference loop (tabs), a header longer than a BGZF member, a long record spanning members, and 10^4 short records."""
    seq = lambda n, alpha="ACGT": "".join(rng.choice(list(alpha), size=n))
    parts = [b"text before the first header\n"]
    parts.append(b">empty\n")
    parts.append(b">allN\n" + b"NNNNNNNNNN\n" * 30)
    s = seq(3000)
    parts.append(b">crlf record\r\n" + "\r\n".join(s[i:i + 70] for i in range(0, len(s), 70)).encode() + b"\r\n")
    s = seq(2000, "acgtn")
    parts.append(b">lower\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode() + b"\n")
    s = seq(900)
    parts.append(b">tabs\n" + "\n".join("\t" + s[i:i + 50] for i in range(0, len(s), 50)).encode() + b"\n")
    parts.append(b">" + b"H" * 5000 + b" very long header\n" + seq(500).encode() + b"\n")
    s = "NNN" + seq(150_000) + "NN"
    parts.append(b">long spanning record\n" + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode() + b"\n")
    for k in range(10_000):
        parts.append(b">s%d\n" % k + seq(int(rng.integers(1, 40))).encode() + b"\n")
    parts.append(b">last no newline\n" + seq(333).encode())
    return b"".join(parts)


def _records(path):
    from deepgrp_amd.fasta import DeviceRecord, read_multi_fasta_device
    out = []
    for header, rec in read_multi_fasta_device(str(path)):
        if isinstance(rec, DeviceRecord):
            idx = rec.d_idx.cpu().numpy().tobytes() if rec.length > 0 else b""
            out.append((header, "dev", rec.startpos, rec.length, idx))
        else:
            out.append((header, "str", rec))
    return out


@pytest.mark.parametrize("form", ["bgzf", "gzip", "multi"])
def test_read_multi_fasta_device_on_gz(tmp_path, form):
    from deepgrp_amd import gz
    rng = np.random.default_rng(8)
    data = _odd_fasta(rng)
    fa = tmp_path / "x.fa"
    fa.write_bytes(data)
    if form == "bgzf":
        comp = gz.bgzf_compress(data, 6, block=1000)                     # many member boundaries: headers and records span them
    elif form == "gzip":
        comp = gzip.compress(data, 6)
    else:                                                                  # plain members, BGZF members, plain again
        a, b = len(data) // 3, 2 * len(data) // 3
        comp = gzip.compress(data[:a]) + gz.bgzf_compress(data[a:b], eof=False) + gzip.compress(data[b:], 1)
    fz = tmp_path / "x.fa.gz"
    fz.write_bytes(comp)
    assert gz.walk_members(comp).kind == ("bgzf" if form == "bgzf" else "gzip")
    want, got = _records(fa), _records(fz)
    assert len(want) > 10_000
    assert got == want


def _cli_fasta(rng) -> bytes:
    seq = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    parts = []
    for k, n in enumerate((5000, 40, 2500, 8000)):
        s = "NN" + seq(n) + "N"
        parts.append(b">chr%d\n" % (k + 1) + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)).encode() + b"\n")
    return b"".join(parts)


def test_cli_predict_and_evaluate_on_gz(tmp_path):
    from deepgrp_amd import gz, synthetic
    from deepgrp_amd.__main__ import main
    rng = np.random.default_rng(3)
    data = _cli_fasta(rng)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    forms = {"bgzf": gz.bgzf_compress(data, block=3000), "gzip": gzip.compress(data)}
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    flags = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
    main(flags + ["predict", model, str(fa), "--output", str(tmp_path / "plain.tsv")])
    plain = (tmp_path / "plain.tsv").read_text()
    assert plain.count("\n") > 3
    ann = tmp_path / "ann.bed"
    ann.write_text("".join(line for k in (1, 3, 4) for line in synthetic.synthetic_annotation(8000, contig=k, name=f"chr{k}", flank=100)))
    main(["evaluate", model, str(ann), str(fa), "--output", str(tmp_path / "plain_eval.tsv"), "--json", str(tmp_path / "plain.json")])
    for name, comp in forms.items():
        fz = tmp_path / f"in_{name}.fa.gz"
        fz.write_bytes(comp)
        tsv = tmp_path / f"{name}.tsv"
        main(flags + ["predict", model, str(fz), "--output", str(tsv)])
        got = tsv.read_text()
        assert got.count(str(fz)) == plain.count(str(fa))                 # first column: the file name as given
        assert got.replace(str(fz), str(fa)) == plain
        main(["evaluate", model, str(ann), str(fz), "--output", str(tmp_path / f"{name}_eval.tsv"), "--json",
              str(tmp_path / f"{name}.json")])
        assert (tmp_path / f"{name}_eval.tsv").read_text().replace(str(fz), str(fa)) == (tmp_path / "plain_eval.tsv").read_text()
        js = json.loads((tmp_path / f"{name}.json").read_text().replace(str(fz), str(fa)))
        assert js == json.loads((tmp_path / "plain.json").read_text())


def test_corrupt_bgzf_member_then_predict(tmp_path):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.fasta import read_multi_fasta_device
    rng = np.random.default_rng(4)
    data = _cli_fasta(rng)
    comp = bytearray(gz.bgzf_compress(data, block=2000))
    members = gz.walk_members(bytes(comp))
    k = 2
    crc_at = int(members.data_off[k] + members.data_len[k])
    comp[crc_at] ^= 0x40                                                   # member k's CRC-32 no longer matches
    bad = tmp_path / "bad.fa.gz"
    bad.write_bytes(bytes(comp))
    with pytest.raises(gz.GzipError) as e:
        list(read_multi_fasta_device(str(bad)))
    assert e.value.offset == int(members.start[k])
    assert str(bad) in str(e.value) and f"offset {int(members.start[k])}" in str(e.value) and "CRC" in str(e.value)
    with pytest.raises(gz.GzipError):
        main(["predict", os.path.join(GOLDEN, "model_u8_T20.h5"), str(bad), "--output", str(tmp_path / "bad.tsv")])
    good = tmp_path / "good.fa.gz"
    good.write_bytes(gz.bgzf_compress(data, block=2000))
    fa = tmp_path / "good.fa"
    fa.write_bytes(data)
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    main(["predict", model, str(good), "--output", str(tmp_path / "good.tsv")])
    main(["predict", model, str(fa), "--output", str(tmp_path / "plain.tsv")])
    assert (tmp_path / "good.tsv").read_text().replace(str(good), str(fa)) == (tmp_path / "plain.tsv").read_text()
    assert (tmp_path / "plain.tsv").read_text().count("\n") > 3
