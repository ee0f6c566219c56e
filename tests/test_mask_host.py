"""predict --mask_dir on the CPU: flag parsing, the refusals that come before any prediction, and the byte mapping of records that go
through the reference's line loop (masking.sequence_byte_offsets) against fasta.LineLoop itself."""
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN


def _args(argv):
    from deepgrp_amd.__main__ import CommandLineParser
    return CommandLineParser().parse_args(argv).args


def test_mask_flags_parse_in_both_forms():
    a = _args(["--mask_dir", "out", "m.h5", "x.fa"])                              # README form, the flag in front
    assert (a.command, a.mask_dir, a.model, a.FASTA) == ("predict", "out", "m.h5", ["x.fa"])
    a = _args(["-b", "7", "--mask", "hard", "--mask_classes", "1,3", "--mask_dir", "d", "m.h5", "x.fa", "y.fa"])
    assert (a.command, a.mask, a.mask_classes, a.mask_dir, a.FASTA) == ("predict", "hard", (1, 3), "d", ["x.fa", "y.fa"])
    a = _args(["predict", "m.h5", "x.fa", "--mask_dir", "d", "--mask", "soft"])
    assert (a.mask_dir, a.mask) == ("d", "soft")
    a = _args(["predict", "m.h5", "x.fa"])
    assert getattr(a, "mask_dir", None) is None and getattr(a, "mask_classes", None) is None
    with pytest.raises(SystemExit):
        _args(["predict", "m.h5", "x.fa", "--mask", "medium"])
    with pytest.raises(SystemExit):
        _args(["predict", "m.h5", "x.fa", "--mask_classes", "1,x"])


def _refused(argv, match):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert match in str(e.value)


def test_mask_refusals_before_any_prediction(tmp_path, monkeypatch):
    import deepgrp_amd.model as dgmodel
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGT\n")
    other = tmp_path / "sub"
    other.mkdir()
    (other / "a.fa").write_bytes(b">s\nACGT\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    out = str(tmp_path / "o.tsv")
    mdir = str(tmp_path / "masked")
    loaded = []
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **k: loaded.append(1) or (_ for _ in ()).throw(AssertionError("ran")))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: loaded.append(1) or (_ for _ in ()).throw(AssertionError("ran")))
    _refused(["predict", model, "-", "--mask_dir", mdir, "--output", out], "standard input")
    _refused(["predict", model, str(fa) + ".gz.npz", "--mask_dir", mdir, "--output", out], ".npz")
    _refused(["predict", model, str(fa), str(other / "a.fa"), "--mask_dir", mdir, "--output", out], "same file name")
    _refused(["predict", model, str(fa), "--mask_dir", str(tmp_path), "--output", out], "overwrite the input")
    _refused(["predict", model, str(fa), "--mask", "hard", "--output", out], "need --mask_dir")
    assert not loaded and not os.path.exists(mdir) and not os.path.exists(out)


def test_mask_refuses_labels_the_model_lacks(tmp_path, monkeypatch):
    """The class check needs the model (its class count) and still comes before any prediction."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import pipeline
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGT\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")
    classes = 5

    class Stub:                                             # what predict reads of the model before it builds the pipeline
        input_shape, output_shape = (None, 20, 4), (None, 20, classes)

    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **k: Stub())
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: Stub())
    monkeypatch.setattr(pipeline, "ContigPipeline", lambda *a, **k: (_ for _ in ()).throw(AssertionError("ran")))
    for bad in (f"1,{classes}", "0"):
        _refused(["predict", model, str(fa), "--mask_dir", str(tmp_path / "m"), "--mask_classes", bad, "--output",
                  str(tmp_path / "o.tsv")], "--mask_classes")
    from deepgrp_amd.masking import class_bits
    assert class_bits(None) == (1 << 64) - 2 and class_bits([1, 3]) == 0b1010
    with pytest.raises(ValueError):
        class_bits([0])


def _loop_records(chunk: bytes):
    """fasta.LineLoop over the chunk as `open(path, "r")` reads it."""
    from deepgrp_amd.fasta import LineLoop
    loop = LineLoop()
    lines = io.TextIOWrapper(io.BytesIO(chunk), encoding=None, newline=None)
    return list(loop.feed(lines)) + list(loop.flush())


_ODD = [b" ", b"\t", b"\x0b", b"\x0c", b"\x1c", b"\x1d", b"\x1e", b"\x1f"]


def _random_chunk(rng) -> bytes:
    """A piece of a FASTA file that is not plain: edge whitespace of every kind, lone CR, CRLF, '>' lines after leading spaces,
    headers without a name, text before the first header."""
    out = []
    if rng.random() < 0.5:
        out.append(b"".join(rng.choice(list(b"ACGTacgtNn*-"), size=int(rng.integers(1, 20))).astype(np.uint8).tobytes() for _ in [0]))
    for _r in range(int(rng.integers(1, 5))):
        lead = b"".join(rng.choice(_ODD, size=int(rng.integers(0, 3))))
        name = b"" if rng.random() < 0.15 else b"rec%d x" % int(rng.integers(1000))
        out.append(lead + b">" + name)
        for _l in range(int(rng.integers(0, 6))):
            body = rng.choice(list(b"ACGTacgtNnRY.*"), size=int(rng.integers(1, 40))).astype(np.uint8).tobytes()
            if rng.random() < 0.5:
                k = int(rng.integers(0, len(body) + 1))
                body = body[:k] + b"".join(rng.choice(_ODD, size=int(rng.integers(1, 3)))) + body[k:]  # inner whitespace
            pre = b"".join(rng.choice(_ODD, size=int(rng.integers(0, 3))))
            post = b"".join(rng.choice(_ODD, size=int(rng.integers(0, 3))))
            out.append(pre + body + post)
    ends = [b"\n", b"\r\n", b"\r"]
    text = b""
    for line in out:
        text += line + ends[int(rng.integers(0, 3))]
    if rng.random() < 0.3:
        text = text.rstrip(b"\r\n")                      # no final line end
    return text


def test_sequence_byte_offsets_follow_the_line_loop():
    from deepgrp_amd.masking import sequence_byte_offsets
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(400):
        chunk = _random_chunk(rng)
        want = _loop_records(chunk)
        got = sequence_byte_offsets(chunk)
        assert [h for h, _o in got] == [h for h, _s in want], chunk
        arr = np.frombuffer(chunk, np.uint8)
        for (_h, offs), (_h2, seq) in zip(got, want):
            assert offs is not None
            assert bytes(arr[offs]).upper() == seq.encode(), chunk
            checked += 1
    assert checked > 300


def test_sequence_byte_offsets_cases():
    from deepgrp_amd.masking import sequence_byte_offsets
    got = sequence_byte_offsets(b"junk before\n  >a b\r\n AC gt \rN\x1c\n>\nTT\n>c\n")
    assert [h for h, _o in got] == ["a b", "c"]
    assert got[0][1].tolist() == [21, 22, 23, 24, 25, 28] and got[1][1].size == 0
    assert sequence_byte_offsets(b"ACGT\n") == []
    nonascii = sequence_byte_offsets(b">u\nAC\xc3\xa9GT\n>v\nAC\n")
    assert nonascii[0][0] == "u" and nonascii[0][1] is None and nonascii[1][1].tolist() == [13, 14]
    with pytest.raises(IndexError):
        sequence_byte_offsets(b">a\nAC\n\nGT\n")
    with pytest.raises(IndexError):
        _loop_records(b">a\nAC\n\nGT\n")
