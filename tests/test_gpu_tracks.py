"""predict --track_dir on the GPU: dgrp_track_text against the numpy statement of the format (tracks.reference_text) byte for byte,
the command line's track files against that statement applied to ContigPipeline.merged of every record, in every input form and
mode, and the TSV and masked FASTA unchanged by the flag."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SCAN_TILE = 2048


def _kernel_text(probs: torch.Tensor, startpos, name: bytes, cls, digits, bin, cap=None):
    """dgrp_track_text on a device [n, C] array; with `cap` first at that capacity (must be too small: *h_bytes is still the full
    length and nothing is written), then with exactly the room reported."""
    from deepgrp_amd._lib import check, lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    n, c = probs.shape
    wb = L.dgrp_track_workspace_bytes(n, bin)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=probs.device)
    total = C.c_int64(-1)
    if cap is not None:
        text = torch.full((max(cap, 1),), 0x5A, dtype=torch.uint8, device=probs.device)
        check(L.dgrp_track_text(probs.data_ptr(), n, c, cls, digits, bin, startpos, name, len(name), text.data_ptr(), cap,
                                C.byref(total), work.data_ptr(), wb, stream_ptr()), "dgrp_track_text")
        assert total.value > cap
        assert bool((text == 0x5A).all()), "a too-small buffer was written"
    size = total.value if cap is not None else (1 << 22)
    text = torch.empty(max(size, 1), dtype=torch.uint8, device=probs.device)
    check(L.dgrp_track_text(probs.data_ptr(), n, c, cls, digits, bin, startpos, name, len(name), text.data_ptr(), size,
                            C.byref(total), work.data_ptr(), wb, stream_ptr()), "dgrp_track_text")
    assert total.value <= size
    return text[:total.value].cpu().numpy().tobytes()


def _boundary_values(rng, n, digits):
    """float32 neighbours of (k + 0.5) / 10^D (the rounding boundaries), 0 and 1."""
    k = rng.integers(0, 10 ** digits, size=n)
    mid = ((k + 0.5) / 10 ** digits).astype(np.float32)
    step = rng.integers(-1, 2, size=n)
    v = np.where(step < 0, np.nextafter(mid, np.float32(0)), np.where(step > 0, np.nextafter(mid, np.float32(1)), mid))
    pick = rng.random(n)
    v = np.where(pick < 0.1, np.float32(0), np.where(pick < 0.2, np.float32(1), v))
    return np.clip(v, 0, 1).astype(np.float32)


def _column(rng, style, n, digits):
    if style == "runs":                                    # long constant runs, some of them 0
        out = np.empty(n, np.float32)
        p = 0
        while p < n:
            ln = int(rng.integers(1, 400))
            out[p:p + ln] = 0 if rng.random() < 0.3 else rng.choice([rng.random(), 1.0, 0.5])
            p += ln
        return out
    if style == "noise":
        return rng.random(n).astype(np.float32)
    return _boundary_values(rng, n, digits)


NAMES = [b"chr1", b"caf\xe9 \xff\xfe-\xc3\xa9", b"scaffold_" + b"x" * 300]


def test_track_kernel_against_the_statement():
    from deepgrp_amd.tracks import reference_text
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    checked = lines = 0
    for Cn in (2, 5, 16):
        for digits in (1, 2, 3, 4):
            for bin in (1, 7, 50):
                for n in sorted({1, max(bin - 1, 1), SCAN_TILE - 1, SCAN_TILE + 1, 3 * SCAN_TILE * bin + 5}):
                    style = ("runs", "noise", "edges")[checked % 3]
                    arr = rng.random((n, Cn)).astype(np.float32)
                    cls = int(rng.integers(0, Cn))
                    arr[:, cls] = _column(rng, style, n, digits)
                    startpos = int(rng.choice([0, bin * 3 + 1, 123_457, 10 ** 11 + 3]))
                    name = NAMES[checked % len(NAMES)]
                    want = reference_text(arr[:, cls], startpos, name, digits, bin)
                    got = _kernel_text(torch.from_numpy(arr).to(dev), startpos, name, cls, digits, bin,
                                       cap=len(want) // 2 if checked % 4 == 0 and len(want) > 2 else None)
                    assert got == want, (Cn, digits, bin, n, style, startpos)
                    checked += 1
                    lines += want.count(b"\n")
    assert checked > 150 and lines > 100_000


def _exact_text(L, probs, startpos, name, cls, digits, bin):
    """dgrp_track_text in a workspace of exactly dgrp_track_workspace_bytes(n, bin) bytes and a text buffer of exactly the length
    a first call (cap 0) reports."""
    from deepgrp_amd._lib import check
    from deepgrp_amd.pipeline import stream_ptr
    n, c = probs.shape
    wb = L.dgrp_track_workspace_bytes(n, bin)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=probs.device)
    total = C.c_int64(-1)
    text = torch.empty(1, dtype=torch.uint8, device=probs.device)
    for _ in range(2):
        check(L.dgrp_track_text(probs.data_ptr(), n, c, cls, digits, bin, startpos, name, len(name), text.data_ptr(), max(total.value, 0),
                                C.byref(total), work.data_ptr(), wb, stream_ptr()), "dgrp_track_text")
        if total.value > 0 and text.numel() != total.value:
            text = torch.empty(total.value, dtype=torch.uint8, device=probs.device)
    return text[:total.value].cpu().numpy().tobytes()


def test_track_kernel_long_names():
    """Names of 300 bytes and of exactly the name room through the one-record entry: the ten lines of the first are assembled in
    the write kernel's staging area, those of the second (655 KB) pass its size and take the direct (unstaged) branch."""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.tracks import reference_text
    L = lib()
    rng = np.random.default_rng(11)
    n, Cn, bin = 65, 2, 7
    arr = rng.random((n, Cn)).astype(np.float32)
    d = torch.from_numpy(arr).cuda()
    for name in (b"n" * 300, bytes(rng.integers(33, 127, 65536, dtype=np.uint8))):
        for cls in range(Cn):
            want = reference_text(arr[:, cls], 3, name, 2, bin)
            assert want.count(b"\n") == 10                          # noise: every bin its own line
            assert _exact_text(L, d, 3, name, cls, 2, bin) == want, (len(name), cls)


def test_track_kernel_offsets_in_the_exact_workspace():
    """Every offset, in a workspace of exactly the query's size: the shapes where the offset-free bin bound, the tile rounding and
    the lane / wave switch could disagree with the call."""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.tracks import reference_text
    L = lib()
    rng = np.random.default_rng(12)
    checked = lines = 0
    for n in (1, 63, 64, 65, 2049):
        arr = rng.random((n, 2)).astype(np.float32)
        arr[:, 1] = _column(rng, "runs", n, 2)
        d = torch.from_numpy(arr).cuda()
        for bin in (1, 7, 200):
            for startpos in (0, bin * 3 + bin // 2, 10 ** 11 + 3):
                for cls in (0, 1):
                    want = reference_text(arr[:, cls], startpos, b"chr1", 2, bin)
                    assert _exact_text(L, d, startpos, b"chr1", cls, 2, bin) == want, (n, bin, startpos, cls)
                    checked += 1
                    lines += want.count(b"\n")
    assert checked == 90 and lines > 3000


def test_track_kernel_tens_of_mbp():
    """One record of 40 Mbp (runs, a stretch of noise, boundary values) at base resolution and at bin 50, name with non-ASCII."""
    from deepgrp_amd.tracks import reference_text
    rng = np.random.default_rng(9)
    n, Cn, cls = 40_000_000, 5, 3
    col = np.repeat(np.where(rng.random(40_000) < 0.4, 0, rng.random(40_000)).astype(np.float32), 1000)
    col[5_000_000:5_300_000] = rng.random(300_000)
    col[20_000_000:20_100_000] = _boundary_values(rng, 100_000, 2)
    d = torch.zeros((n, Cn), dtype=torch.float32, device="cuda")
    d[:, cls] = torch.from_numpy(col).cuda()
    name = b"chr\xce\xb1 2"
    for bin in (1, 50):
        want = reference_text(col, 77, name, 2, bin)
        assert _kernel_text(d, 77, name, cls, 2, bin, cap=1000 if bin == 1 else None) == want
    assert want.count(b"\n") > 10_000


def test_track_kernel_index_beyond_2_to_32():
    """Rows whose element index i * C + c passes 2^32 (16 classes, 280 M rows): the values there reach the text."""
    n, Cn, cls = 280_000_000, 16, 15
    d = torch.zeros((n, Cn), dtype=torch.float32, device="cuda")
    a = (1 << 32) // Cn + 1000
    d[a:a + 500, cls] = 0.5
    d[n - 1, cls] = 1.0
    d[5, cls] = 0.25
    got = _kernel_text(d, 3, b"big", cls, 2, 1)
    assert got == (b"big\t8\t9\t0.25\n" + b"big\t%d\t%d\t0.50\n" % (a + 3, a + 503) + b"big\t%d\t%d\t1.00\n" % (n + 2, n + 3))
    del d
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the command line
def _write_fasta(path, records):
    with open(path, "wb") as fh:
        for h, s in records:
            fh.write(b">" + h + b"\n" + b"\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + b"\n")


def _records(rng, T):
    """Leading, trailing and interior N, records shorter than the window, a header with non-ASCII characters (UTF-8: the
    reference's loop reads text)."""
    from deepgrp_amd import synthetic
    g = synthetic.synthetic_chromosome(60_000, contig=3, flank=800)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    return [(b"chr1 first record", g),
            (b"tiny", r(T - 5)),
            ("nn\u03b1\u00e9 desc".encode(), b"N" * 37 + r(3000) + b"N" * 500 + r(2000) + b"N" * 11),
            (b"short2", b"NN" + r(T + 3)),
            (b"last", g[10_000:31_000])]


def _expected(model_file, records, flags, spec, fast):
    """{class: bytes} by the statement, from ContigPipeline.merged of every record."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.pipeline import ContigPipeline, upload_sequence
    from deepgrp_amd.tracks import reference_text
    model = dgmodel.load_model(model_file)
    pipe = ContigPipeline(model, flags.get("-s", 50), 256, 50, 50, use_mss=True, fast=fast)
    out = {c: [] for c in spec["classes"]}
    for name, seq in records:
        st, d_idx = upload_sequence(seq)
        merged = pipe.merged(d_idx).cpu().numpy()
        for c in spec["classes"]:
            out[c].append(reference_text(merged[:, c], st, name, spec["digits"], spec["bin"]))
    return {c: b"".join(v) for c, v in out.items()}


def _trained_model(tmp_path):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import synthetic
    w = synthetic.trained_weights()
    path = str(tmp_path / "trained.h5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path, 200


def _npz(path, seq: bytes):
    idx = np.frombuffer(seq, np.uint8)
    code = np.full(256, 4, np.int64)
    code[[65, 67, 71, 84]] = [0, 1, 2, 3]
    fwd = np.zeros((5, idx.size), np.int8)
    fwd[code[idx], np.arange(idx.size)] = 1
    np.savez_compressed(path, fwd=fwd)


@pytest.mark.parametrize("which", ["trained", "attention"])
def test_cli_tracks_every_input_and_mode(tmp_path, monkeypatch, which):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    if which == "trained":
        model_file, T = _trained_model(tmp_path)
    else:
        model_file, T = os.path.join(GOLDEN, "model_u60_T342_att.h5"), 342
    rng = np.random.default_rng(17)
    records = _records(rng, T)
    fa = tmp_path / "in.fa"
    _write_fasta(fa, records)
    fagz = tmp_path / "in.fa.gz"
    fagz.write_bytes(gz.bgzf_compress(fa.read_bytes(), block=7000))
    npz = tmp_path / "chrQ.fa.gz.npz"
    _npz(npz, records[2][1])
    modes = [
        ("default", [], str(fa), dict(classes=(1, 2, 3, 4), digits=2, bin=1)),
        ("m", ["-m"], str(fa), dict(classes=(0, 2), digits=3, bin=7)),
        ("fast", ["--fast"], str(fa), dict(classes=(1, 4), digits=2, bin=50)),
        ("vv", ["-vv"], str(fa), dict(classes=(1, 2, 3, 4), digits=4, bin=1)),
        ("bgzf", [], str(fagz), dict(classes=(2,), digits=1, bin=1)),
        ("npz", [], str(npz), dict(classes=(1, 3), digits=2, bin=7)),
        ("stdin", [], "-", dict(classes=(1, 2, 3, 4), digits=2, bin=1)),
    ]
    for label, extra, inp, spec in modes:
        tflags = ["--track_dir", str(tmp_path / label), "--track_digits", str(spec["digits"]), "--track_bin", str(spec["bin"])]
        if spec["classes"] != (1, 2, 3, 4):
            tflags += ["--track_classes", ",".join(map(str, spec["classes"]))]
        outs = {}
        for tag, more in (("plain", []), ("tracks", tflags)):
            if inp == "-":
                monkeypatch.setattr(sys, "stdin", io.StringIO(fa.read_text(errors="surrogateescape")))
            tsv = tmp_path / f"{label}.{tag}.tsv"
            v = [a for a in extra if a == "-vv"]
            main(v + ["predict", model_file, inp, "--output", str(tsv)] + [a for a in extra if a != "-vv"] + more)
            outs[tag] = tsv.read_bytes()
        main(["predict", model_file, str(fa), "--output", str(tmp_path / "reset.tsv")])    # (logging back to the default level)
        assert outs["tracks"] == outs["plain"], label
        assert outs["plain"].count(b"\n") > 0 or label == "npz"
        recs = [(b"chrQ", records[2][1])] if label == "npz" else [(h.split()[0], s) for h, s in records]
        want = _expected(model_file, recs, {}, spec, fast=label == "fast")
        base = "stdin" if inp == "-" else os.path.basename(inp)
        assert sorted(os.listdir(tmp_path / label)) == sorted(f"{base}.class{c}.bedGraph" for c in spec["classes"]), label
        for c in spec["classes"]:
            got = (tmp_path / label / f"{base}.class{c}.bedGraph").read_bytes()
            assert got == want[c], (label, c)
        assert sum(len(v) for v in want.values()) > 0, label


def test_cli_tracks_fp32_only_model(tmp_path):
    """A model with more units than the fused kernels take runs on the plain-fp32 kernels; its tracks follow its merged array."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    w = synthetic.synthetic_weights(288, 4, False, seed=3, gain=3.0)
    model_file = str(tmp_path / "u288.h5")
    dgmodel.save_keras_hdf5(model_file, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=40)
    assert getattr(dgmodel.load_model(model_file), "fp32_only", False)
    rng = np.random.default_rng(4)
    records = [(b"a", b"NN" + rng.choice(list(b"ACGT"), size=3000).astype(np.uint8).tobytes()),
               (b"b", rng.choice(list(b"ACGT"), size=35).astype(np.uint8).tobytes())]
    fa = tmp_path / "u.fa"
    _write_fasta(fa, records)
    main(["-s", "9", "predict", model_file, str(fa), "--output", str(tmp_path / "p.tsv")])
    main(["-s", "9", "predict", model_file, str(fa), "--output", str(tmp_path / "t.tsv"), "--track_dir", str(tmp_path / "T")])
    assert (tmp_path / "p.tsv").read_bytes() == (tmp_path / "t.tsv").read_bytes()
    want = _expected(model_file, records, {"-s": 9}, dict(classes=(1, 2, 3), digits=2, bin=1), fast=False)
    for c in (1, 2, 3):
        assert (tmp_path / "T" / f"u.fa.class{c}.bedGraph").read_bytes() == want[c]
    assert len(want[1]) > 0


def test_cli_tracks_leave_tsv_and_masks_alone_on_many_short_records(tmp_path):
    """A file of many short records runs as batches without --track_dir and record by record with it: the same TSV, the same
    masked FASTA."""
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    model_file, _T = _trained_model(tmp_path)
    raw = synthetic.synthetic_chromosome(400_000, contig=2, flank=1000)[2000:-2000]
    recs = [(b"ctg%d" % k, raw[k * 3000:(k + 1) * 3000 - (k % 7) * 300]) for k in range(120)]
    fa = tmp_path / "asm.fa"
    _write_fasta(fa, recs)
    for extra in ([], ["-m"], ["--fast"]):
        main(["predict", model_file, str(fa), "--output", str(tmp_path / "p.tsv"), "--mask_dir", str(tmp_path / "mp")] + extra)
        main(["predict", model_file, str(fa), "--output", str(tmp_path / "t.tsv"), "--mask_dir", str(tmp_path / "mt"),
              "--track_dir", str(tmp_path / "T"), "--track_bin", "50"] + extra)
        assert (tmp_path / "t.tsv").read_bytes() == (tmp_path / "p.tsv").read_bytes(), extra
        assert (tmp_path / "mt" / "asm.fa").read_bytes() == (tmp_path / "mp" / "asm.fa").read_bytes(), extra
        assert (tmp_path / "p.tsv").read_bytes().count(b"\n") > 20
        got = (tmp_path / "T" / "asm.fa.class1.bedGraph").read_bytes()
        want = _expected(model_file, recs, {}, dict(classes=(1,), digits=2, bin=50), fast="--fast" in extra)[1]
        assert got == want and got


def test_cli_tracks_failure_leaves_only_finished_inputs(tmp_path):
    """An all-N record in the second input stops predict as before; the first input's tracks are in place, nothing of the second."""
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    rng = np.random.default_rng(2)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    good, bad = tmp_path / "good.fa", tmp_path / "bad.fa"
    _write_fasta(good, [(b"g1", r(800)), (b"g2", r(300))])
    _write_fasta(bad, [(b"b1", r(700)), (b"allN", b"N" * 40), (b"b3", r(500))])
    tdir = tmp_path / "T"
    for vv in ([], ["-vv"]):
        with pytest.raises(ValueError, match="negative dimensions"):
            main(vv + ["predict", model_file, str(good), str(bad), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir)])
        main(["predict", model_file, str(good), "--output", str(tmp_path / "reset.tsv")])
        assert sorted(os.listdir(tdir)) == [f"good.fa.class{c}.bedGraph" for c in (1, 2, 3, 4)], vv
        for c in (1, 2, 3, 4):
            os.remove(tdir / f"good.fa.class{c}.bedGraph")
