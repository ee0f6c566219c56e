"""predict --track_dir on the CPU: flag parsing, the refusals that come before any device work, the argument checks of
dgrp_track_text / dgrp_track_workspace_bytes, and the numpy statement of the bedGraph format (tracks.reference_text) on cases
written out by hand."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

EINVAL, ENOMEM = -1, -3
P = 0x10000                    # a non-NULL pointer value that is never dereferenced: an earlier check fails


def _args(argv):
    from deepgrp_amd.__main__ import CommandLineParser
    return CommandLineParser().parse_args(argv).args


def test_track_flags_parse_in_both_forms():
    a = _args(["--track_dir", "D", "model.h5", "chr.fa"])                                  # README short form
    assert (a.command, a.track_dir, a.model, a.FASTA) == ("predict", "D", "model.h5", ["chr.fa"])
    a = _args(["--track_classes", "1,3", "--track_digits", "3", "--track_bin", "50", "--track_dir", "D", "-s", "7", "m.h5", "x.fa",
               "y.fa"])
    assert (a.command, a.track_classes, a.track_digits, a.track_bin, a.step_size, a.FASTA) == \
        ("predict", (1, 3), 3, 50, 7, ["x.fa", "y.fa"])
    a = _args(["predict", "m.h5", "-", "--track_dir", "D", "--track_classes", "0"])
    assert (a.track_dir, a.track_classes, a.FASTA) == ("D", (0,), ["-"])
    a = _args(["predict", "m.h5", "x.fa"])
    assert all(getattr(a, k, None) is None for k in ("track_dir", "track_classes", "track_digits", "track_bin"))
    for bad in (["--track_classes", "1,x"], ["--track_digits", "two"], ["--track_bin", "1.5"]):
        with pytest.raises(SystemExit):
            _args(["predict", "m.h5", "x.fa", "--track_dir", "D"] + bad)


def _refused(argv, match):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert match in str(e.value), str(e.value)


def test_track_refusals_before_any_device_work(tmp_path, monkeypatch):
    import deepgrp_amd.model as dgmodel
    from deepgrp_amd import pipeline
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">r\nACGT\n")
    other = tmp_path / "sub"
    other.mkdir()
    (other / "a.fa").write_bytes(b">s\nACGT\n")
    model = os.path.join(GOLDEN, "model_u8_T20.h5")                    # 5 classes
    out = str(tmp_path / "o.tsv")
    tdir = str(tmp_path / "tracks")
    ran = lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work"))
    monkeypatch.setattr(dgmodel, "load_model", ran)
    monkeypatch.setattr(dgmodel, "device_model", ran)
    monkeypatch.setattr(pipeline, "upload_sequence", ran)
    t = ["--track_dir", tdir, "--output", out]
    _refused(["predict", model, str(fa), "--track_classes", "1", "--output", out], "need --track_dir")
    _refused(["predict", model, str(fa), "--track_digits", "2", "--output", out], "need --track_dir")
    _refused(["--track_bin", "5", model, str(fa), "--output", out], "need --track_dir")
    _refused(["predict", model, str(fa), "--track_digits", "0"] + t, "--track_digits")
    _refused(["predict", model, str(fa), "--track_digits", "5"] + t, "--track_digits")
    _refused(["predict", model, str(fa), "--track_bin", "0"] + t, "--track_bin")
    _refused(["predict", model, str(fa), "--track_bin", "-3"] + t, "--track_bin")
    _refused(["predict", model, str(fa), "--track_classes", "1,5"] + t, "--track_classes: label 5")
    _refused(["predict", model, str(fa), "--track_classes", "-1"] + t, "--track_classes: label -1")
    _refused(["predict", model, str(fa), str(other / "a.fa")] + t, "same file name")
    _refused(["predict", model, str(fa), str(fa)] + t, "same file name")
    _refused(["predict", model, "-", "-"] + t, "same file name")
    _refused(["--track_dir", tdir, "evaluate", model, str(fa), str(fa), "--output", out], "belongs to predict")
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(["predict", model, str(fa)] + t, "WORLD_SIZE")
    assert not os.path.exists(tdir) and not os.path.exists(out)


def test_track_plan_names_and_classes(tmp_path):
    from deepgrp_amd import tracks
    a = _args(["predict", "m.h5", "-", str(tmp_path / "x.fa.gz"), "--track_dir", str(tmp_path / "T")])
    p = tracks.plan(a)
    assert p.bases == {"-": "stdin", str(tmp_path / "x.fa.gz"): "x.fa.gz"} and (p.digits, p.bin, p.classes) == (2, 1, None)
    assert tracks.resolve(p, 5).classes == (1, 2, 3, 4)
    assert tracks.resolve(p._replace(classes=(3, 0, 3)), 5).classes == (3, 0)
    assert tracks.track_path("T", "x.fa.gz", 2) == os.path.join("T", "x.fa.gz.class2.bedGraph")


# ---------------------------------------------------------------- the C ABI
def _lib():
    from deepgrp_amd._lib import lib
    return lib()


def _track_call(n=100, Cn=5, cls=1, digits=2, bin=1, offset=0, name=b"chr1", name_len=None, text=P, cap=1 << 20, h=True,
                probs=P, work=P, wb=1 << 30):
    hb = C.pointer(C.c_int64(-7)) if h else None
    return _lib().dgrp_track_text(probs, n, Cn, cls, digits, bin, offset, name, len(name or b"") if name_len is None else name_len,
                                  text, cap, hb, work, wb, None)


@pytest.mark.parametrize("kw,match", [
    (dict(n=-1), "bad n"), (dict(n=1 << 50), "bad n"),
    (dict(Cn=0), "bad C/cls"), (dict(Cn=65), "bad C/cls"), (dict(cls=5), "bad C/cls"), (dict(cls=-1), "bad C/cls"),
    (dict(digits=0), "digits"), (dict(digits=5), "digits"),
    (dict(bin=0), "bad bin"), (dict(bin=-4), "bad bin"), (dict(offset=-1), "bad offset"),
    (dict(cap=-1), "name_len/cap"), (dict(name_len=-2), "name_len/cap"),
    (dict(probs=None), "NULL pointer"), (dict(work=None), "NULL pointer"), (dict(text=None), "NULL pointer"),
    (dict(name=None, name_len=3), "NULL pointer"), (dict(h=False), "NULL h_bytes"),
])
def test_track_text_argument_checks(kw, match):
    rc = _track_call(**kw)
    assert rc == EINVAL
    assert match in _lib().dgrp_last_error().decode()


def test_track_text_without_device_work():
    L = _lib()
    assert L.dgrp_track_workspace_bytes(-1, 1) == 0 and L.dgrp_track_workspace_bytes(10, 0) == 0
    assert L.dgrp_track_workspace_bytes(1 << 50, 1) == 0
    ws = L.dgrp_track_workspace_bytes
    # 4 bytes per bin at least; never less for a longer record, never more for a wider bin
    ns, bins = (1, 63, 1000, 2047, 2048, 2049, 100_000, 10_000_000), (1, 2, 7, 50, 64, 65, 1000)
    assert all(ws(n, 1) >= 4 * n for n in ns)
    assert all(ws(a, b) <= ws(a2, b) for b in bins for a, a2 in zip(ns, ns[1:]))
    assert all(ws(n, b) >= ws(n, b2) for n in ns for b, b2 in zip(bins, bins[1:]))
    assert ws(1000, 50) > 0
    assert ws(1 << 39, 1) == 0 and ws(1 << 40, 4) > 0                  # the 2^39 bins of one call
    h = C.c_int64(-7)
    # an empty record writes nothing (NULL buffers are fine); a workspace below the bound is refused before any launch
    assert L.dgrp_track_text(None, 0, 5, 1, 2, 1, 3, b"x", 1, None, 0, C.byref(h), None, 0, None) == 0 and h.value == 0
    assert _track_call(wb=L.dgrp_track_workspace_bytes(100, 1) - 1) == ENOMEM
    assert "workspace" in L.dgrp_last_error().decode()
    assert "dgrp_track_text" in __import__("deepgrp_amd._lib", fromlist=["exported_symbols"]).exported_symbols()


def test_track_text_name_room():
    """A name of exactly DGRP_TRACK_NAME_ROOM bytes passes the argument checks (the workspace check is what refuses this call);
    one byte more is a bad argument, and the message names the limit."""
    L = _lib()
    room = 65536
    short = L.dgrp_track_workspace_bytes(100, 1) - 1
    assert _track_call(name=b"x" * room, wb=short) == ENOMEM
    assert "workspace" in L.dgrp_last_error().decode()
    assert _track_call(name=b"x" * (room + 1), wb=short) == EINVAL
    msg = L.dgrp_last_error().decode()
    assert "name" in msg and str(room) in msg, msg


# ---------------------------------------------------------------- the format, stated in numpy
def test_reference_text_by_hand():
    from deepgrp_amd.tracks import quantise, reference_text
    f = lambda *v: np.array(v, np.float32)
    # base resolution: runs of equal value are one line, zeros are gaps, coordinates start at startpos
    col = f(0, 0.25, 0.25, 0.001, 0, 1.0, 1.0, 0.5)
    assert reference_text(col, 10, b"chr1") == (b"chr1\t11\t13\t0.25\n"
                                                b"chr1\t15\t17\t1.00\n"
                                                b"chr1\t17\t18\t0.50\n")
    # 0.001 rounds to 0 at two digits but not at three; 0.125 -> 0.13 (half up); values print from the integer
    assert reference_text(f(0.001, 0.125), 0, b"r", digits=3) == b"r\t0\t1\t0.001\nr\t1\t2\t0.125\n"
    assert reference_text(f(0.125, 0.125), 0, b"r", digits=2) == b"r\t0\t2\t0.13\n"
    assert reference_text(f(0.96, 0.05), 0, b"r", digits=1) == b"r\t0\t1\t1.0\nr\t1\t2\t0.1\n"
    assert reference_text(f(0.5), 0, b"r", digits=4) == b"r\t0\t1\t0.5000\n"
    # bins aligned to the coordinate: startpos 7, bin 5 -> [7,10) [10,15) [15,17); a bin's value is its maximum
    col = f(0.1, 0.3, 0.2, 0, 0, 0.3, 0, 0, 0, 0.7)
    assert reference_text(col, 7, b"c", bin=5) == b"c\t7\t15\t0.30\nc\t15\t17\t0.70\n"
    assert reference_text(col, 7, b"c", bin=100) == b"c\t7\t17\t0.70\n"
    # raw name bytes, an empty record, a record of zeros
    assert reference_text(f(1.0), 0, "caf\udce9".encode("utf-8", "surrogateescape")) == b"caf\xe9\t0\t1\t1.00\n"
    assert reference_text(f(), 5, b"x") == b"" and reference_text(np.zeros(9, np.float32), 5, b"x") == b""
    # the two float32 roundings: 0.005f * 100 rounds up to 0.5 before the +0.5, so 0.005 -> 0.01; 0.00499999 stays 0
    assert quantise(f(0.005), 2)[0] == 1 and quantise(f(0.00499), 2)[0] == 0
    assert list(quantise(f(0, 1, 0.5, 0.95), 1)) == [0, 10, 5, 10]
