"""`evaluate` on the CPU: the annotation parser against a plain line loop, the command line's refusals before any GPU work, and
the report (TSV and JSON) against prediction._calculate_metrics."""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

MODEL_H5 = os.path.join(GOLDEN, "model_u60_T342_att.h5")       # 5 classes


def _loop(path, repeats):
    out = {}
    for line in open(path):
        c = line.split()
        if not c or c[0].startswith("#"):
            continue
        if int(c[3]) in repeats:
            out.setdefault(c[0], []).append((int(c[1]), int(c[2]), int(c[3])))
    return out


@pytest.mark.parametrize("repeats", [(1, 2, 3, 4), (1, 3), (2,), tuple(range(1, 20))])
def test_read_annotation_vs_line_loop(repeats):
    from deepgrp_amd.evaluation import read_annotation
    path = os.path.join(GOLDEN, "parse_rm_expect.bed")
    got = read_annotation(path, repeats)
    want = _loop(path, repeats)
    assert sorted(got) == sorted(want)
    for name, rows in want.items():
        g = got[name]
        assert list(zip(g["start"].tolist(), g["end"].tolist(), g["label"].tolist())) == rows
        for number in repeats:
            assert int((g["label"] == number).sum()) == sum(1 for r in rows if r[2] == number)


def test_read_annotation_comments_blank_lines_and_extra_columns(tmp_path):
    from deepgrp_amd.evaluation import read_annotation
    p = tmp_path / "a.bed"
    p.write_text("# header\n\nchr1\t10\t20\t1\tL1\tLINE\n   \n  # indented comment\nchr2 5 5 2\nchr1\t0\t3\t4\n#chr1\t0\t9\t1\n"
                 "chr1\t1\t2\t7\n")
    got = read_annotation(str(p), [1, 2, 3, 4])
    assert sorted(got) == ["chr1", "chr2"]
    assert got["chr1"][["start", "end", "label"]].tolist() == [(10, 20, 1), (0, 3, 4)]
    assert got["chr2"][["start", "end", "label"]].tolist() == [(5, 5, 2)]
    assert read_annotation(str(p), [5]) == {}


@pytest.mark.parametrize("bad,why", [("chr1\t-1\t5\t1", "negative begin"), ("chr1\t9\t5\t1", "end below begin"),
                                     ("chr1\t1.5\t5\t1", "begin"), ("chr1\t1\tx\t1", "end"), ("chr1\t1\t5\tAlu", "repeat number"),
                                     ("chr1\t1\t5", "expected")])
def test_read_annotation_errors_name_the_line(tmp_path, bad, why):
    from deepgrp_amd.evaluation import AnnotationError, read_annotation
    p = tmp_path / "a.bed"
    p.write_text("# x\nchr1\t0\t4\t1\n\n" + bad + "\nchr1\t8\t9\t2\n")
    with pytest.raises(AnnotationError) as e:
        read_annotation(str(p), [1, 2])
    assert f"{p}:4:" in str(e.value) and why in str(e.value)


def test_read_annotation_is_vectorised(tmp_path):
    """200 k lines of three contigs: every kept row, grouped by contig in file order (the numeric columns are parsed in one pass)."""
    from deepgrp_amd.evaluation import read_annotation
    rng = np.random.default_rng(3)
    n = 200_000
    b = rng.integers(0, 10**8, n)
    lines = "".join(f"chr{k % 3}\t{x}\t{x + 100}\t{k % 5}\tname\tfam\n" for k, x in enumerate(b))
    p = tmp_path / "big.bed"
    p.write_text(lines)
    got = read_annotation(str(p), [1, 2, 3, 4])
    assert sorted(got) == ["chr0", "chr1", "chr2"]
    for c in range(3):
        k = np.arange(c, n, 3)
        k = k[k % 5 != 0]
        g = got[f"chr{c}"]
        assert np.array_equal(g["start"], b[k]) and np.array_equal(g["end"], b[k] + 100) and np.array_equal(g["label"], k % 5)


# ------------------------------------------------------------------------- command line
def test_evaluate_parses():
    from deepgrp_amd.__main__ import CommandLineParser
    a = CommandLineParser().parse_args(["-s", "25", "-l", "30", "evaluate", "m.h5", "ann.bed", "a.fa", "b.fa", "-m", "--fast",
                                        "--repeats", "1,3", "--min_overlap", "0.25", "--output", "r.tsv", "--json", "r.json"]).args
    assert a.command == "evaluate" and a.model == "m.h5" and a.annotation == "ann.bed" and a.FASTA == ["a.fa", "b.fa"]
    assert a.no_use_mss and a.fast and a.repeats == (1, 3) and a.min_overlap == 0.25 and a.output == "r.tsv" and a.json == "r.json"
    assert a.step_size == 25 and a.min_mss_length == 30
    d = CommandLineParser().parse_args(["evaluate", "m.h5", "ann.bed", "a.fa"]).args
    assert d.repeats is None and d.min_overlap == 0.5 and d.output == "-" and d.json is None and not d.no_use_mss


def test_readme_form_does_not_prepend_predict():
    from deepgrp_amd.__main__ import CommandLineParser
    a = CommandLineParser().parse_args(["-x", "40", "evaluate", "m.h5", "ann.bed", "a.fa"]).args
    assert a.command == "evaluate" and a.xdrop_length == 40
    assert CommandLineParser().parse_args(["m.h5", "a.fa"]).args.command == "predict"


@pytest.mark.parametrize("repeats", ["0", "5", "1,2,9"])
def test_repeats_outside_the_model_are_refused_on_the_host(tmp_path, monkeypatch, repeats):
    """The class count comes from the HDF5 file on the host; nothing reaches the GPU (the library is not even called)."""
    from deepgrp_amd import pipeline
    from deepgrp_amd.__main__ import main
    monkeypatch.setattr(pipeline, "require_gpu", lambda: pytest.fail("GPU touched"))
    monkeypatch.setattr(pipeline, "DeviceModel", lambda *a, **k: pytest.fail("GPU touched"))
    ann = tmp_path / "a.bed"
    ann.write_text("chr1\t0\t10\t1\n")
    with pytest.raises(SystemExit) as e:
        main(["evaluate", MODEL_H5, str(ann), str(tmp_path / "x.fa"), "--repeats", repeats])
    assert "not a repeat class" in str(e.value.code) and "1..4" in str(e.value.code)


def test_bad_annotation_and_overlap_are_refused_on_the_host(tmp_path, monkeypatch):
    from deepgrp_amd import pipeline
    from deepgrp_amd.__main__ import main
    monkeypatch.setattr(pipeline, "DeviceModel", lambda *a, **k: pytest.fail("GPU touched"))
    ann = tmp_path / "a.bed"
    ann.write_text("chr1\t0\t10\t1\nchr1\t20\t10\t2\n")
    with pytest.raises(SystemExit) as e:
        main(["evaluate", MODEL_H5, str(ann), "x.fa"])
    assert f"{ann}:2:" in str(e.value.code)
    for theta in ("0", "1.5", "-0.1"):
        with pytest.raises(SystemExit) as e:
            main(["evaluate", MODEL_H5, str(ann), "x.fa", "--min_overlap", theta])
        assert "--min_overlap" in str(e.value.code)


def test_world_size_two_is_refused(tmp_path, monkeypatch):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", lambda *a, **k: pytest.fail("went past the WORLD_SIZE check"))
    with pytest.raises(SystemExit) as e:
        main(["evaluate", MODEL_H5, "ann.bed", "x.fa"])
    assert "WORLD_SIZE" in str(e.value.code)


# ------------------------------------------------------------------------- report
def _acc(cnf, elements, found, segments, supported, theta=0.5):
    from deepgrp_amd.evaluation import Accumulator
    C = len(cnf)
    a = Accumulator(C, theta)
    a.cnf[:] = cnf
    a.bases = int(np.sum(cnf))
    a.elements[:], a.found[:], a.segments[:], a.supported[:] = elements, found, segments, supported
    return a


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_report_numbers_equal_calculate_metrics(seed):
    from deepgrp_amd.evaluation import report, tsv_report
    from deepgrp_amd.prediction import _calculate_metrics
    rng = np.random.default_rng(seed)
    C = 5
    cnf = rng.integers(0, 10**7, (C, C))
    if seed == 1:
        cnf[3, :] = 0                      # a class without truth: TPR 0/0
        cnf[:, 3] = 0                      # and never predicted: PPV 0/0
    el = rng.integers(0, 100, C)
    el[0] = 0
    fo = np.minimum(el, rng.integers(0, 100, C))
    sg = rng.integers(0, 100, C)
    sg[0] = 0
    su = np.minimum(sg, rng.integers(0, 100, C))
    rep = report(_acc(cnf, el, fo, sg, su), dict(model="m.h5"))
    with np.errstate(divide="ignore", invalid="ignore"):
        want = _calculate_metrics(cnf)
    js = json.loads(json.dumps(rep, allow_nan=False))
    assert js["model"] == "m.h5" and js["classes"] == C and js["bases"] == int(cnf.sum())
    assert js["confusion_matrix"] == cnf.tolist()
    for k, v in want.items():
        got = js["metrics"][k]
        vals = np.asarray(v, float).ravel()
        gl = got if isinstance(got, list) else [got]
        assert len(gl) == vals.size
        for g, w in zip(gl, vals):
            assert (g is None and math.isnan(w)) or g == float(w), k
    assert js["metrics"]["TotalACC"] == np.trace(cnf) / cnf.sum()
    assert js["elements"] == el.tolist() and js["found"] == fo.tolist() and js["segments"] == sg.tolist()
    assert js["supported"] == su.tolist() and js["min_overlap"] == 0.5

    lines = tsv_report(rep).splitlines()
    assert lines[0] == "#class\ttrue_bases\tpredicted_bases\tTP\tFP\tFN\tTPR\tPPV\tF1\telements\tfound\tsegments\tsupported"
    assert len(lines) == 1 + C + 2
    for c in range(C):
        f = lines[1 + c].split("\t")
        tp = int(cnf[c, c])
        assert [int(x) for x in f[:6]] == [c, int(cnf[c].sum()), int(cnf[:, c].sum()), tp, int(cnf[:, c].sum()) - tp,
                                          int(cnf[c].sum()) - tp]
        for x, key in zip(f[6:9], ("TPR", "PPV", "F1")):
            w = float(want[key][c])
            assert x == repr(w)                            # 'nan' for NaN, exact digits otherwise
        assert [int(x) for x in f[9:]] == [int(el[c]), int(fo[c]), int(sg[c]), int(su[c])]
    assert lines[-2] == "#TotalACC\t" + repr(float(np.trace(cnf) / cnf.sum()))
    assert lines[-1] == "#MCC\t" + repr(float(want["MCC"]))
    if seed == 1:
        assert lines[4].split("\t")[6:9] == ["nan", "nan", "nan"]
        assert js["metrics"]["TPR"][3] is None and js["metrics"]["PPV"][3] is None and js["metrics"]["F1"][3] is None


def test_report_of_nothing_is_nan_not_an_error():
    from deepgrp_amd.evaluation import report, tsv_report
    rep = report(_acc(np.zeros((3, 3), np.int64), [0] * 3, [0] * 3, [0] * 3, [0] * 3), {})
    assert rep["metrics"]["TotalACC"] is None and rep["metrics"]["MCC"] is None
    assert tsv_report(rep).splitlines()[-1] == "#MCC\tnan"
    json.dumps(rep, allow_nan=False)


def test_synthetic_annotation_is_the_planted_truth():
    from deepgrp_amd import synthetic
    from deepgrp_amd.preprocessing import preprocess_y
    import tempfile
    n = 300_000
    lines = synthetic.synthetic_annotation(n, contig=4, name="chrS", flank=2000)
    _idx, lab = synthetic.synthetic_truth(n, contig=4, flank=2000)
    with tempfile.NamedTemporaryFile("w", suffix=".bed", delete=False) as fh:
        fh.writelines(lines)
    try:
        y = preprocess_y(fh.name, "chrS", n, [1, 2, 3, 4]).argmax(axis=0)
    finally:
        os.remove(fh.name)
    assert len(lines) > 10 and (y == lab).all()


@pytest.mark.parametrize("filename,header,name", [
    ("chr.fa", "chr1", "chr1"), ("chr.fa", "chr2 assembled 2009", "chr2"), ("-", "scaffold_7\tx", "scaffold_7"),
    ("chr.fa", "  padded  name", "padded")])
def test_record_name_of_fasta_records(filename, header, name):
    from deepgrp_amd.evaluation import record_name
    assert record_name(filename, header) == name


def test_record_name_of_npz_inputs(tmp_path):
    """A `.npz` input is named after its file: the basename up to the first '.' (the header is ignored)."""
    from deepgrp_amd.evaluation import record_name
    for fname, name in (("chr3.fa.gz.npz", "chr3"), ("chrX.npz", "chrX"), ("hg.chr21.fa.gz.npz", "hg")):
        p = tmp_path / "d.e" / fname
        p.parent.mkdir(exist_ok=True)
        p.write_bytes(b"")
        assert record_name(str(p), fname[:-4]) == name
    assert record_name(str(tmp_path / "missing.fa.gz.npz"), "missing.fa.gz") == "missing.fa.gz"     # not a file: a header
