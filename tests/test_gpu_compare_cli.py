"""`compare` from the command line, in child processes: `predict` writes a TSV, `compare` reads it back, and its standard output is
`evaluate`'s for the same inputs -- FASTA and .2bit; the errors a user meets are worded, not traced."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _run(args, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "deepgrp_amd"] + [str(a) for a in args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert "Traceback" not in r.stderr, r.stderr
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr)
    return r


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Two planted records and one without annotation, the trained synthetic model, a table of the planted truth; the FASTA and the
    same records as .2bit, each predicted once."""
    from deepgrp_amd import model as dgmodel, synthetic, twobit
    d = tmp_path_factory.mktemp("cli")
    w = synthetic.trained_weights()
    model = str(d / "synth.hdf5")
    dgmodel.save_keras_hdf5(model, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    recs, lines = [], []
    for k, (n, fl) in enumerate(((30_000, 400), (22_000, 0), (9_000, 100))):
        recs.append((f"chr{k + 1}" + (" assembled by hand" if k == 0 else ""), synthetic.synthetic_chromosome(n, contig=30 + k, flank=fl)))
        if k < 2:
            lines += synthetic.synthetic_annotation(n, contig=30 + k, name=f"chr{k + 1}", flank=fl)
    fa = d / "g.fa"
    with open(fa, "wb") as fh:
        for header, seq in recs:
            fh.write(b">" + header.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    tb = d / "g.2bit"
    twobit.write_file([twobit.record_name(h) for h, _s in recs], [twobit.pack_record(s) for _h, s in recs], str(tb))
    ann = d / "truth.bed"
    ann.write_text("".join(lines))
    out = dict(model=model, ann=str(ann), dir=d, fa=str(fa), tb=str(tb))
    for key in ("fa", "tb"):
        out[key + "_pred"] = str(d / f"{key}.pred.tsv")
        _run(["predict", model, out[key], "--output", out[key + "_pred"]])
    return out


@pytest.mark.parametrize("key", ("fa", "tb"), ids=("fasta", "2bit"))
def test_stdout_is_evaluates(world, key):
    e = _run(["evaluate", world["model"], world["ann"], world[key]])
    c = _run(["compare", world[key + "_pred"], world["ann"], world[key]])
    assert c.stdout == e.stdout and c.stdout.startswith("#class\t") and len(c.stdout.splitlines()) == 8
    rows = [ln.split("\t") for ln in c.stdout.splitlines()[1:6]]
    assert sum(int(f[11]) for f in rows) == sum(1 for _ in open(world[key + "_pred"])) > 0     # every predicted row was scored
    assert sum(int(f[3]) for f in rows[1:]) > 0                                                 # and the model finds planted repeats


def test_an_out_of_range_label_names_file_and_line(world, tmp_path):
    lines = open(world["fa_pred"]).read().splitlines(True)
    f = lines[2].rstrip("\n").split("\t")
    lines[2] = "\t".join(f[:-1] + ["7"]) + "\n"
    p = tmp_path / "bad.tsv"
    p.write_text("".join(lines))
    r = _run(["compare", p, world["ann"], world["fa"]], ok=False)
    assert r.stdout == "" and f"{p}:3: label 7 is not a class of 1..4" in r.stderr
    assert _run(["compare", p, world["ann"], world["fa"], "--classes", "8", "--repeats", "1,2,3,4"]).stdout.startswith("#class\t")


def test_a_negative_begin_in_a_table_is_read_annotations_message(world, tmp_path):
    from deepgrp_amd.evaluation import AnnotationError, read_annotation
    p = tmp_path / "calls.txt"
    p.write_text("chr1 100 200 1\nchr1 -5 20 2\nchr2 5 9 1\n")
    with pytest.raises(AnnotationError) as e:
        read_annotation(str(p), None)
    r = _run(["compare", p, world["ann"], world["fa"], "--predicted_format", "table"], ok=False)
    assert r.stdout == "" and str(e.value) in r.stderr and f"{p}:2: negative begin" in r.stderr
    # and a short line, which the device reports and the host words
    p.write_text("chr1 100 200 1\nchr1 5\n")
    r = _run(["compare", p, world["ann"], world["fa"]], ok=False)
    assert f"{p}:2: expected contig, begin, end and repeat number" in r.stderr


def test_no_predicted_row_is_not_no_annotation_row(world, tmp_path):
    p = tmp_path / "other.tsv"
    p.write_text("g.fa\t1\t100\t200\t1\ng.fa\t2 x\t100\t200\t2\n")
    r = _run(["compare", p, world["ann"], world["fa"]], ok=False)
    assert "no predicted row names a record of the inputs" in r.stderr and "'chr1'" in r.stderr and "'1'" in r.stderr
    assert "no annotation row" not in r.stderr
    a = tmp_path / "other.bed"
    a.write_text("1\t10\t500\t1\n")
    r = _run(["compare", world["fa_pred"], a, world["fa"]], ok=False)
    assert "no annotation row names a record of the inputs" in r.stderr and "no predicted row" not in r.stderr


def test_foreign_tables_are_flattened_and_counted(world, tmp_path):
    """dna-brnn's shape: contig begin end label, overlapping and unsorted, with a label the model does not have."""
    p = tmp_path / "calls.txt"
    p.write_text("chr2 5000 5600 2\nchr1 900 1500 1\nchr1 1200 1800 3\nchr1 1000 1100 9\nchr1 1500 1600 1\n")
    js = tmp_path / "r.json"
    _run(["compare", p, world["ann"], world["fa"], "--json", js])
    import json
    rep = json.load(open(js))
    assert rep["predicted_format"] == "table" and rep["predicted_rows"] == {"read": 5, "dropped": 1, "flattened": 3}
    assert rep["segments"] == [0, 1, 1, 1, 0] and rep["records"] == 3
    cnf = np.array(rep["confusion_matrix"])
    assert cnf[:, 1].sum() == 700 and cnf[:, 3].sum() == 200 and cnf[:, 2].sum() == 600
