"""GFF3 from the command line, in child processes: `predict --bed_dir D --bed_gff3` writes a file, `compare` reads it back as
PREDICTED and as ANNOTATION; `evaluate` takes a GFF3 annotation; names with alternatives, the type column, dropped rows, the host
route and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gff_in_cases import feature, gff_of_table

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = "LTR|ERV1|ERVK,LINE|L1,Alu,Satellite|a/b"
FAMILY_OF = {1: (b"LTR", b"ERV1", b"ERVK"), 2: (b"LINE", b"L1"), 3: (b"Alu",), 4: (b"Satellite", b"a%2Fb", b"a%2fb")}


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
    """Two planted records and one without annotation, the trained synthetic model, a table of the planted truth; one `predict` run
    that writes the TSV and the GFF3, a second that writes the .gff3.gz."""
    from deepgrp_amd import model as dgmodel, synthetic
    d = tmp_path_factory.mktemp("gffcli")
    w = synthetic.trained_weights()
    model = str(d / "synth.hdf5")
    dgmodel.save_keras_hdf5(model, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    recs, lines = [], []
    for k, (n, fl) in enumerate(((120_000, 400), (90_000, 0), (9_000, 100))):
        recs.append((f"chr{k + 1}" + (" assembled by hand" if k == 0 else ""), synthetic.synthetic_chromosome(n, contig=30 + k, flank=fl)))
        if k < 2:
            lines += synthetic.synthetic_annotation(n, contig=30 + k, name=f"chr{k + 1}", flank=fl)
    fa = d / "x.fa"
    with open(fa, "wb") as fh:
        for header, seq in recs:
            fh.write(b">" + header.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    ann = d / "truth.bed"
    ann.write_text("".join(lines))
    out = dict(model=model, ann=str(ann), dir=d, fa=str(fa), tsv=str(d / "pred.tsv"), gff=str(d / "plain" / "x.fa.gff3"),
               gz=str(d / "gz" / "x.fa.gff3.gz"))
    _run(["predict", model, fa, "--output", out["tsv"], "--bed_dir", d / "plain", "--bed_gff3"])
    _run(["predict", model, fa, "--output", d / "again.tsv", "--bed_dir", d / "gz", "--bed_gff3", "--bed_gzip"])
    assert open(out["gff"], "rb").read(16) == b"##gff-version 3\n" and open(d / "again.tsv").read() == open(out["tsv"]).read()
    out["report"] = _run(["compare", out["tsv"], out["ann"], fa]).stdout
    return out


def _tsv_rows(path):
    rows = []
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        rows.append((f[1].split()[0], int(f[-3]), int(f[-2]), int(f[-1])))
    return rows


@pytest.mark.parametrize("key", ("gff", "gz"), ids=("plain", "gzip"))
def test_predicts_gff3_gives_the_report_of_its_tsv(world, key, tmp_path):
    js = tmp_path / "r.json"
    c = _run(["compare", world[key], world["ann"], world["fa"], "--json", js])                # no flag: sniffed, default names
    assert c.stdout == world["report"] and c.stdout.startswith("#class\t") and len(c.stdout.splitlines()) == 8
    rep = json.load(open(js))
    rows = _tsv_rows(world["tsv"])
    assert rep["predicted_format"] == "gff3" and rep["predicted_rows"] == {"read": len(rows), "dropped": 0, "flattened": len(rows)} and len(rows) > 20
    assert _run(["compare", world[key], world["ann"], world["fa"], "--predicted_format", "gff3", "--gff_key", "Name"]).stdout == world["report"]


def test_the_gff3_as_annotation_of_its_own_tsv(world, tmp_path):
    js = tmp_path / "r.json"
    _run(["compare", world["tsv"], world["gff"], world["fa"], "--json", js])
    rep = json.load(open(js))
    present = {r[3] for r in _tsv_rows(world["tsv"])}
    assert len(present) >= 2
    for c in sorted(present):
        assert rep["metrics"]["TPR"][c] == 1.0 and rep["metrics"]["PPV"][c] == 1.0, c
    cnf = np.array(rep["confusion_matrix"])
    assert cnf.sum() == np.trace(cnf) and rep["found"] == rep["elements"] and rep["supported"] == rep["segments"]


def test_evaluate_on_a_gff3_of_the_tables_rows(world, tmp_path):
    from gff_in_cases import NAMES4
    table = [ln.split() for ln in open(world["ann"]) if ln.strip() and not ln.startswith("#")]
    rows = [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in table]
    assert all(1 <= r[3] <= 4 for r in rows) and len(rows) > 10
    p = tmp_path / "truth.gff3"
    p.write_bytes(gff_of_table(rows, NAMES4))
    names = ",".join("|".join(a.decode() for a in e if b";" not in a and b"%" not in a) for e in NAMES4)
    want = _run(["evaluate", world["model"], world["ann"], world["fa"], "--boundaries", tmp_path / "t", "--strata", tmp_path / "t"])
    got = _run(["evaluate", world["model"], p, world["fa"], "--annotation_format", "gff3", "--annotation_names", names, "--boundaries", tmp_path / "g",
                "--strata", tmp_path / "g"])
    assert got.stdout == want.stdout and got.stdout.startswith("#class\t")
    for ext in (".boundaries.tsv", ".fragments.tsv", ".strata.tsv", ".strata.bases.tsv"):      # no divergence: NA, as for the table
        assert open(str(tmp_path / "g") + ext).read() == open(str(tmp_path / "t") + ext).read(), ext
    assert "NA" in open(str(tmp_path / "g") + ".strata.tsv").read()
    # --repeats filters the numbers as it filters the table's fourth column
    from deepgrp_amd import gffin
    from deepgrp_amd.evaluation import read_annotation
    a, b = read_annotation(world["ann"], [1, 3]), gffin.read_annotation(str(p), NAMES4, b"Name", [1, 3])
    assert list(a) == list(b) and b.route == "device" and all(a[k].tolist() == b[k].tolist() for k in a) and sum(len(v) for v in a.values()) < len(rows)


@pytest.mark.parametrize("by_type", (False, True), ids=("name", "type"))
def test_alternatives_type_column_and_dropped_rows(world, tmp_path, by_type):
    rows = _tsv_rows(world["tsv"])
    text = [b"##gff-version 3\n"]
    for i, (contig, a, e, label) in enumerate(rows):
        fam = FAMILY_OF[label][i % len(FAMILY_OF[label])]
        text.append(feature(contig.encode(), a + 1, e, b"ID=%d;Name=%s" % (i, b"class1" if by_type else fam), typ=fam if by_type else b"repeat_region") + b"\n")
    junk = [] if by_type else [feature(b"chr1", 500, 900, b"ID=j1;Name=Unknown"), feature(b"chr2", 1, 9000, b"ID=j2"), feature(b"chr1", 50, 60, b"Name=LTRs")]
    text[3:3] = [ln + b"\n" for ln in junk]
    p, js = tmp_path / "named.gff3", tmp_path / "r.json"
    p.write_bytes(b"".join(text) + b"##FASTA\n>chr1\nACGT\n")
    c = _run(["compare", p, world["ann"], world["fa"], "--predicted_names", FAMILIES, "--json", js] + (["--gff_by_type"] if by_type else []))
    assert c.stdout == world["report"]
    assert json.load(open(js))["predicted_rows"] == {"read": len(rows) + len(junk), "dropped": len(junk), "flattened": len(rows)}
    if not by_type:                                                  # without the names nothing is a class: every row is dropped and counted
        from deepgrp_amd.compare import read_predicted
        got = read_predicted(str(p), "auto", 5)
        assert got.format == "gff3" and got.route == "device" and len(got) == 0 and got.rows_dropped == got.rows_read == len(rows) + len(junk)


def test_the_host_route_reads_the_same_rows(world):
    from deepgrp_amd import gffin
    names = gffin.default_names(5)
    for path in (world["gff"], world["gz"]):
        a, b = gffin.read_predicted(path, names, b"Name", 5), gffin.read_predicted(path, names, b"Name", 5, device=False)
        assert (a.route, b.route) == ("device", "host") and list(a) == list(b) == ["chr1", "chr2", "chr3"][:len(a)]
        assert (a.rows_read, a.rows_dropped) == (b.rows_read, b.rows_dropped)
        for name in a:
            assert a[name].tobytes() == b[name].tobytes() and a.lines[name].tolist() == b.lines[name].tolist()
    rows = _tsv_rows(world["tsv"])
    assert sorted((n, int(r["start"]), int(r["end"]), int(r["label"])) for n, v in a.items() for r in v) == sorted(rows)


def test_errors_are_worded(world, tmp_path):
    p = tmp_path / "bad.gff3"
    good = open(world["gff"], "rb").read()
    p.write_bytes(good + b"chr1\tdeepgrp\trepeat_region\t5\t9\n")
    r = _run(["compare", p, world["ann"], world["fa"]], ok=False)
    assert r.stdout == "" and f"{p}:{good.count(bytes([10])) + 1}: expected nine fields between tabs: 'chr1\\tdeepgrp" in r.stderr
    p.write_bytes(good + feature(start=0, end=7) + b"\n")
    r = _run(["compare", world["tsv"], p, world["fa"]], ok=False)
    assert f"{p}:{good.count(bytes([10])) + 1}: negative begin: " in r.stderr
    r = _run(["compare", world["tsv"], world["gff"], world["fa"], "--offtarget", tmp_path / "o"], ok=False)
    assert "--offtarget" in r.stderr and "holds the rows of the modelled classes only" in r.stderr
    r = _run(["evaluate", world["model"], world["gff"], world["fa"], "--offtarget", tmp_path / "o"], ok=False)
    assert "holds the rows of the modelled classes only" in r.stderr
    assert os.listdir(tmp_path) == ["bad.gff3"]


def test_train_refuses_gff3(world, tmp_path):
    toml = tmp_path / "p.toml"
    toml.write_text("units = 16\nvecsize = 50\nbatch_size = 32\nn_batches = 2\nn_epochs = 1\nattention = true\ndropout = 0.25\nlearning_rate = 0.005\n")
    for flags in ([],):
        r = _run(["train", toml, world["fa"], world["fa"], world["gff"], "--logdir", tmp_path / "log"] + flags, ok=False)
        assert f"train: {world['gff']} is GFF3" in r.stderr and not os.path.exists(tmp_path / "log")
