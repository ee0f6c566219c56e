"""`compare` on the GPU at the library level: the rows `predict` wrote, sent through the other door, must give `evaluate`'s report to
the byte -- the table, the JSON outside `info`, and the files of --strata, --offtarget and --boundaries -- for records on their own
and for a file of short records that `evaluate` runs as batches; flattening on the device against its numpy statement; a table and
a listing against themselves.

The model is small and random (units 8, window 20, step 5) with the bias of the output layer pushed towards the repeat classes, so
that every record of mixed bases gets rows; one unit is wired to follow the bases A and T (the second strand reads the complement)
and to decide for the background where it is on, so the record `quiet`, all T, has no predicted row.  (Every other record loses
its A and T bases to the background: many short rows.)"""
import json
import os

import numpy as np
import pytest

import rm_cases
from compare_cases import FOREIGN, FOREIGN_SPAN, SEG, rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOP = ["-s", "5", "-l", "40", "-x", "10"]
INFO_KEYS = {"model", "annotation", "inputs", "repeats", "options", "predicted", "predicted_format", "predicted_rows"}
FAMILY = {1: "HSATII", 2: "ALR/Alpha", 3: "SINE/Alu", 4: "LINE/L1"}


def _model(tmp_path):
    from deepgrp_amd import model as dgmodel, synthetic
    w = synthetic.synthetic_weights(units=8, classes=5, seed=3, gain=3.0)
    w["ff_bias"] = np.array([-1.5, 0.4, 0.4, 0.4, 0.4], np.float32)
    # unit 0: update gate shut (the state is the candidate), the candidate +1 on A and T and -1 elsewhere, nothing recurrent; its weight
    # for the background outweighs whatever the other seven units say
    u = 8
    w["kernel"][:, 0], w["recurrent_kernel"][:, 0] = -10.0, 0.0
    w["kernel"][:, 2 * u], w["recurrent_kernel"][:, 2 * u] = [6.0, -6.0, -6.0, 6.0, -6.0], 0.0
    w["ff_kernel"][0] = [40.0, 0.0, 0.0, 0.0, 0.0]
    path = str(tmp_path / "small.hdf5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=20)
    return path


def _write_fasta(path, records):
    with open(path, "wb") as fh:
        for header, seq in records:
            fh.write(b">" + header.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")


def _seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _annotations(tmp_path, rng, named, stem):
    """The same truth as a table and as a `.out` listing: rows of the classes 1..4 (overlapping, one sticking out of its record), a
    row of a class outside --repeats and, in the listing, rows of families the model does not have."""
    table, listing = [], [rm_cases.HEADER.rstrip("\n")]
    for name, n in named:
        for _ in range(max(n // 40, 2)):
            s = int(rng.integers(0, max(n - 30, 1)))
            e = s + int(rng.integers(5, 80))
            lab = int(rng.integers(1, 5))
            table.append(f"{name}\t{s}\t{e}\t{lab}\trep\t{FAMILY[lab]}\n")
            listing.append(rm_cases.out_line(ctg=name, begin=s + 1, end=e, rep="rep", fam=FAMILY[lab], tok0=str(int(rng.integers(200, 3000)))))
        table.append(f"{name}\t3\t30\t6\trep\tLINE/L2\n")
        listing.append(rm_cases.out_line(ctg=name, begin=4, end=30, rep="L2a", fam="LINE/L2"))
        listing.append(rm_cases.out_line(ctg=name, begin=max(n // 2, 1), end=n // 2 + 25, rep="Charlie1", fam="DNA/hAT-Charlie"))
    table.append("elsewhere\t10\t50\t1\n")
    listing.append(rm_cases.out_line(ctg="elsewhere", begin=11, end=50, fam="SINE/Alu"))
    t, l = tmp_path / f"{stem}.bed", tmp_path / f"{stem}.fa.out"
    t.write_text("# truth\n" + "".join(table))
    l.write_text("\n".join(listing) + "\n")
    return str(t), str(l)


def _world(tmp_path, records, annotated, stem, tail=()):
    from deepgrp_amd.__main__ import main
    rng = np.random.default_rng(17)
    model = _model(tmp_path)
    fa = str(tmp_path / f"{stem}.fa")
    _write_fasta(fa, records)
    table, listing = _annotations(tmp_path, rng, annotated, stem)
    pred = str(tmp_path / f"{stem}.pred.tsv")
    main(TOP + ["predict", model, fa, "--output", pred] + list(tail))
    return dict(model=model, fa=fa, table=table, listing=listing, pred=pred, dir=tmp_path, stem=stem, tail=list(tail))


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """Four records: N runs at both ends, plain, absent from the annotation, and all T (no predicted row).  Labelled by the softmax
    (-m): the MSS path gives the last bases of every record, which no full window covers, a row of their own."""
    rng = np.random.default_rng(5)
    records = [("withN some words", b"N" * 37 + _seq(rng, 410) + b"N" * 21), ("plain", _seq(rng, 333)), ("unannotated x", _seq(rng, 260)),
               ("quiet", b"T" * 33)]
    return _world(tmp_path_factory.mktemp("four"), records, [("withN", 468), ("plain", 333), ("quiet", 33)], "four", ["-m"])


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """About 40 records of 60-120 bases, some with N flanks: `evaluate` runs them as batches."""
    rng = np.random.default_rng(6)
    records, annotated = [], []
    for k in range(40):
        n = int(rng.integers(60, 121))
        lead, trail = (int(rng.integers(1, 9)), int(rng.integers(1, 9))) if k % 4 == 0 else (0, 0)
        records.append((f"ctg{k} scaffold", b"N" * lead + _seq(rng, n) + b"N" * trail))
        if k % 5:
            annotated.append((f"ctg{k}", n + lead + trail))
    return _world(tmp_path_factory.mktemp("many"), records, annotated, "many")


def _evaluate_and_compare(w, ann, reports):
    from deepgrp_amd.__main__ import main
    d, stem = w["dir"], w["stem"]
    tag = f"{stem}.{'listing' if ann == w['listing'] else 'table'}"
    extra = lambda side: [x for r in reports for x in (f"--{r}", str(d / f"{tag}.{side}"))]
    main(TOP + ["evaluate", w["model"], ann, w["fa"], "--output", str(d / f"{tag}.e.tsv"), "--json", str(d / f"{tag}.e.json")] + extra("e") + w["tail"])
    main(["compare", w["pred"], ann, w["fa"], "--output", str(d / f"{tag}.c.tsv"), "--json", str(d / f"{tag}.c.json")] + extra("c"))
    read = lambda p: open(d / p, "rb").read()
    ej, cj = json.load(open(d / f"{tag}.e.json")), json.load(open(d / f"{tag}.c.json"))
    return tag, read, ej, cj


def _same_report(w, ann, reports):
    tag, read, ej, cj = _evaluate_and_compare(w, ann, reports)
    assert read(f"{tag}.c.tsv") == read(f"{tag}.e.tsv")
    assert {k: v for k, v in cj.items() if k not in INFO_KEYS} == {k: v for k, v in ej.items() if k not in INFO_KEYS}
    assert set(ej) - INFO_KEYS >= {"confusion_matrix", "metrics", "elements", "found", "segments", "supported"} | set(reports)
    assert sum(ej["segments"]) > 0 and sum(ej["elements"]) > 0 and ej["outside"] >= 0
    assert cj["predicted"] == w["pred"] and cj["predicted_format"] == "tsv" and cj["classes"] == 5
    assert "model" not in cj and "fast" not in cj["options"]
    nrows = sum(1 for _ in open(w["pred"]))
    assert cj["predicted_rows"] == {"read": nrows, "dropped": 0, "flattened": nrows} and nrows == sum(ej["segments"])
    suffixes = {"strata": [".strata.tsv"], "offtarget": [".offtarget.tsv", ".offtarget.rows.tsv"], "boundaries": [".boundaries.tsv", ".fragments.tsv"]}
    for r in reports:
        for s in suffixes[r]:
            assert read(f"{tag}.c{s}") == read(f"{tag}.e{s}"), s
    if "strata" in reports:
        assert os.path.exists(w["dir"] / f"{tag}.e.strata.bases.tsv") and not os.path.exists(w["dir"] / f"{tag}.c.strata.bases.tsv")
    return ej, cj


def test_predict_rows_come_back_as_evaluates_report_table(four):
    ej, _cj = _same_report(four, four["table"], ["strata", "boundaries"])
    assert ej["records"] == 4 and ej["records_annotated"] == 3


def test_predict_rows_come_back_as_evaluates_report_listing(four):
    ej, _cj = _same_report(four, four["listing"], ["strata", "offtarget", "boundaries"])
    assert ej["records"] == 4 and ej["records_annotated"] == 3


def test_the_four_records_are_what_the_cases_ask_for(four):
    from deepgrp_amd.compare import read_predicted
    from deepgrp_amd.evaluation import read_annotation
    pred = read_predicted(four["pred"], "auto", 5)
    assert pred.format == "tsv" and pred.route == "device"
    assert {"withN", "plain", "unannotated"} <= set(pred) and "quiet" not in pred          # all T: background
    ann = read_annotation(four["table"], [1, 2, 3, 4])
    assert "unannotated" not in ann and "quiet" in ann and "elsewhere" in ann
    host = read_predicted(four["pred"], "tsv", 5, device=False)
    assert host.route == "host" and list(host) == list(pred)
    for name in pred:
        assert pred[name].tolist() == host[name].tolist() and pred.lines[name].tolist() == host.lines[name].tolist()


def test_the_batched_path(many, monkeypatch):
    from deepgrp_amd.evaluation import Accumulator
    from deepgrp_amd.pipeline import ContigPipeline
    batched, adds = [], []
    real_batch, real_add = ContigPipeline.run_batch, Accumulator.add

    def counting(self, d_base, offsets, *a, **k):
        batched.append(len(offsets))
        return real_batch(self, d_base, offsets, *a, **k)

    def add(self, origins, lengths, *a, **k):
        adds.append(len(lengths))
        return real_add(self, origins, lengths, *a, **k)
    monkeypatch.setattr(ContigPipeline, "run_batch", counting)
    monkeypatch.setattr(Accumulator, "add", add)
    ej, _cj = _same_report(many, many["table"], [])
    assert ej["records"] == 40 and sum(batched) == 40 and max(batched) > 1     # evaluate ran them as batches
    assert adds[-1] == 40 and sum(adds) == 80                                    # compare: one work item, one Accumulator.add
    adds.clear()
    ej, _cj = _same_report(many, many["listing"], ["strata", "offtarget", "boundaries"])
    assert ej["records"] == 40 and max(adds[:-1]) > 1 and adds[-1] == 40 and sum(adds) == 80


def test_library_call_gives_the_same_table(four):
    from deepgrp_amd import compare as dgcompare
    from deepgrp_amd.__main__ import _records_of
    from deepgrp_amd.evaluation import tsv_report
    pred = dgcompare.read_predicted(four["pred"], "auto", 5)
    ann = dgcompare.read_table(four["table"], [1, 2, 3, 4])
    assert ann.route == "device"
    rep = dgcompare.compare(pred, ann, [(four["fa"], _records_of(four["fa"]))], 5, [1, 2, 3, 4], 0.5, dict(predicted=four["pred"]))
    want = four["dir"] / "four.table.e.tsv"
    if not want.exists():
        _evaluate_and_compare(four, four["table"], [])
    assert tsv_report(rep).encode() == open(want, "rb").read()
    assert rep["repeats"] == [1, 2, 3, 4] and rep["predicted_rows"]["flattened"] == rep["predicted_rows"]["read"]


def test_read_table_is_read_annotation(four):
    from deepgrp_amd.compare import read_table
    from deepgrp_amd.evaluation import read_annotation
    for repeats in (None, [1, 2, 3, 4], [2]):
        got, want = read_table(four["table"], repeats), read_annotation(four["table"], repeats)
        assert got.route == "device" and list(got) == list(want)
        for name in want:
            assert got[name].tolist() == want[name].tolist()


# ---------------------------------------------------------------- flattening on the device
def test_flatten_on_the_device_is_the_numpy_statement():
    from deepgrp_amd.compare import flatten, flatten_reference
    names = sorted(FOREIGN)
    o, n = FOREIGN_SPAN
    # every case as a record of its own, and all of them as the records of one work item, between records without rows
    for group in [[k] for k in names] + [names]:
        given = [FOREIGN[k][0] for k in group]
        org, ln = [o] * len(group), [n] * len(group)
        if len(group) > 1:
            given, org, ln = [rows()] + given + [rows((5, 9, 1))], [0] + org + [0], [50] + ln + [0]
        got = flatten(org, ln, given)
        assert len(got) == len(given)
        for r, g in enumerate(got):
            want = flatten_reference(org[r], ln[r], given[r])
            assert g.dtype == SEG and g[["start", "end", "label"]].tolist() == want[["start", "end", "label"]].tolist(), group[max(r - 1, 0)]
            assert (g["contig"] == r).all()
        if len(group) == 1:
            assert got[0][["start", "end", "label"]].tolist() == FOREIGN[group[0]][1][["start", "end", "label"]].tolist()
    rng = np.random.default_rng(2)
    for n in (1, 2, 2047, 2048, 2049, 5000):                                     # around the tile of the run extraction
        s = rng.integers(90, 110 + n, 80)
        given = rows(*[(int(a), int(a) + int(rng.integers(0, 200)), int(rng.integers(1, 5))) for a in s])
        got = flatten([100], [n], [given])[0]
        assert got[["start", "end", "label"]].tolist() == flatten_reference(100, n, given)[["start", "end", "label"]].tolist()


# ---------------------------------------------------------------- a table and a listing against themselves
@pytest.mark.parametrize("form", ("table", "listing"))
def test_a_file_against_itself_is_perfect(four, form):
    from deepgrp_amd import annotation as dgann, compare as dgcompare
    from deepgrp_amd.__main__ import _records_of
    path = four[form]
    pred = dgcompare.read_predicted(path, "auto", 5)
    assert pred.format == ("table" if form == "table" else "repeatmasker") and pred.route == "device"
    assert pred.rows_dropped == 3 and pred.rows_read - pred.rows_dropped == sum(len(v) for v in pred.values())
    ann = dgcompare.read_table(path, [1, 2, 3, 4]) if form == "table" else dgann.evaluation_rows(path, [1, 2, 3, 4])
    rep = dgcompare.compare(pred, ann, [(four["fa"], _records_of(four["fa"]))], 5, [1, 2, 3, 4])
    cnf = np.array(rep["confusion_matrix"])
    assert (cnf == np.diag(np.diag(cnf))).all() and rep["metrics"]["TotalACC"] == 1.0
    present = [c for c in range(5) if cnf[c, c]]
    assert 0 in present and len(present) >= 3
    for c in present:
        assert rep["metrics"]["TPR"][c] == 1.0 and rep["metrics"]["PPV"][c] == 1.0
    # overlapping rows were flattened: every flattened row lies on its own class (an element under a smaller label may be lost)
    assert rep["supported"] == rep["segments"] and sum(rep["segments"]) == rep["predicted_rows"]["flattened"] > 0
    assert rep["predicted_rows"]["read"] == pred.rows_read and rep["predicted_rows"]["dropped"] == pred.rows_dropped
