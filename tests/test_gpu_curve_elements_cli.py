"""`evaluate --curves --curve_elements` from the command line: one FASTA of about 300 kb -- a record long enough to run alone and
thirty short ones that batch -- with a planted annotation that has nested rows, run once with --curves and once with both flags.
The flag adds PREFIX.elements.tsv and the JSON key curves.elements and changes nothing else; the file equals curves.elements_tsv of
counts rebuilt here from the scores `predict --bed_dir` prints (an element's detection score as an order statistic of the scores
on its bases, not by bisection) and a numpy-painted truth."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

THETA = 0.5


def _write_fasta(path, records):
    with open(path, "wb") as fh:
        for header, seq in records:
            fh.write(b">" + header.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")


def _model(tmp_path):
    from deepgrp_amd import model as dgmodel, synthetic
    w = synthetic.trained_weights()
    path = str(tmp_path / "synth.hdf5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path


def _inputs(tmp_path):
    """-> (FASTA path, [(header, sequence)], annotation path, {name: [(begin, end, label)]})"""
    from deepgrp_amd import synthetic
    from deepgrp_amd.runner import SMALL_RECORD
    recs, lines = [], []
    n0, fl = 268_000, 1500
    assert n0 - 2 * fl > SMALL_RECORD                                  # runs alone
    recs.append(("chrL the long one", synthetic.synthetic_chromosome(n0, contig=41, flank=fl)))
    lines += synthetic.synthetic_annotation(n0, contig=41, name="chrL", flank=fl)
    # rows over the edge of the evaluated span, nested rows of other classes, a row inside the leading N block
    lines += [f"chrL\t{fl - 40}\t{fl + 60}\t2\tedge\tflank\n", f"chrL\t100000\t103000\t1\tover\tlap\n", f"chrL\t101000\t102000\t3\tover\tlap\n",
              f"chrL\t{fl // 4}\t{fl // 2}\t4\tinN\tflank\n", f"chrL\t50000\t90000\t2\tlong\tnest\n", f"chrL\t60000\t60300\t2\tin\tnest\n"]
    n = 60_000
    seq = synthetic.synthetic_chromosome(n, contig=42, flank=0)
    _idx, lab = synthetic.synthetic_truth(n, contig=42, flank=0)
    rng = np.random.default_rng(5)
    p = 0
    for k in range(30):
        ln = int(rng.integers(700, 2001))
        piece, truth = seq[p:p + ln], lab[p:p + ln]
        lead, trail = (int(rng.integers(1, 90)), int(rng.integers(1, 90))) if k % 3 == 0 else (0, 0)
        name = f"ctg{k}"
        recs.append((name, b"N" * lead + piece + b"N" * trail))
        edge = np.flatnonzero(np.diff(truth.astype(np.int16), prepend=0, append=0))
        for b, e in zip(edge[:-1], edge[1:]):
            if truth[b] and k % 10 != 9:                               # every tenth record has no annotation row
                lines.append(f"{name}\t{b + lead}\t{e + lead}\t{int(truth[b])}\n")
                if e - b > 40 and k % 4 == 1:                          # the same element once more, as two nested halves
                    lines.append(f"{name}\t{b + lead}\t{(b + e) // 2 + lead}\t{int(truth[b])}\n")
        p += ln
    fa = tmp_path / "in.fa"
    _write_fasta(fa, recs)
    ann = tmp_path / "in.bed"
    ann.write_text("".join(lines))
    rows = {}
    for l in lines:
        c = l.split()
        rows.setdefault(c[0], []).append((int(c[1]), int(c[2]), int(c[3])))
    return str(fa), recs, str(ann), rows


def _span_and_truth(seq, rows):
    """(startpos, truth int8 over the kept bases): the smallest label among the rows that cover a base, 0 where none does."""
    a = np.frombuffer(seq, np.uint8)
    nonn = np.flatnonzero(a != ord("N"))
    st, en = int(nonn[0]), int(nonn[-1]) + 1
    full = np.zeros(len(seq), np.int8)
    for lab in (4, 3, 2, 1):
        for b, e, l in rows:
            if l == lab:
                full[b:e] = lab
    return st, full[st:en]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Everything the tests below read, made once: evaluate --curves without and with --curve_elements, predict --bed_dir."""
    from deepgrp_amd.__main__ import main
    tmp = tmp_path_factory.mktemp("curve_elements")
    model = _model(tmp)
    fa, recs, ann, ann_rows = _inputs(tmp)
    for name, flags in (("without", []), ("with", ["--curve_elements"])):
        (tmp / name).mkdir()
        main(["evaluate", model, ann, fa, "--output", str(tmp / name / "report.tsv"), "--json", str(tmp / name / "report.json"),
              "--curves", str(tmp / name / "run")] + flags)
    (tmp / "beds").mkdir()
    main(["predict", model, fa, "--output", str(tmp / "pred.tsv"), "--bed_dir", str(tmp / "beds")])
    bed = os.listdir(tmp / "beds")
    assert len(bed) == 1
    pred = {}
    for line in open(tmp / "beds" / bed[0]):
        f = line.rstrip("\n").split("\t")
        pred.setdefault(f[0], []).append((int(f[1]), int(f[2]), int(f[3][len("class"):]), int(f[4])))
    return dict(tmp=tmp, recs=recs, ann_rows=ann_rows, pred=pred, without=json.load(open(tmp / "without" / "report.json")),
                with_=json.load(open(tmp / "with" / "report.json")))


@pytest.fixture(scope="module")
def counts(run):
    """(det [5, 1002], seg, sup [5, 1001], every detection score) rebuilt from predict's BED and the inputs."""
    det = np.zeros((5, 1002), np.int64)
    seg = np.zeros((5, 1001), np.int64)
    sup = np.zeros((5, 1001), np.int64)
    scores_seen = []
    for header, seq in run["recs"]:
        name = header.split()[0]
        st, truth = _span_and_truth(seq, run["ann_rows"].get(name, []))
        n = len(truth)
        label = np.zeros(n, np.int64)
        score = np.zeros(n, np.int64)
        for s, e, lab, sc in run["pred"].get(name, []):
            assert st <= s < e <= st + n
            label[s - st:e - st], score[s - st:e - st] = lab, sc
            seg[lab, sc] += 1
            sup[lab, sc] += int((truth[s - st:e - st] == lab).sum()) >= THETA * (e - s)
        for b, e, lab in run["ann_rows"].get(name, []):
            a, z = min(max(b - st, 0), n), min(max(e - st, 0), n)
            if z <= a:
                continue                                               # no base inside the evaluated span: not an element here
            need = int(np.ceil(THETA * (z - a)))
            mine = np.sort(score[a:z][label[a:z] == lab])[::-1]        # the scores on its bases, highest first
            d = int(mine[need - 1]) if len(mine) >= need else -1       # the need-th highest: with m above it too few bases are left
            det[lab, d + 1] += 1
            scores_seen.append(d)
    return det, seg, sup, scores_seen


def test_the_flag_adds_one_file_and_changes_no_other(run):
    tmp = run["tmp"]
    assert sorted(os.listdir(tmp / "without")) == ["report.json", "report.tsv", "run.bases.tsv", "run.rows.tsv"]
    assert sorted(os.listdir(tmp / "with")) == ["report.json", "report.tsv", "run.bases.tsv", "run.elements.tsv", "run.rows.tsv"]
    for f in ("report.tsv", "run.bases.tsv", "run.rows.tsv"):
        assert (tmp / "without" / f).read_bytes() == (tmp / "with" / f).read_bytes(), f


def test_json_differs_by_the_elements_key_alone(run, counts):
    from deepgrp_amd import curves
    a, b = run["without"], json.loads(json.dumps(run["with_"]))
    assert sorted(a["curves"]) == ["auroc", "average_precision", "best_f1", "best_threshold", "bins"]
    got = b["curves"].pop("elements")
    for js in (a, b):                                                  # the two runs write to different directories
        js.pop("output", None)
    assert a == b
    det, seg, sup, _seen = counts
    want = curves.element_summary(det, seg, sup)
    assert sorted(got) == ["best_f1", "best_min_score", "recall_at_0"]
    for k, v in want.items():
        assert got[k] == [None if np.isnan(x) else x for x in v], k
    assert got["recall_at_0"][0] is None and all(x is not None for x in got["recall_at_0"][1:])       # every repeat class has elements


def test_elements_file_is_the_statement_from_predicts_bed_scores(run, counts):
    from deepgrp_amd import curves
    det, seg, sup, seen = counts
    assert len(seen) > 30 and len(set(seen)) >= 3 and -1 in seen         # several detection scores: the curve is not flat
    got = (run["tmp"] / "with" / "run.elements.tsv").read_text()
    assert got == curves.elements_tsv(det, seg, sup)


def test_elements_file_against_the_report_and_the_rows_file(run):
    lines = (run["tmp"] / "with" / "run.elements.tsv").read_text().splitlines()
    rows = (run["tmp"] / "with" / "run.rows.tsv").read_text().splitlines()
    assert lines[0] == "#class\tmin_score\telements\tfound\trecall\tsegments\tsupported\tprecision\tF1"
    assert len(lines) == len(rows) == 1 + 4 * 1001
    js = run["with_"]
    distinct = set()
    for c in range(1, 5):
        block = [l.split("\t") for l in lines[1 + (c - 1) * 1001:1 + c * 1001]]
        assert [f[:2] for f in block] == [[str(c), str(m)] for m in range(1001)]
        assert int(block[0][2]) == js["elements"][c] and int(block[0][3]) == js["found"][c]     # m = 0 is the report's operating point
        assert len({f[2] for f in block}) == 1
        found = np.array([int(f[3]) for f in block])
        assert (np.diff(found) <= 0).all()                             # found never rises with m
        distinct |= set(np.flatnonzero(np.diff(found)).tolist())
        for f, r in zip(block, rows[1 + (c - 1) * 1001:1 + c * 1001]):
            assert f[5:8] == r.split("\t")[2:5]
    assert len(distinct) >= 3
