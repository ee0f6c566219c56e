"""`evaluate --curves` from the command line against statements built here: one FASTA of about 300 kb -- a record long enough to run
alone and thirty short ones that batch -- with a planted annotation; PREFIX.bases.tsv from ContigPipeline.merged per record, a
numpy-painted truth and a numpy histogram; PREFIX.rows.tsv from the scores `predict --bed_dir` prints and the same truth; the report
with and without the flag; `.npz` input and -m."""
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
    lines += [f"chrL\t{fl - 40}\t{fl + 60}\t2\tedge\tflank\n", f"chrL\t100000\t103000\t1\tover\tlap\n", f"chrL\t101000\t102000\t3\tover\tlap\n",
              f"chrL\t{fl // 4}\t{fl // 2}\t4\tinN\tflank\n"]
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


def _truth_of(seq, rows):
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


def _statement(model_file, recs, ann_rows, bins, use_mss=True):
    """-> (hist [C, 2, bins], {name: (startpos, truth)}) from ContigPipeline.merged of every record."""
    from deepgrp_amd import curves, model as dgmodel
    from deepgrp_amd.pipeline import ContigPipeline, upload_sequence
    pipe = ContigPipeline(dgmodel.load_model(model_file), 50, 256, 50, 50, use_mss=use_mss)
    hist, truths = None, {}
    for header, seq in recs:
        name = header.split()[0]
        st, truth = _truth_of(seq, ann_rows.get(name, []))
        st2, d_idx = upload_sequence(seq)
        merged = pipe.merged(d_idx).cpu().numpy()
        assert st2 == st and len(merged) == len(truth)
        h, flag = curves.reference_hist(merged, truth, bins)
        assert flag == 0
        hist = h if hist is None else hist + h
        truths[name] = (st, truth)
    return hist, truths


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Everything the tests below read, made once: evaluate without and with --curves, predict --bed_dir, the statement."""
    from deepgrp_amd.__main__ import main
    tmp = tmp_path_factory.mktemp("curves")
    model = _model(tmp)
    fa, recs, ann, ann_rows = _inputs(tmp)
    main(["evaluate", model, ann, fa, "--output", str(tmp / "plain.tsv"), "--json", str(tmp / "plain.json")])
    main(["evaluate", model, ann, fa, "--output", str(tmp / "curves.tsv"), "--json", str(tmp / "curves.json"), "--curves", str(tmp / "run")])
    (tmp / "beds").mkdir()
    main(["predict", model, fa, "--output", str(tmp / "pred.tsv"), "--bed_dir", str(tmp / "beds")])
    hist, truths = _statement(model, recs, ann_rows, 1000)
    return dict(tmp=tmp, model=model, fa=fa, recs=recs, ann=ann, ann_rows=ann_rows, hist=hist, truths=truths,
                plain=json.load(open(tmp / "plain.json")), curves=json.load(open(tmp / "curves.json")))


def test_only_the_two_files_appear(run):
    names = sorted(f for f in os.listdir(run["tmp"]) if f.startswith("run") or f.startswith(".run"))
    assert names == ["run.bases.tsv", "run.rows.tsv"]


def test_bases_file_is_the_statement(run):
    from deepgrp_amd import curves
    got = (run["tmp"] / "run.bases.tsv").read_text()
    assert got == curves.bases_tsv(run["hist"])
    lines = got.splitlines()
    assert len(lines) == 1 + 5 * 1000
    js = run["curves"]
    for c in range(5):
        f = lines[1 + c * 1000].split("\t")                            # threshold 0: every base is called
        assert f[:2] == [str(c), "0.0"]
        assert int(f[2]) + int(f[3]) == js["bases"] == int(run["hist"][c].sum())
        assert int(f[2]) == sum(js["confusion_matrix"][c]) == int(run["hist"][c, 1].sum())
    assert js["bases"] == sum(len(t) for _st, t in run["truths"].values())


def test_rows_file_is_the_statement_from_predicts_bed_scores(run):
    from deepgrp_amd import curves
    seg = np.zeros((5, 1001), np.int64)
    sup = np.zeros((5, 1001), np.int64)
    bed = [f for f in os.listdir(run["tmp"] / "beds")]
    assert len(bed) == 1
    nrows = 0
    for line in open(run["tmp"] / "beds" / bed[0]):
        f = line.rstrip("\n").split("\t")
        name, s, e, lab, score = f[0], int(f[1]), int(f[2]), int(f[3][len("class"):]), int(f[4])
        st, truth = run["truths"][name]
        hits = int((truth[s - st:e - st] == lab).sum())
        seg[lab, score] += 1
        sup[lab, score] += hits >= THETA * (e - s)
        nrows += 1
    assert nrows > 30 and len(set(np.nonzero(seg)[1])) > 3              # rows of several scores
    got = (run["tmp"] / "run.rows.tsv").read_text()
    assert got == curves.rows_tsv(seg, sup)
    lines = got.splitlines()
    assert len(lines) == 1 + 4 * 1001
    js = run["curves"]
    for c in range(1, 5):
        f = lines[1 + (c - 1) * 1001].split("\t")
        assert f[:2] == [str(c), "0"] and int(f[2]) == js["segments"][c] and int(f[3]) == js["supported"][c]


def test_report_is_byte_identical_and_json_gains_one_key(run):
    from deepgrp_amd import curves
    assert (run["tmp"] / "plain.tsv").read_bytes() == (run["tmp"] / "curves.tsv").read_bytes()
    plain, with_curves = run["plain"], dict(run["curves"])
    assert "curves" not in plain
    got = with_curves.pop("curves")
    assert with_curves == plain
    want = curves.summaries(run["hist"])
    assert got["bins"] == 1000 and sorted(got) == ["auroc", "average_precision", "best_f1", "best_threshold", "bins"]
    for k, v in want.items():
        assert got[k] == [None if np.isnan(x) else x for x in v], k
    assert all(a is not None and a > 0.5 for a in got["auroc"])        # the trained model ranks planted repeats above background


def test_the_plain_run_stays_on_the_fused_call(run, monkeypatch, tmp_path):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.pipeline import ContigPipeline
    monkeypatch.setattr(ContigPipeline, "merged", lambda *a, **k: pytest.fail("the merged path ran without --curves"))
    monkeypatch.setattr(ContigPipeline, "run_batch_probs", lambda *a, **k: pytest.fail("the merged path ran without --curves"))
    main(["evaluate", run["model"], run["ann"], run["fa"], "--output", str(tmp_path / "again.tsv")])
    assert (tmp_path / "again.tsv").read_bytes() == (run["tmp"] / "plain.tsv").read_bytes()


def test_npz_input_without_mss_and_other_bins(run, tmp_path):
    from deepgrp_amd import curves
    from deepgrp_amd.__main__ import main
    # a short record with annotation rows and no N at either end (an .npz has no startpos)
    header, seq = next((h, s) for h, s in run["recs"][1:] if h in run["ann_rows"] and s[:1] != b"N" and s[-1:] != b"N")
    idx = np.frombuffer(seq, np.uint8)
    code = np.full(256, 4, np.int64)
    code[[65, 67, 71, 84]] = [0, 1, 2, 3]
    fwd = np.zeros((5, idx.size), np.int8)
    fwd[code[idx], np.arange(idx.size)] = 1
    npz = tmp_path / (header + ".fa.gz.npz")
    np.savez_compressed(npz, fwd=fwd)
    for flags in (["-m"], []):
        main(["evaluate", run["model"], run["ann"], str(npz), "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json"),
              "--curves", str(tmp_path / "c"), "--curve_bins", "64"] + flags)
        hist, _truths = _statement(run["model"], [(header, seq)], run["ann_rows"], 64, use_mss=not flags)
        assert (tmp_path / "c.bases.tsv").read_text() == curves.bases_tsv(hist)
        js = json.load(open(tmp_path / "r.json"))
        assert js["curves"]["bins"] == 64 and js["bases"] == len(seq)
        rows = (tmp_path / "c.rows.tsv").read_text().splitlines()
        assert len(rows) == 1 + 4 * 1001
        for c in range(1, 5):
            f = rows[1 + (c - 1) * 1001].split("\t")
            assert int(f[2]) == js["segments"][c] and int(f[3]) == js["supported"][c]
