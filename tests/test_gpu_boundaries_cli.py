"""`evaluate --boundaries` from the command line against statements built here: a synthetic record of 200 kb and a short one that goes
through the batch path, a small model, and a RepeatMasker listing of the planted repeats -- some listed as two abutting rows, some
beginning late or ending behind the planted run, one sticking out of the evaluated span.  Both files and the JSON key against numpy
over `predict`'s rows and the annotation, the report with and without the flag, two runs, the table form and the gzip listing,
--boundary_join 0, and the flag beside --curves, --strata and --offtarget."""
import contextlib
import gzip
import io
import json
import os

import numpy as np
import pytest

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

THETA = 0.5
REPEATS = [1, 2, 3, 4]
N, FLANK = 200_000, 1000
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
SUFFIXES = (".boundaries.tsv", ".fragments.tsv")


def _model(tmp_path):
    from deepgrp_amd import model as dgmodel, synthetic
    w = synthetic.trained_weights()
    path = str(tmp_path / "synth.hdf5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path


def _inputs(tmp):
    """-> (FASTA path, {name: sequence}, the listing's lines)"""
    from deepgrp_amd import synthetic
    long_seq = synthetic.synthetic_chromosome(N, contig=10, flank=FLANK)
    short_seq = b"NNN" + synthetic.synthetic_chromosome(1800, contig=11, flank=0) + b"NN"
    lines = []
    for k, row in enumerate(synthetic.synthetic_annotation(N, contig=10, name="chr1", flank=FLANK)):
        ctg, b, e, lab = row.split("\t")[:4]
        b, e, lab = int(b), int(e), int(lab)
        fam = rm_cases.FAMILIES[lab - 1]
        if k % 4 == 0 and e - b > 40:                                    # one element as two abutting rows
            mid = b + (e - b) // 3
            lines += [rm_cases.out_line(ctg, b + 1, mid, "x", fam), rm_cases.out_line(ctg, mid + 1, e, "x", fam)]
        elif k % 7 == 3:
            lines.append(rm_cases.out_line(ctg, b + 16, e, "x", fam))      # listed 15 bases late: the predicted run sticks out in front
        elif k % 7 == 5:
            lines.append(rm_cases.out_line(ctg, b + 1, e + 25, "x", fam))  # listed 25 bases long: the predicted run ends early
        else:
            lines.append(rm_cases.out_line(ctg, b + 1, e, "x", fam, "+C"[k % 2]))
    lines += [rm_cases.out_line("chr1", FLANK - 39, FLANK + 60, "x", rm_cases.FAMILIES[0]),     # sticks out of the evaluated span
              rm_cases.out_line("chr1", 10, 500, "x", rm_cases.FAMILIES[1]),                    # wholly inside the N flank
              rm_cases.out_line("ctgS", 101, 700, "x", rm_cases.FAMILIES[0]), rm_cases.out_line("ctgS", 701, 1500, "x", rm_cases.FAMILIES[0]),
              rm_cases.out_line("chrUn", 10, 500, "x", rm_cases.FAMILIES[2])]
    fa = tmp / "in.fa"
    with open(fa, "wb") as fh:
        for name, seq in (("chr1", long_seq), ("ctgS", short_seq)):
            fh.write(b">" + name.encode() + b" synthetic\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    return str(fa), {"chr1": long_seq, "ctgS": short_seq}, lines


def _evaluate(tmp, tag, model, ann, fa, *flags):
    from deepgrp_amd.__main__ import main
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        main(["evaluate", model, ann, fa, "--repeats", ",".join(map(str, REPEATS)), "--json", str(tmp / f"{tag}.json")] + list(flags))
    js = json.load(open(tmp / f"{tag}.json"))
    return out.getvalue(), js


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd._scripts import parse_rm
    tmp = tmp_path_factory.mktemp("boundaries")
    model = _model(tmp)
    fa, seqs, lines = _inputs(tmp)
    text = rm_cases.HEADER + "\n".join(lines) + "\n"
    listing, table, zipped = tmp / "rm.out", tmp / "rm.bed", tmp / "rm.out.gz"
    listing.write_text(text)
    parse_rm.main([str(listing), "-o", str(table)])
    with gzip.open(zipped, "wb") as fh:
        fh.write(text.encode("ascii"))
    r = dict(tmp=tmp, model=model, fa=fa, seqs=seqs, table_path=str(table))
    b = lambda tag: ("--boundaries", str(tmp / tag))
    r["plain"] = _evaluate(tmp, "plain", model, str(listing), fa)
    r["run"] = _evaluate(tmp, "run", model, str(listing), fa, *b("run"))
    r["again"] = _evaluate(tmp, "again", model, str(listing), fa, *b("again"))
    r["table"] = _evaluate(tmp, "table", model, str(table), fa, *b("table"))
    r["gz"] = _evaluate(tmp, "gz", model, str(zipped), fa, *b("gz"))
    r["join"] = _evaluate(tmp, "join", model, str(listing), fa, *b("join"), "--boundary_join", "0", "--boundary_max", "64")
    r["w64"] = _evaluate(tmp, "w64", model, str(listing), fa, *b("w64"), "--boundary_max", "64")
    others = lambda tag: ("--curves", str(tmp / tag), "--strata", str(tmp / tag), "--offtarget", str(tmp / tag))
    r["all"] = _evaluate(tmp, "all", model, str(listing), fa, *b("all"), *others("all"))
    r["three"] = _evaluate(tmp, "three", model, str(listing), fa, *others("three"))
    main(["predict", model, fa, "--output", str(tmp / "pred.tsv")])
    return r


def _paint(rows, st, en):
    """The label track of [st, en): the smallest label among the rows that cover a base, 0 where none does."""
    t = np.zeros(en - st, np.int8)
    for q in sorted(rows, key=lambda q: -int(q["label"])):
        a, e = min(max(int(q["start"]), st), en), min(max(int(q["end"]), st), en)
        if e > a:
            t[a - st:e - st] = int(q["label"])
    return t


def _statement(run, W, join=None):
    """A boundaries.Boundaries filled from the table form of the annotation and predict's rows, record by record, in numpy."""
    from deepgrp_amd import boundaries, evaluation
    from deepgrp_amd.curves import need_of
    ann = evaluation.read_annotation(run["table_path"], REPEATS)
    pred = {}
    for line in open(run["tmp"] / "pred.tsv"):
        f = line.rstrip("\n").split("\t")
        pred.setdefault(f[1].split()[0], []).append((int(f[2]), int(f[3]), int(f[4]), 0))
    assert sorted(pred) == ["chr1", "ctgS"]
    bd = boundaries.Boundaries(5, W, join)
    for name, seq in run["seqs"].items():
        nonn = np.flatnonzero(np.frombuffer(seq, np.uint8) != ord("N"))
        st, en = int(nonn[0]), int(nonn[-1]) + 1
        p_rows = np.array(pred[name], SEG)
        t_rows = np.ascontiguousarray(ann[name], SEG)
        truth, called = _paint(t_rows, st, en), _paint(p_rows, st, en)
        units = t_rows if join is None else boundaries.join_rows(t_rows, join)
        for view, (rows, track) in enumerate(((units, called), (p_rows, truth))):
            b = boundaries.reference_bounds([st], [en - st], [track], [rows], W)
            clen = np.maximum(np.clip(rows["end"], st, en) - np.clip(rows["start"], st, en), 0)
            frag, edge, tally, flag = boundaries.reference_bound_hist([st], [en - st], [rows], b, need_of(THETA, clen), 5, W)
            assert flag == 0
            bd.count(view, frag, edge, tally)
    return bd


def test_both_files_and_the_json_key_equal_numpy_over_predicts_rows_and_the_annotation(run):
    from deepgrp_amd import boundaries
    tmp = run["tmp"]
    assert sorted(f for f in os.listdir(tmp) if f.startswith(("run.", ".run"))) == ["run.boundaries.tsv", "run.fragments.tsv", "run.json"]
    bd = _statement(run, 200)
    # the world holds what the flag is for: found rows in both views, exact and inexact edges on either side, elements in pieces
    assert bd.tally[0, :, 0].sum() > 5 and bd.tally[1, :, 0].sum() > 5 and bd.frag[:, :, 1].sum() > 5
    assert bd.edge[:, :, :, :200].sum() > 0 and bd.edge[:, :, :, 201:].sum() > 0
    assert bd.edge[0, :, 0, :200].sum() > 0                               # elements listed late: the predicted run begins in front of them
    assert (tmp / "run.boundaries.tsv").read_text() == boundaries.boundaries_tsv(bd.edge, 200)
    assert (tmp / "run.fragments.tsv").read_text() == boundaries.fragments_tsv(bd.frag)
    _text, js = run["run"]
    assert js["boundaries"] == json.loads(json.dumps(bd.summary()))
    assert js["boundaries"]["max"] == 200 and js["boundaries"]["join"] is None
    for v, (total, found) in enumerate((("elements", "found"), ("segments", "supported"))):
        view = js["boundaries"]["views"][("element", "row")[v]]
        assert [c["rows"] for c in view] == js[total] and [c["found"] for c in view] == js[found]       # the rule is evaluate's own
    lines = (tmp / "run.boundaries.tsv").read_text().splitlines()
    assert lines[0].startswith("# offset: ") and lines[1] == "view\tclass\tside\toffset\tcount\tshare"
    w64 = _statement(run, 64)
    assert (tmp / "w64.boundaries.tsv").read_text() == boundaries.boundaries_tsv(w64.edge, 64)
    assert (tmp / "w64.fragments.tsv").read_text() == (tmp / "run.fragments.tsv").read_text()


def test_the_report_is_byte_identical_and_the_json_gains_one_key(run):
    (plain_text, plain), (text, js) = run["plain"], run["run"]
    assert text == plain_text and text.startswith("#class\t")
    js = dict(js)
    assert "boundaries" not in plain
    s = js.pop("boundaries")
    assert js == plain
    assert sorted(s) == ["join", "max", "views"] and sorted(s["views"]) == ["element", "row"] and len(s["views"]["row"]) == 5
    for key in ("found", "exact_start", "exact_end", "exact_both", "within_10_start", "within_10_end", "median_abs_start", "median_abs_end",
                "mean_runs", "share_runs_ge_2"):
        assert key in s["views"]["element"][1]


def test_two_runs_the_table_form_and_the_gzip_listing_write_identical_files(run):
    tmp = run["tmp"]
    for other in ("again", "table", "gz"):
        for suffix in SUFFIXES:
            assert (tmp / ("run" + suffix)).read_bytes() == (tmp / (other + suffix)).read_bytes(), (other, suffix)
    assert run["again"] == run["run"]
    for other in ("table", "gz"):
        (text, js), (want_text, want) = run[other], run["run"]
        js, want = dict(js), dict(want)
        js.pop("annotation"), want.pop("annotation")
        assert text == want_text and js == want


def test_join_0_changes_the_element_view_and_leaves_the_row_view(run):
    from deepgrp_amd import boundaries
    tmp = run["tmp"]
    joined, apart = _statement(run, 64, 0), _statement(run, 64)
    assert (tmp / "join.boundaries.tsv").read_text() == boundaries.boundaries_tsv(joined.edge, 64, 0)
    assert (tmp / "join.fragments.tsv").read_text() == boundaries.fragments_tsv(joined.frag)
    assert joined.frag[0].sum() < apart.frag[0].sum() and not np.array_equal(joined.edge[0], apart.edge[0])
    assert np.array_equal(joined.frag[1], apart.frag[1]) and np.array_equal(joined.edge[1], apart.edge[1])
    for suffix in SUFFIXES:
        a, b = ((tmp / (tag + suffix)).read_text().splitlines() for tag in ("join", "w64"))
        assert [x for x in a if x.startswith("row\t")] == [x for x in b if x.startswith("row\t")]
        assert [x for x in a if x.startswith("element\t")] != [x for x in b if x.startswith("element\t")]
    (text, js), (want_text, want) = run["join"], run["w64"]
    assert text == want_text and js["boundaries"]["join"] == 0 and js["boundaries"]["views"]["row"] == want["boundaries"]["views"]["row"]
    assert js["boundaries"]["views"]["element"] != want["boundaries"]["views"]["element"] and js["elements"] == want["elements"]


def test_beside_curves_strata_and_offtarget_every_file_is_what_its_flag_writes_alone(run):
    tmp = run["tmp"]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("all.")) == [
        "all.bases.tsv", "all.boundaries.tsv", "all.fragments.tsv", "all.json", "all.offtarget.rows.tsv", "all.offtarget.tsv", "all.rows.tsv",
        "all.strata.bases.tsv", "all.strata.tsv"]
    for suffix in SUFFIXES:
        assert (tmp / ("all" + suffix)).read_bytes() == (tmp / ("run" + suffix)).read_bytes()
    for suffix in (".bases.tsv", ".rows.tsv", ".strata.tsv", ".strata.bases.tsv", ".offtarget.tsv", ".offtarget.rows.tsv"):
        assert (tmp / ("all" + suffix)).read_bytes() == (tmp / ("three" + suffix)).read_bytes()
    (text, js), (_t, alone), (_c, three) = run["all"], run["run"], run["three"]
    js = dict(js)
    assert text == run["plain"][0] and js.pop("boundaries") == alone["boundaries"] and js == three
