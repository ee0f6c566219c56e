"""`evaluate --strata` from the command line against statements built here: a synthetic record of 60 kb and a short one that goes
through the batch path, a small model, and a RepeatMasker listing whose lines carry divergences on both sides of the edges.  The
element lines against numpy over `predict`'s rows of the same records, the base lines against the painted keys, the report with and
without the flag, the table form (everything `NA`) and the host path of the listing."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

THETA = 0.5
DIVS = ["2.1", "7.5", "12.0", "18.3", "26.", "33.3", "x", "5.0", "4.99", "30"]          # `x`: not stated; 5.0 and 30 sit on edges
DIV_EDGES, LEN_EDGES = (50, 100, 150, 200, 250, 300), (100, 300, 1000, 3000)
N, FLANK = 60_000, 1000


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
        lines.append(rm_cases.out_line(ctg, int(b) + 1, int(e), "x", rm_cases.FAMILIES[int(lab) - 1], "+C"[k % 2]).replace("10.5", DIVS[k % len(DIVS)], 1))
        if k % 3 == 0:
            lines.append(rm_cases.out_line(ctg, int(b) + 1, int(e), "(CA)n", "Simple_repeat"))
        for j, flen in enumerate((50, 150, 400, 1200, 3500)):             # fragments of the planted run, every length bin
            if flen < int(e) - int(b):
                at = int(b) + (j * 137) % (int(e) - int(b) - flen)
                lines.append(rm_cases.out_line(ctg, at + 1, at + flen, "x", rm_cases.FAMILIES[int(lab) - 1]).replace("10.5", DIVS[(5 * k + j + 1) % len(DIVS)], 1))
    for j in range(8):                                                    # and rows wherever they fall: most of them are missed
        at, flen = FLANK + 2000 + 6500 * j, (80, 250, 900, 2500)[j % 4]
        lines.append(rm_cases.out_line("chr1", at + 1, at + flen, "x", rm_cases.FAMILIES[j % 4]).replace("10.5", DIVS[(j + 3) % len(DIVS)], 1))
    lines += [rm_cases.rmsk_line("chr1", FLANK + 100, FLANK + 900, "L2a", "LINE", "L2"),             # milliDiv 13: 1.3 %
              rm_cases.out_line("chr1", 20_001, 24_000, "x", "LINE/L1").replace("10.5", "21.7", 1),   # long, over whatever lies there
              rm_cases.out_line("chr1", 21_001, 21_050, "x", "LINE/L1").replace("10.5", "3.3", 1),    # nested, same label, lower stratum
              rm_cases.out_line("chr1", FLANK - 39, FLANK + 60, "x", "SINE/Alu").replace("10.5", "9.9", 1),   # sticks out of the evaluated span
              rm_cases.out_line("chr1", 10, 500, "x", "SINE/Alu"),                                    # wholly inside the N flank: no element
              rm_cases.out_line("ctgS", 101, 700, "x", "SINE/Alu").replace("10.5", "14.2", 1),
              rm_cases.out_line("ctgS", 1, 40, "x", "LINE/L1").replace("10.5", "0.0", 1),
              rm_cases.out_line("chrUn", 10, 500, "x", "SINE/MIR")]
    fa = tmp / "in.fa"
    with open(fa, "wb") as fh:
        for name, seq in (("chr1", long_seq), ("ctgS", short_seq)):
            fh.write(b">" + name.encode() + b" synthetic\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
    return str(fa), {"chr1": long_seq, "ctgS": short_seq}, lines


def _evaluate(tmp, tag, model, ann, fa, *flags):
    from deepgrp_amd.__main__ import main
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        main(["evaluate", model, ann, fa, "--json", str(tmp / f"{tag}.json")] + list(flags))
    js = json.load(open(tmp / f"{tag}.json"))
    return out.getvalue(), js


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd._scripts import parse_rm
    tmp = tmp_path_factory.mktemp("strata")
    model = _model(tmp)
    fa, seqs, lines = _inputs(tmp)
    text = rm_cases.HEADER + "\n".join(lines) + "\n"
    listing, table, host = tmp / "rm.out", tmp / "rm.bed", tmp / "rm_host.out"
    listing.write_text(text)
    parse_rm.main([str(listing), "-o", str(table)])
    host.write_bytes(b"# caf\xc3\xa9\n" + text.encode("ascii"))              # one byte outside plain ASCII, in a comment line
    r = dict(tmp=tmp, model=model, fa=fa, seqs=seqs, lines=lines, listing=str(listing))
    r["plain"] = _evaluate(tmp, "plain", model, str(listing), fa)
    r["strata"] = _evaluate(tmp, "strata", model, str(listing), fa, "--strata", str(tmp / "run"))
    r["again"] = _evaluate(tmp, "again", model, str(listing), fa, "--strata", str(tmp / "again"))
    r["table"] = _evaluate(tmp, "table", model, str(table), fa, "--strata", str(tmp / "tab"))
    r["host"] = _evaluate(tmp, "host", model, str(host), fa, "--strata", str(tmp / "host"))
    r["both"] = _evaluate(tmp, "both", model, str(listing), fa, "--strata", str(tmp / "both"), "--curves", str(tmp / "both"))
    r["curves"] = _evaluate(tmp, "curves", model, str(listing), fa, "--curves", str(tmp / "only"))
    main(["predict", model, fa, "--output", str(tmp / "pred.tsv")])
    return r


def _read(path):
    """[fields] of the lines that are not comments, and the comment lines."""
    rows, comments = [], []
    for line in open(path):
        (comments if line.startswith("#") else rows).append(line.rstrip("\n").split("\t"))
    return rows, comments


def _elements(run):
    """(label, stratum, clipped length, record name, clipped begin, clipped end) of the listing's kept rows, from its own lines."""
    from deepgrp_amd import annotation, strata
    from deepgrp_amd._scripts import parse_rm
    exact, one_off = parse_rm.pentamer_sets()
    out = []
    for line in run["lines"]:
        got = list(parse_rm.read_repeatmasker(exact, one_off, [line]))
        if not got or got[0].ctg not in run["seqs"] or not 1 <= got[0].typ <= 4:
            continue
        r = got[0]
        seq = np.frombuffer(run["seqs"][r.ctg], np.uint8)
        nonn = np.flatnonzero(seq != ord("N"))
        st, en = int(nonn[0]), int(nonn[-1]) + 1
        s = int(strata.div_bin([annotation.millidiv_of_line(line)], DIV_EDGES)[0]) * 5 + int(strata.len_bin([r.end - r.start], LEN_EDGES)[0])
        a, e = min(max(r.start, st), en), min(max(r.end, st), en)
        out.append((r.typ, s, max(e - a, 0), r.ctg, a, e))
    return out


def test_both_files_appear_and_nothing_else(run):
    names = sorted(f for f in os.listdir(run["tmp"]) if f.startswith(("run", ".run")))
    assert names == ["run.strata.bases.tsv", "run.strata.tsv"]
    rows, comments = _read(run["tmp"] / "run.strata.tsv")
    assert "overlapping annotation rows count twice" in "\t".join(comments[0])
    assert comments[1] == ["#class", "divergence", "length", "elements", "found", "recall", "element_bases", "element_hits", "base_recall"]
    assert len(rows) == 4 * (8 * 5 + 5 + 8 + 1)
    assert [r[1] for r in rows[:40:5]] == ["0-5", "5-10", "10-15", "15-20", "20-25", "25-30", "30+", "NA"]
    assert [r[2] for r in rows[:5]] == ["0-100", "100-300", "300-1000", "1000-3000", "3000+"]


def test_the_margins_equal_the_report(run):
    _text, js = run["strata"]
    rows, _c = _read(run["tmp"] / "run.strata.tsv")
    both = {int(r[0]): r for r in rows if r[1] == "*" and r[2] == "*"}
    assert sorted(both) == [1, 2, 3, 4]
    for c, r in both.items():
        assert (int(r[3]), int(r[4])) == (js["elements"][c], js["found"][c])
    assert sum(js["elements"]) > 20 and sum(js["found"]) > 0
    for c in range(1, 5):
        for col, star in ((1, 2), (2, 1)):                               # each margin sums to the `* *` line too
            part = [r for r in rows if int(r[0]) == c and r[star] == "*" and r[col] != "*"]
            assert sum(int(r[3]) for r in part) == js["elements"][c] and sum(int(r[4]) for r in part) == js["found"][c]
    s = js["strata"]
    assert s["divergence_edges"] == [5.0, 10.0, 15.0, 20.0, 25.0, 30.0] and s["length_edges"] == [100, 300, 1000, 3000] and s["bins"] == 100
    by_div = {(int(r[0]), r[1]): r[5] for r in rows if r[2] == "*" and r[1] != "*"}
    for c in range(1, 5):
        for i, d in enumerate(s["divergence_bins"]):
            assert repr(float("nan") if s["recall_by_divergence"][c][i] is None else s["recall_by_divergence"][c][i]) == by_div[(c, d)]


def test_each_stratum_line_is_numpy_over_predicts_rows(run):
    pred = {}
    for line in open(run["tmp"] / "pred.tsv"):
        f = line.rstrip("\n").split("\t")
        pred.setdefault(f[1].split()[0], []).append((int(f[2]), int(f[3]), int(f[4])))
    assert sorted(pred) == ["chr1", "ctgS"]
    track = {}
    for name, seq in run["seqs"].items():
        t = np.zeros(len(seq), np.int64)
        for s, e, lab in pred[name]:
            t[s:e] = lab
        track[name] = t
    want = np.zeros((4, 5, 40), np.int64)
    for lab, s, clen, name, a, e in _elements(run):
        if clen == 0:
            continue
        hits = int((track[name][a:e] == lab).sum())
        want[0, lab, s] += 1
        want[1, lab, s] += hits >= THETA * clen
        want[2, lab, s] += clen
        want[3, lab, s] += hits
    assert (want[0].sum(axis=0) > 0).sum() >= 8 and want[1].sum() > 0     # several strata hold elements, some are found
    assert want[0, :, 35:].sum() > 0 and want[0, :, :5].sum() > 0         # NA and the first divergence bin among them
    rows, _c = _read(run["tmp"] / "run.strata.tsv")
    got = np.zeros_like(want)
    for k, r in enumerate(rows[:4 * 40]):
        c, s = 1 + k // 40, k % 40
        assert int(r[0]) == c
        got[:, c, s] = [int(r[3]), int(r[4]), int(r[6]), int(r[7])]
    np.testing.assert_array_equal(got, want)


def test_bases_at_threshold_0_are_the_painted_bases(run):
    from deepgrp_amd import strata
    SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
    painted = np.zeros((5, 40), np.int64)
    by_rec = {}
    for lab, s, clen, name, a, e in _elements(run):
        by_rec.setdefault(name, []).append((a, e, lab, s))
    for name, items in by_rec.items():
        rows = np.zeros(len(items), SEG)
        rows["start"], rows["end"], rows["label"] = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
        key = strata.reference_keys([0], [len(run["seqs"][name])], [rows], [np.array([i[3] for i in items], np.uint8)])[0]
        live = key[key != 0xFFFFFFFF]
        np.add.at(painted, ((live >> 8).astype(np.int64), (live & 255).astype(np.int64)), 1)
    rows, comments = _read(run["tmp"] / "run.strata.bases.tsv")
    assert comments == [["#class", "divergence", "length", "threshold", "TP", "FN", "TPR"]] and len(rows) == 4 * 40 * 100
    got = np.zeros_like(painted)
    for k in range(4 * 40):
        r = rows[k * 100]
        assert r[3] == "0.0" and int(r[5]) == 0
        got[1 + k // 40, k % 40] = int(r[4])
        tp = [int(x[4]) for x in rows[k * 100:(k + 1) * 100]]
        assert all(a >= b for a, b in zip(tp, tp[1:])) and all(int(x[4]) + int(x[5]) == tp[0] for x in rows[k * 100:(k + 1) * 100])
    np.testing.assert_array_equal(got, painted)
    _text, js = run["strata"]
    assert got.sum(axis=1)[1:].tolist() == [sum(js["confusion_matrix"][c]) for c in range(1, 5)]     # every annotated base once


def test_the_report_is_byte_identical_and_the_json_gains_one_key(run):
    (plain_text, plain), (text, js) = run["plain"], run["strata"]
    assert text == plain_text and text.startswith("#class\t")
    js = dict(js)
    assert "strata" not in plain and sorted(js.pop("strata")) == ["bins", "divergence_bins", "divergence_edges", "length_bins", "length_edges",
                                                                  "recall_by_divergence", "recall_by_length"]
    assert js == plain


def test_two_runs_write_identical_files(run):
    for suffix in (".strata.tsv", ".strata.bases.tsv"):
        assert (run["tmp"] / ("run" + suffix)).read_bytes() == (run["tmp"] / ("again" + suffix)).read_bytes()
    assert run["again"] == run["strata"]


def test_with_curves_both_sets_of_files_are_what_each_flag_writes_alone(run):
    tmp = run["tmp"]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("both.")) == ["both.bases.tsv", "both.json", "both.rows.tsv", "both.strata.bases.tsv",
                                                                           "both.strata.tsv"]
    for suffix in (".strata.tsv", ".strata.bases.tsv"):
        assert (tmp / ("both" + suffix)).read_bytes() == (tmp / ("run" + suffix)).read_bytes()
    for suffix in (".bases.tsv", ".rows.tsv"):
        assert (tmp / ("both" + suffix)).read_bytes() == (tmp / ("only" + suffix)).read_bytes()
    (text, js), (_t, with_strata), (_c, with_curves) = run["both"], run["strata"], run["curves"]
    js = dict(js)
    assert text == run["plain"][0] and js.pop("strata") == with_strata["strata"] and js == with_curves


def test_the_table_form_puts_everything_in_NA(run):
    rows, _c = _read(run["tmp"] / "tab.strata.tsv")
    listing_rows, _c = _read(run["tmp"] / "run.strata.tsv")
    stated = [r for r in rows if r[1] not in ("NA", "*")]
    assert stated and all(r[3:5] == ["0", "0"] and r[6:8] == ["0", "0"] for r in stated)
    pick = lambda rs, d: {(r[0], r[2]): r[3:] for r in rs if r[1] == d}
    assert pick(rows, "NA") == pick(listing_rows, "*") == pick(rows, "*")      # the length margins of the listing, all under NA
    (text, js), (_t, with_listing) = run["table"], run["strata"]
    assert text == run["plain"][0] and js["elements"] == with_listing["elements"] and js["found"] == with_listing["found"]
    bases, _c = _read(run["tmp"] / "tab.strata.bases.tsv")
    assert all(int(r[4]) == 0 and int(r[5]) == 0 for r in bases if r[1] != "NA") and sum(int(r[4]) for r in bases if r[3] == "0.0") > 2000


def test_the_host_path_of_the_listing_gives_the_same_files(run):
    from deepgrp_amd import annotation
    assert annotation.read_listing(run["listing"]).route == "device"
    assert annotation.read_listing(str(run["tmp"] / "rm_host.out")).route == "host"
    for suffix in (".strata.tsv", ".strata.bases.tsv"):
        assert (run["tmp"] / ("run" + suffix)).read_bytes() == (run["tmp"] / ("host" + suffix)).read_bytes()
    (text, js), (want_text, want) = run["host"], run["strata"]
    js, want = dict(js), dict(want)
    assert js.pop("annotation").endswith("rm_host.out") and want.pop("annotation").endswith("rm.out")
    assert text == want_text and js == want
