"""`evaluate --offtarget` from the command line against statements built here: a synthetic record of 60 kb and a short one that goes
through the batch path, a small model, and a RepeatMasker listing with rows of the modelled classes, other families over the planted
repeats of a class that --repeats leaves out, and planted repeats the listing does not mention.  Both files against numpy over
`predict`'s rows and the listing's own lines, the report with and without the flag, two runs, the gzip and the host path of the
listing, the table form, and the flag beside --strata and --curves."""
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
REPEATS = [1, 2, 3]                                                     # class 4 (LINE/L1) is predicted but not modelled by the annotation
N, FLANK = 60_000, 1000
NONE = 0xFFFFFFFF
OTHER = ("LINE/L1", "LINE/CR1", "DNA/hAT-Charlie", "LINE/L1", "LTR/ERVK")


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
        if lab == 4:                                                     # the class outside --repeats: other families lie there
            lines.append(rm_cases.out_line(ctg, b + 1, e, "x", OTHER[k % len(OTHER)], "+C"[k % 2]))
            if k % 2:
                lines.append(rm_cases.out_line(ctg, b + 11, e + 40, "x", "DNA/hAT"))        # a second family over it: the first in byte order wins
        elif k % 5 == 0:
            continue                                                     # a planted repeat the listing does not mention: `none`
        else:
            lines.append(rm_cases.out_line(ctg, b + 1, e, "x", rm_cases.FAMILIES[lab - 1], "+C"[k % 2]))
            if k % 3 == 0:
                lines.append(rm_cases.out_line(ctg, max(b - 30, 0) + 1, e + 30, "x", "Low_complexity"))   # an un-modelled row under a modelled one
    for j in range(8):                                                   # rows wherever they fall
        at, flen = FLANK + 2000 + 6500 * j, (80, 250, 900, 2500)[j % 4]
        lines.append(rm_cases.out_line("chr1", at + 1, at + flen, "x", (rm_cases.FAMILIES[j % 4], "SINE/MIR", "Unknown")[j % 3]))
    lines += [rm_cases.rmsk_line("chr1", FLANK + 100, FLANK + 900, "L2a", "LINE", "L2"),
              rm_cases.rmsk_line("chr1", FLANK + 700, FLANK + 1900, "x", "Unknown", "Unknown"),
              rm_cases.out_line("chr1", FLANK - 39, FLANK + 60, "x", "SINE/Alu"),                     # sticks out of the evaluated span
              rm_cases.out_line("chr1", 10, 500, "x", "LINE/L2"),                                     # wholly inside the N flank
              rm_cases.out_line("ctgS", 101, 700, "x", "SINE/Alu"), rm_cases.out_line("ctgS", 1, 400, "x", "LINE/L1"),
              rm_cases.out_line("ctgS", 901, 1500, "(CA)n", "Simple_repeat"),
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
        main(["evaluate", model, ann, fa, "--repeats", ",".join(map(str, REPEATS)), "--json", str(tmp / f"{tag}.json")] + list(flags))
    js = json.load(open(tmp / f"{tag}.json"))
    return out.getvalue(), js


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd._scripts import parse_rm
    tmp = tmp_path_factory.mktemp("offtarget")
    model = _model(tmp)
    fa, seqs, lines = _inputs(tmp)
    text = rm_cases.HEADER + "\n".join(lines) + "\n"
    listing, table, host, zipped = tmp / "rm.out", tmp / "rm.bed", tmp / "rm_host.out", tmp / "rm.out.gz"
    listing.write_text(text)
    parse_rm.main([str(listing), "-o", str(table)])
    host.write_bytes(b"# caf\xc3\xa9\n" + text.encode("ascii"))              # one byte outside plain ASCII, in a comment line
    with gzip.open(zipped, "wb") as fh:
        fh.write(text.encode("ascii"))
    r = dict(tmp=tmp, model=model, fa=fa, seqs=seqs, lines=lines, listing=str(listing), table=str(table))
    r["plain"] = _evaluate(tmp, "plain", model, str(listing), fa)
    r["off"] = _evaluate(tmp, "off", model, str(listing), fa, "--offtarget", str(tmp / "run"))
    r["again"] = _evaluate(tmp, "again", model, str(listing), fa, "--offtarget", str(tmp / "again"))
    r["class"] = _evaluate(tmp, "class", model, str(listing), fa, "--offtarget", str(tmp / "cls"), "--offtarget_by", "class")
    r["gz"] = _evaluate(tmp, "gz", model, str(zipped), fa, "--offtarget", str(tmp / "gz"))
    r["host"] = _evaluate(tmp, "host", model, str(host), fa, "--offtarget", str(tmp / "host"))
    r["all"] = _evaluate(tmp, "all", model, str(listing), fa, "--offtarget", str(tmp / "all"), "--strata", str(tmp / "all"), "--curves", str(tmp / "all"))
    r["two"] = _evaluate(tmp, "two", model, str(listing), fa, "--strata", str(tmp / "two"), "--curves", str(tmp / "two"))
    main(["predict", model, fa, "--output", str(tmp / "pred.tsv")])
    return r


def _statement(run):
    """(hist [2, 5, K], rows [5, 6], families) from the listing's own lines (parse_rm) and predict's rows, a loop per row."""
    from deepgrp_amd._scripts import parse_rm
    exact, one_off = parse_rm.pentamer_sets()
    parsed = []
    for line in run["lines"]:
        r = parse_rm.parse_line(line)
        assert r.ctg is not None
        numbered = list(parse_rm.read_repeatmasker(exact, one_off, [line]))
        parsed.append((r.ctg, r.start, r.end, numbered[0].typ if numbered else 0, r.fam))
    families = sorted(set(p[4] for p in parsed), key=lambda s: s.encode())
    K = 64 + len(families) + 1
    pred = {}
    for line in open(run["tmp"] / "pred.tsv"):
        f = line.rstrip("\n").split("\t")
        pred.setdefault(f[1].split()[0], []).append((int(f[2]), int(f[3]), int(f[4])))
    assert sorted(pred) == ["chr1", "ctgS"]
    hist, rows = np.zeros((2, 5, K), np.int64), np.zeros((5, 6), np.int64)
    for name, seq in run["seqs"].items():
        arr = np.frombuffer(seq, np.uint8)
        nonn = np.flatnonzero(arr != ord("N"))
        st, en = int(nonn[0]), int(nonn[-1]) + 1
        keys = np.full(len(seq), NONE, np.int64)
        for ctg, b, e, typ, fam in parsed:
            if ctg == name and e > b:
                key = typ if typ in REPEATS else 64 + families.index(fam)
                keys[b:e] = np.minimum(keys[b:e], key)
        col = np.where(keys == NONE, K - 1, keys)
        track = np.zeros(len(seq), np.int64)
        for s, e, lab in pred[name]:
            track[s:e] = lab
        np.add.at(hist[0], (track[st:en], col[st:en]), 1)
        for s, e, lab in pred[name]:
            a, z = min(max(s, st), en), min(max(e, st), en)
            if z <= a:
                continue
            span = keys[a:z]
            four = [int((span == lab).sum()), int(((span < 64) & (span != lab)).sum()), int(((span >= 64) & (span != NONE)).sum()),
                    int((span == NONE).sum())]
            rows[lab, 0] += 1
            if four[0] >= THETA * (z - a):
                rows[lab, 1] += 1
            else:
                rows[lab, 2 + four.index(max(four))] += 1
                np.add.at(hist[1], (np.full(z - a, lab), col[a:z]), 1)
    return hist, rows, families


def test_both_files_equal_numpy_over_predicts_rows_and_the_listing(run):
    from deepgrp_amd import offtarget
    names = sorted(f for f in os.listdir(run["tmp"]) if f.startswith(("run", ".run")))
    assert names == ["run.offtarget.rows.tsv", "run.offtarget.tsv"]
    hist, rows, families = _statement(run)
    # the world holds what the flag is for: predicted class 4 on other families, predicted repeats on nothing, modelled over un-modelled
    assert hist[0, 4, 64:-1].sum() > 1000 and hist[0, 1:4, -1].sum() > 500 and hist[0, 0, 64:-1].sum() > 0 and hist[1].sum() > 1000
    assert rows[4, 4] > 0 and rows[1:4, 1].sum() > 0 and rows[:, 5].sum() > 0
    assert (run["tmp"] / "run.offtarget.tsv").read_text() == offtarget.offtarget_tsv(hist, families, "family")
    assert (run["tmp"] / "run.offtarget.rows.tsv").read_text() == offtarget.rows_tsv(rows)
    assert (run["tmp"] / "cls.offtarget.tsv").read_text() == offtarget.offtarget_tsv(hist, families, "class")
    assert (run["tmp"] / "cls.offtarget.rows.tsv").read_text() == offtarget.rows_tsv(rows)
    _text, js = run["off"]
    assert [int(r[0]) for r in rows] == js["segments"] and [int(r[1]) for r in rows] == js["supported"]
    cnf = np.asarray(js["confusion_matrix"])
    for lab in REPEATS:                                                  # the columns of the labels are the confusion matrix, transposed
        assert hist[0, :, lab].tolist() == cnf[lab].tolist()
    assert hist[0, :, 64:].sum(axis=1).tolist() == cnf[0].tolist()
    lines = (run["tmp"] / "run.offtarget.tsv").read_text().splitlines()
    assert lines[0].startswith("# ") and lines[1] == "scope\tpredicted\tunder\tbases\tshare"
    for scope in (0, 1):                                                 # every family under predicted class 4 has its line
        under = [families[i] for i in np.flatnonzero(hist[scope, 4, 64:-1])]
        assert len(under) >= 2 and all(f"{('all', 'unsupported')[scope]}\t4\t{nm}\t" in "\n".join(lines) for nm in under)


def test_the_report_is_byte_identical_and_the_json_gains_one_key(run):
    (plain_text, plain), (text, js) = run["plain"], run["off"]
    assert text == plain_text and text.startswith("#class\t")
    js = dict(js)
    assert "offtarget" not in plain
    s = js.pop("offtarget")
    assert js == plain
    assert sorted(s) == ["by", "classes", "families"] and s["by"] == "family" and len(s["classes"]) == 5
    c4 = s["classes"][4]
    assert c4["offtarget"] > 0.5 and c4["top"][0][0] in ("LINE/L1", "DNA/hAT", "LINE/CR1", "DNA/hAT-Charlie", "LTR/ERVK")
    assert abs(c4["modelled"] + c4["offtarget"] + c4["unannotated"] - 1.0) < 1e-12
    assert run["class"][1]["offtarget"]["by"] == "class" and run["class"][0] == plain_text


def test_two_runs_the_gzip_and_the_host_path_write_identical_files(run):
    from deepgrp_amd import annotation
    tmp = run["tmp"]
    assert annotation.read_listing(run["listing"], all_rows=True).route == "device"
    assert annotation.read_listing(str(tmp / "rm.out.gz"), all_rows=True).route == "device"
    assert annotation.read_listing(str(tmp / "rm_host.out"), all_rows=True).route == "host"
    for other in ("again", "gz", "host"):
        for suffix in (".offtarget.tsv", ".offtarget.rows.tsv"):
            assert (tmp / ("run" + suffix)).read_bytes() == (tmp / (other + suffix)).read_bytes(), (other, suffix)
    assert run["again"] == run["off"]
    for other in ("gz", "host"):
        (text, js), (want_text, want) = run[other], run["off"]
        js, want = dict(js), dict(want)
        js.pop("annotation"), want.pop("annotation")
        assert text == want_text and js == want


def test_beside_strata_and_curves_every_file_is_what_its_flag_writes_alone(run):
    tmp = run["tmp"]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("all.")) == ["all.bases.tsv", "all.json", "all.offtarget.rows.tsv", "all.offtarget.tsv",
                                                                          "all.rows.tsv", "all.strata.bases.tsv", "all.strata.tsv"]
    for suffix in (".offtarget.tsv", ".offtarget.rows.tsv"):
        assert (tmp / ("all" + suffix)).read_bytes() == (tmp / ("run" + suffix)).read_bytes()
    for suffix in (".bases.tsv", ".rows.tsv", ".strata.tsv", ".strata.bases.tsv"):
        assert (tmp / ("all" + suffix)).read_bytes() == (tmp / ("two" + suffix)).read_bytes()
    (text, js), (_t, off), (_c, two) = run["all"], run["off"], run["two"]
    js = dict(js)
    assert text == run["plain"][0] and js.pop("offtarget") == off["offtarget"] and js == two


def test_the_table_form_is_refused_by_name(run):
    from deepgrp_amd.__main__ import main
    tmp = run["tmp"]
    with pytest.raises(SystemExit) as e:
        main(["evaluate", run["model"], run["table"], run["fa"], "--offtarget", str(tmp / "tab")])
    assert "--offtarget" in str(e.value) and "rm.bed" in str(e.value) and "table" in str(e.value) and "genome.fa.out" in str(e.value)
    assert not [f for f in os.listdir(tmp) if f.startswith("tab")]
