"""predict --bed_dir --bed_rmout end to end, each run in a child process (tests/rmout_cli_child.py): on a file of one long record (the
record path) and on a file of 300 short records (the batch path) the `.out` is rmout.HEADER + rmout.reference_lines composed from
the run's own rows and scores, and the inflated `.out.gz` at --gzip_level 0 and 1 is the same bytes; the IDs run through records and
batches, with and without --rmout_join; --bed_min_score, --rmout_repeats and --bed_names take effect; the TSV is the bytes of a run
without the flag; the `parse_rm` console script, `compare` and `evaluate` read the listing back as the rows it was written from
(the `.out.gz` through the device listing parser, named by --annotation_format: the sniffer inflates the first BGZF member, which holds
the title lines alone); an all-N record, a record without a base, .2bit and stdin inputs; a record name
that cannot be written."""
import json
import os
import pickle
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from deepgrp_amd import gz, rmout  # noqa: E402

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
KW = {"b": 7, "s": 4, "x": 5, "l": 3}
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
CHILD = os.path.join(ROOT, "tests", "rmout_cli_child.py")
INFO_KEYS = {"model", "annotation", "inputs", "repeats", "options", "predicted", "predicted_format", "predicted_rows"}
JOIN = 40


def _fasta(recs):
    return b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs)


def _child(tmp, jobs, stdin=None, fails=None):
    """The jobs one after the other in ONE child process -> its stderr.  fails: the words of the error it must end with."""
    spec = os.path.join(str(tmp), "jobs%d.json" % len(os.listdir(str(tmp))))
    with open(spec, "w") as fh:
        json.dump(jobs, fh)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, CHILD, spec], cwd=ROOT, env=env, capture_output=True, timeout=300, input=stdin)
    if fails is not None:
        assert r.returncode != 0 and fails in r.stderr.decode("utf-8", "replace"), r.stderr.decode("utf-8", "replace")[-3000:]
    else:
        assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    return r.stderr.decode("utf-8", "replace")


def _inflate(data):
    out, off = [], 0
    while off < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[off:]))
        off = len(data) - len(d.unused_data)
    return b"".join(out)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _state(composed, min_score=0, pairs=None, join=None):
    """The listing of a composition: the header, then every record's lines with the IDs running on -> (text, lines, IDs)."""
    pairs = rmout.pairs_of_repeats(range(1, composed["classes"])) if pairs is None else pairs
    out, lines, ids = [rmout.HEADER], 0, 0
    for name, rows, scores, rec_end in composed["records"]:
        text, n, used = rmout.reference_lines([name], False, rows, scores, min_score, [rec_end], pairs, join, ids)
        out.append(text)
        lines, ids = lines + n, ids + used
    return b"".join(out), lines, ids


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The inputs and, from one child process, their compositions."""
    d = tmp_path_factory.mktemp("rmout_in")
    rng = np.random.default_rng(43)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    one = d / "one.fa"
    one.write_bytes(_fasta([(b"long one record", b"NNN" + seq(300_000) + b"NNNNN")]))  # above runner.SMALL_RECORD: on its own
    many = d / "many.fa"
    many.write_bytes(_fasta([(b"ctg%d some words" % i, seq(int(rng.integers(60, 900)))) for i in range(300)]))
    mix = d / "mix.fa"                                                                # a record without a base between records with rows
    mix_recs = [(b"m1 a", seq(1500)), (b"none no sequence at all", b""), (b"m2", b"NN" + seq(900) + b"N"), (b"m3", seq(2500))]
    mix.write_bytes(_fasta(mix_recs))
    paths = {"one": str(one), "many": str(many), "mix": str(mix)}
    _child(d, [{"compose": dict(model_file=MODEL, path=paths[k], out=str(d / (k + ".pkl")), flags=KW)} for k in paths])
    composed = {}
    for k in paths:
        with open(d / (k + ".pkl"), "rb") as fh:
            composed[k] = pickle.load(fh)
    assert composed["one"]["classes"] == 5
    return paths, composed, mix_recs


@pytest.fixture(scope="module")
def runs(tmp_path_factory, inputs):
    """One child: no flag, plain, both gzip levels, --rmout_join, then the readers on what was written."""
    paths, _composed, _mix = inputs
    t = tmp_path_factory.mktemp("rmout_runs")
    base = FLAGS + ["predict", MODEL, paths["one"], paths["many"]]
    run = lambda k, *more: {"main": base + ["--output", str(t / (k + ".tsv")), "--bed_dir", str(t / k), "--bed_rmout"] + list(more)}
    jobs = [{"main": base + ["--output", str(t / "none.tsv")]}, run("plain"), run("gz0", "--bed_gzip", "--gzip_level", "0"),
            run("gz1", "--bed_gzip", "--gzip_level", "1"), run("join", "--rmout_join", str(JOIN)),
            {"main": FLAGS + ["predict", MODEL, paths["many"], "--output", str(t / "many.tsv")]}]
    listing, packed, ann = str(t / "plain" / "many.fa.out"), str(t / "gz1" / "many.fa.out.gz"), str(t / "ann.bed")
    jobs += [{"parse_rm": [listing, "-o", ann]},
             {"main": ["compare", str(t / "many.tsv"), packed, paths["many"], "--repeats", "1,2,3,4", "--annotation_format", "repeatmasker",
                       "--json", str(t / "c_gz.json"),
                       "--output", str(t / "c_gz.tsv")]},
             {"main": FLAGS + ["evaluate", MODEL, listing, paths["many"], "--json", str(t / "e.json"), "--output", str(t / "e.tsv")]},
             {"main": ["compare", listing, ann, paths["many"], "--json", str(t / "c_out.json"), "--output", str(t / "c_out.tsv")]},
             {"main": ["compare", str(t / "many.tsv"), ann, paths["many"], "--json", str(t / "c_tsv.json"), "--output", str(t / "c_tsv.tsv")]}]
    _child(t, jobs)
    return t


def test_the_files_are_the_statement_and_the_tsv_is_unchanged(inputs, runs):
    paths, composed, _mix = inputs
    t = runs
    tsv = _read(t / "none.tsv")
    assert tsv == _read(t / "plain.tsv") == _read(t / "gz0.tsv") == _read(t / "gz1.tsv") == _read(t / "join.tsv")
    assert sorted(os.listdir(t / "plain")) == ["many.fa.out", "one.fa.out"] == sorted(os.listdir(t / "join"))
    assert sorted(os.listdir(t / "gz0")) == ["many.fa.out.gz", "one.fa.out.gz"] == sorted(os.listdir(t / "gz1"))
    for key in ("one", "many"):
        stem = key + ".fa"
        want, lines, ids = _state(composed[key])
        text = _read(t / "plain" / (stem + ".out"))
        assert lines == ids > 50 and text == want
        for level in (0, 1):
            data = _read(t / ("gz%d" % level) / (stem + ".out.gz"))
            assert data.startswith(rmout.header_member(level)) and data.endswith(gz.BGZF_EOF) and _inflate(data) == want
        # one line per TSV row of this input with start+1 and end; the IDs run through records and batches
        rows = [ln.split("\t") for ln in tsv.decode().split("\n")[:-1] if ln.split("\t")[0] == paths[key]]
        cols = [ln.split() for ln in text.split(b"\n")[3:-1]]
        assert len(rows) == len(cols) == lines
        assert [(int(r[2]) + 1, int(r[3])) for r in rows] == [(int(c[5]), int(c[6])) for c in cols]
        assert [int(c[14]) for c in cols] == list(range(1, lines + 1))
        pairs = rmout.pairs_of_repeats(range(1, 5))
        assert all((c[9], c[10]) == pairs[int(r[4]) - 1] for r, c in zip(rows, cols))
        # --rmout_join: fewer IDs than lines, still running through the file
        joined, jlines, jids = _state(composed[key], join=JOIN)
        assert _read(t / "join" / (stem + ".out")) == joined and jlines == lines and 0 < jids < lines
        assert int(joined.split(b"\n")[-2].split()[14]) == jids
    last = _read(t / "plain" / "one.fa.out").split(b"\n")[-2].split()
    assert composed["one"]["records"][0][3] == 300_003 == int(last[6]) + int(last[7][1:-1])       # the five N behind the bases are not counted


def test_the_readers_take_the_listing_back(inputs, runs):
    paths, composed, _mix = inputs
    t = runs
    tsv = [ln.split("\t") for ln in _read(t / "many.tsv").decode().split("\n")[:-1]]
    table = [ln.split("\t") for ln in _read(t / "ann.bed").decode().split("\n")[:-1]]
    # parse_rm's table: contig, start, end and the number of the label, row for row
    assert [(r[1].split()[0], r[2], r[3], r[4]) for r in tsv] == [(a[0], a[1], a[2], a[3]) for a in table] and len(table) > 50
    load = lambda k: json.load(open(t / (k + ".json")))
    for key in ("c_gz", "e"):                                                         # the listing as ANNOTATION: the rows against themselves
        rep = load(key)
        cnf = np.array(rep["confusion_matrix"])
        assert (cnf == np.diag(np.diag(cnf))).all(), key
        present = [c for c in range(5) if cnf[c, c]]
        assert len(present) >= 2 and all(rep["metrics"]["TPR"][c] == 1.0 and rep["metrics"]["PPV"][c] == 1.0 for c in present), key
    # the listing as PREDICTED: the report of the TSV to the byte outside the info keys
    assert _read(t / "c_out.tsv") == _read(t / "c_tsv.tsv")
    a, b = load("c_out"), load("c_tsv")
    assert {k: v for k, v in a.items() if k not in INFO_KEYS} == {k: v for k, v in b.items() if k not in INFO_KEYS}
    assert a["predicted_format"] == "repeatmasker" and b["predicted_format"] == "tsv"


def test_min_score_repeats_and_names_take_effect(tmp_path, inputs):
    paths, composed, _mix = inputs
    full, n_all, _i = _state(composed["many"])
    scores = sorted({int(ln.split()[0]) for ln in full.split(b"\n")[3:-1]})
    assert len(scores) > 1, "every row has the same score: the filter cannot be told from no filter"
    low = scores[len(scores) // 2]
    names = ["LTR-1#LTR/Gypsy", "AluY#SINE/Alu", "x" * 200 + "#Unknown", "L1HS#LINE/L1"]
    a, b = tmp_path / "a", tmp_path / "b"
    # the README form: the flags in front of the model
    _child(tmp_path, [{"main": ["--bed_rmout", "--bed_gzip", "--bed_dir", str(a), "--bed_min_score", str(low), "--rmout_repeats", "4,3,2,1",
                                "--rmout_join", str(JOIN)] + FLAGS + [MODEL, paths["one"], paths["many"], "--output", str(tmp_path / "a.tsv")]},
                      {"main": FLAGS + ["predict", MODEL, paths["many"], "--output", str(tmp_path / "b.tsv"), "--bed_dir", str(b), "--bed_rmout",
                                        "--bed_names", ",".join(names)]},
                      {"main": FLAGS + ["predict", MODEL, paths["one"], paths["many"], "--output", str(tmp_path / "none.tsv")]}])
    assert _read(tmp_path / "a.tsv") == _read(tmp_path / "none.tsv")                   # the TSV is not filtered
    for key in ("one", "many"):
        want, lines, ids = _state(composed[key], low, rmout.pairs_of_repeats((4, 3, 2, 1)), JOIN)
        assert _inflate(_read(a / (key + ".fa.out.gz"))) == want
        if key == "many":
            assert 0 < ids <= lines < n_all
            back = [parse_rm_number(ln) for ln in want.split(b"\n")[3:-1]]
            assert set(back) <= {1, 2, 3, 4} and len(set(back)) > 1
    want, _l, _i = _state(composed["many"], 0, rmout.pairs_of_names([nm.encode() for nm in names]))
    assert _read(b / "many.fa.out") == want
    got = {(ln.split()[9], ln.split()[10]) for ln in want.split(b"\n")[3:-1]}
    assert got and got <= {tuple(nm.encode().split(b"#")) for nm in names}


def parse_rm_number(line: bytes) -> int:
    from deepgrp_amd._scripts import parse_rm
    return parse_rm.parse_line(line.decode()).typ


def test_other_inputs_and_paths(tmp_path, inputs):
    """A record without a base, .2bit and stdin inputs; -vv (the staged path), -m and --fast run through."""
    import twobit_corpus as tbc
    paths, composed, mix_recs = inputs
    want, lines, _ids = _state(composed["mix"])
    assert lines > 3 and b"none" not in want
    recs2 = []
    for header, s in mix_recs:
        if not s:
            continue
        idx = np.frombuffer(s.translate(bytes.maketrans(b"ACGTN", bytes([0, 1, 2, 3, 4]))), np.uint8)
        codes = np.array([2, 1, 3, 0, 0], np.uint8)[idx]                              # T=0 C=1 A=2 G=3; any two bits under an N block
        edge = np.flatnonzero(np.diff(np.concatenate(([0], (idx == 4).astype(np.int8), [0]))))
        recs2.append(tbc.Rec(header.split()[0], codes, [(int(a), int(b - a)) for a, b in zip(edge[::2], edge[1::2])], [], [0, 0, 0]))
    twobit = tmp_path / "mix.2bit"
    twobit.write_bytes(tbc.write(recs2))
    bgzf = tmp_path / "mix.fa.gz"
    bgzf.write_bytes(gz.bgzf_compress(_read(paths["mix"])))
    out = {k: tmp_path / k for k in ("files", "stdin", "vv", "m", "fast")}
    tsv = lambda k: ["--output", str(tmp_path / (k + ".tsv"))]
    rm = lambda k: ["--bed_dir", str(out[k]), "--bed_rmout"]
    jobs = [{"main": FLAGS + ["predict", MODEL, paths["mix"], str(bgzf), str(twobit)] + tsv("files") + rm("files")},
            {"main": FLAGS + ["predict", MODEL, "-"] + tsv("stdin") + rm("stdin") + ["--bed_gzip"]},
            {"main": ["-vv"] + FLAGS + ["predict", MODEL, paths["mix"]] + tsv("vv") + rm("vv")},
            {"main": FLAGS + ["predict", MODEL, paths["mix"], "-m"] + tsv("m") + rm("m")},
            {"main": FLAGS + ["predict", MODEL, paths["mix"], "--fast"] + tsv("fast") + rm("fast")}]
    _child(tmp_path, jobs, stdin=_read(paths["mix"]))
    assert sorted(os.listdir(out["files"])) == ["mix.2bit.out", "mix.fa.gz.out", "mix.fa.out"]
    assert _read(out["files"] / "mix.fa.out") == want == _read(out["files"] / "mix.fa.gz.out")
    # the .2bit record ends where its last base does, N or not: only `(left)` may differ from the FASTA's listing
    strip = lambda text: [ln.split()[:7] + ln.split()[8:] for ln in text.split(b"\n")[3:-1]]
    assert strip(_read(out["files"] / "mix.2bit.out")) == strip(want)
    assert os.listdir(out["stdin"]) == ["stdin.out.gz"] and _inflate(_read(out["stdin"] / "stdin.out.gz")) == want
    assert _read(out["vv"] / "mix.fa.out") == want
    for k in ("m", "fast"):                                                           # other rows, the same file format: every line reads back
        text = _read(out[k] / "mix.fa.out")
        rows = [ln.split(b"\t") for ln in _read(tmp_path / (k + ".tsv")).split(b"\n")[:-1]]
        cols = [ln.split() for ln in text.split(b"\n")[3:-1]]
        assert text.startswith(rmout.HEADER) and len(cols) == len(rows) > 0
        assert [(int(r[2]) + 1, int(r[3]), int(r[4])) for r in rows] == [(int(c[5]), int(c[6]), parse_rm_number(b" ".join(c))) for c in cols]


def test_an_all_n_record_and_an_unwritable_name(tmp_path, inputs):
    """The all-N record raises as it does without the flag: the finished input has its file, the other one nothing.  A record name
    with a DEL byte: one warning that names file and record, no `.out` for that input, the other input's file present."""
    paths, composed, mix_recs = inputs
    bad = tmp_path / "bad.fa"
    bad.write_bytes(_fasta([mix_recs[0], (b"allN", b"N" * 40), mix_recs[2]]))
    odd = tmp_path / "odd.fa"
    odd.write_bytes(_fasta([mix_recs[0], (b"od\x7fd name", mix_recs[3][1])]))
    d, e = tmp_path / "out", tmp_path / "odd"
    _child(tmp_path, [{"main": FLAGS + ["predict", MODEL, paths["mix"], str(bad), "--output", str(tmp_path / "o.tsv"), "--bed_dir", str(d),
                                        "--bed_rmout", "--bed_gzip"]}], fails="negative dimensions")
    assert os.listdir(d) == ["mix.fa.out.gz"] and _inflate(_read(d / "mix.fa.out.gz")) == _state(composed["mix"])[0]
    err = _child(tmp_path, [{"main": FLAGS + ["predict", MODEL, str(odd), paths["mix"], "--output", str(tmp_path / "p.tsv"), "--bed_dir", str(e),
                                              "--bed_rmout"]}])
    assert os.listdir(e) == ["mix.fa.out"] and _read(e / "mix.fa.out") == _state(composed["mix"])[0]
    said = [ln for ln in err.split("\n") if "no RepeatMasker listing is written (--bed_rmout)" in ln]
    assert len(said) == 1 and str(odd) in said[0] and "od\\x7fd" in said[0]
