"""predict --bed_dir --bed_gff3 end to end, each run in a child process (tests/gff_cli_child.py): on a file of one long record (the
record path) and on a file of 300 short records (the batch path), at --gzip_level 0 and 1, the plain `.gff3` is the inflated
`.gff3.gz` and is gff.HEADER + gff.reference_lines composed from the run's own rows and scores; there is one line per TSV row with
start+1 and end; the ID ordinals run 1..lines across records and batches; the `.tbi` is gff.reference_index of the file and
gff.query finds what a scan finds; the TSV is the bytes of a run without the flag and --bed_dir alone writes today's `.bed`;
--bed_min_score and --bed_names take effect; an all-N record, a record without a base, BGZF, .2bit and stdin inputs; -vv, -m
and --fast."""
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

from deepgrp_amd import bed, gff, gz  # noqa: E402

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
KW = {"b": 7, "s": 4, "x": 5, "l": 3}
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
CHILD = os.path.join(ROOT, "tests", "gff_cli_child.py")


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


def _load(path):
    with open(path, "rb") as fh:
        return pickle.load(fh)


def _state(composed, min_score=0, class_names=None):
    """The GFF3 file of a composition: the header, then every record's lines with the ordinals running on."""
    out, lines = [gff.HEADER], 0
    for name, rows, scores in composed["records"]:
        text, n = gff.reference_lines([name], False, rows, scores, min_score, class_names, lines)
        out.append(text)
        lines += n
    return b"".join(out), lines


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The inputs and, from one child process, their compositions."""
    d = tmp_path_factory.mktemp("gff_in")
    rng = np.random.default_rng(41)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    one = d / "one.fa"
    one.write_bytes(_fasta([(b"long one record", b"NNN" + seq(300_000))]))             # above runner.SMALL_RECORD: on its own
    many = d / "many.fa"
    recs = [(b"ctg%d some words" % i, seq(int(rng.integers(60, 900)))) for i in range(300)]
    recs[17] = (b"ctg16 the name of its predecessor", recs[17][1])                    # consecutive records of one name: one sequence
    recs[40] = (b"odd;name=1 x", recs[40][1])                                         # a name that column 1 escapes
    many.write_bytes(_fasta(recs))
    mix = d / "mix.fa"                                                                # a record without a base between records with rows
    mix_recs = [(b"m1 a", seq(1500)), (b"none no sequence at all", b""), (b"m2", b"NN" + seq(900) + b"N"), (b"m3", seq(2500))]
    mix.write_bytes(_fasta(mix_recs))
    paths = {"one": str(one), "many": str(many), "mix": str(mix)}
    jobs = [{"compose": dict(model_file=MODEL, path=paths[k], out=str(d / (k + ".pkl")), flags=KW)} for k in paths]
    jobs += [{"compose": dict(model_file=MODEL, path=paths["mix"], out=str(d / "mix_m.pkl"), flags=KW, use_mss=False)},
             {"compose": dict(model_file=MODEL, path=paths["mix"], out=str(d / "mix_fast.pkl"), flags=KW, fast=True)}]
    _child(d, jobs)
    composed = {k: _load(d / (k + ".pkl")) for k in ("one", "many", "mix", "mix_m", "mix_fast")}
    return paths, composed, mix_recs


def _check_index(data, tbi, regions):
    payload = _inflate(tbi)
    assert payload == gff.reference_index(data)
    ix = gff.read_index(payload)
    lines = [ln.split(b"\t") for ln in _inflate(data).split(b"\n")[1:-1]]
    found = 0
    for name, beg, end in regions:
        scan = [b"\t".join(f) for f in lines if f[0] == name and int(f[3]) - 1 < end and int(f[4]) > beg]
        assert gff.query(ix, data, name, beg, end) == scan, (name, beg, end)
        found += len(scan)
    assert found > 0
    return ix


@pytest.mark.parametrize("level", [0, 1])
def test_plain_gzip_and_index_at_both_levels(tmp_path, inputs, level):
    paths, composed, _mix = inputs
    base = FLAGS + ["predict", MODEL, paths["one"], paths["many"]]
    today, plain, packed = tmp_path / "today", tmp_path / "plain", tmp_path / "packed"
    _child(tmp_path, [{"main": base + ["--output", str(tmp_path / "none.tsv")]},
                      {"main": base + ["--output", str(tmp_path / "today.tsv"), "--bed_dir", str(today)]},
                      {"main": base + ["--output", str(tmp_path / "plain.tsv"), "--bed_dir", str(plain), "--bed_gff3"]},
                      {"main": base + ["--output", str(tmp_path / "packed.tsv"), "--bed_dir", str(packed), "--bed_gff3", "--bed_gzip", "--bed_index",
                                       "--gzip_level", str(level)]}])
    tsv = _read(tmp_path / "none.tsv")
    assert tsv == _read(tmp_path / "today.tsv") == _read(tmp_path / "plain.tsv") == _read(tmp_path / "packed.tsv")
    assert sorted(os.listdir(today)) == ["many.fa.bed", "one.fa.bed"]
    assert sorted(os.listdir(plain)) == ["many.fa.gff3", "one.fa.gff3"]
    assert sorted(os.listdir(packed)) == ["many.fa.gff3.gz", "many.fa.gff3.gz.tbi", "one.fa.gff3.gz", "one.fa.gff3.gz.tbi"]
    for key in ("one", "many"):
        stem = key + ".fa"
        want, lines = _state(composed[key])
        text, data = _read(plain / (stem + ".gff3")), _read(packed / (stem + ".gff3.gz"))
        assert lines > 50 and text == want and data.endswith(gz.BGZF_EOF) and _inflate(data) == text
        assert data.startswith(gff.header_member(level))
        # --bed_dir alone: today's bytes
        assert _read(today / (stem + ".bed")) == b"".join(bed.reference_lines([nm], False, r, s, 0) for nm, r, s in composed[key]["records"])
        # one line per TSV row of this input, with start+1 and end; the ordinals run through the file
        rows = [ln.split("\t") for ln in tsv.decode().split("\n")[:-1] if ln.split("\t")[0] == paths[key]]
        cols = [ln.split(b"\t") for ln in text.split(b"\n")[1:-1]]
        assert len(rows) == len(cols) == lines
        assert [(int(r[2]) + 1, int(r[3])) for r in rows] == [(int(c[3]), int(c[4])) for c in cols]
        assert [c[8].split(b";")[0] for c in cols] == [b"ID=r%d" % j for j in range(1, lines + 1)]
        assert all(c[8].split(b";")[2] == b"label=" + r[4].encode() and c[8].split(b";")[1] == b"Name=class" + r[4].encode()
                   for r, c in zip(rows, cols))
    ix = _check_index(_read(packed / "one.fa.gff3.gz"), _read(packed / "one.fa.gff3.gz.tbi"),
                      [(b"long", 0, 1 << 29), (b"long", 16_000, 17_000), (b"long", 150_000, 150_500), (b"long", 299_000, 400_000), (b"long", 3, 4)])
    assert ix["names"] == [b"long"] and len(ix["linear"][0]) > 15
    ix = _check_index(_read(packed / "many.fa.gff3.gz"), _read(packed / "many.fa.gff3.gz.tbi"),
                      [(b"ctg0", 0, 1000), (b"ctg16", 0, 1000), (b"ctg16", 100, 101), (b"ctg150", 200, 400), (b"ctg299", 0, 1 << 29),
                       (b"odd%3Bname%3D1", 0, 1000)])
    assert 50 < len(ix["names"]) <= 299 and b"ctg17" not in ix["names"]


def test_min_score_and_names_take_effect(tmp_path, inputs):
    paths, composed, _mix = inputs
    classes = composed["many"]["classes"]
    names = [b"LTR/ERV1", b"a;b=c", b"SINE/Alu&x", b"x" * 255, b"E5", b"F6", b"G7"][:classes - 1]
    assert len(names) == classes - 1
    full, _n = _state(composed["many"])
    scores = sorted({int(ln.split(b";score=")[1].split(b";")[0]) for ln in full.split(b"\n")[1:-1]})
    assert len(scores) > 1, "every row has the same score: the filter cannot be told from no filter"
    low = scores[len(scores) // 2]
    out = tmp_path / "out"
    # the README form: the flags in front of the model
    _child(tmp_path, [{"main": ["--bed_gff3", "--bed_gzip", "--bed_index", "--bed_dir", str(out), "--bed_min_score", str(low), "--bed_names",
                                b",".join(names).decode()] + FLAGS + [MODEL, paths["one"], paths["many"], "--output", str(tmp_path / "o.tsv")]},
                      {"main": FLAGS + ["predict", MODEL, paths["one"], paths["many"], "--output", str(tmp_path / "none.tsv")]}])
    assert _read(tmp_path / "o.tsv") == _read(tmp_path / "none.tsv")                   # the TSV is not filtered
    for key in ("one", "many"):
        want, lines = _state(composed[key], low, names)
        data = _read(out / (key + ".fa.gff3.gz"))
        assert _inflate(data) == want and _inflate(_read(out / (key + ".fa.gff3.gz.tbi"))) == gff.reference_index(data)
        if key == "many":
            assert 0 < lines < _state(composed[key])[1]
            got = {ln.split(b";Name=")[1].split(b";")[0] for ln in want.split(b"\n")[1:-1]}
            assert got and got <= {gff.escape_value(nm) for nm in names} and not any(g.startswith(b"class") for g in got)


def test_other_inputs_and_paths(tmp_path, inputs):
    """A record without a base, BGZF, .2bit and stdin inputs; -vv (the staged path), -m and --fast.  (A record without a name
    cannot come from a sequence file -- the readers drop a record without a header, as the reference does --: BedFiles' rule for it
    is tested on fake writes, tests/test_gff_host.py.)"""
    import twobit_corpus as tbc
    paths, composed, mix_recs = inputs
    want, lines = _state(composed["mix"])
    assert lines > 3 and b"none" not in want
    bgzf = tmp_path / "mix.fa.gz"
    bgzf.write_bytes(gz.bgzf_compress(_read(paths["mix"])))
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
    out = {k: tmp_path / k for k in ("files", "stdin", "vv", "vvgz", "m", "fast")}
    tsv = lambda k: ["--output", str(tmp_path / (k + ".tsv"))]
    gff3 = lambda k: ["--bed_dir", str(out[k]), "--bed_gff3"]
    jobs = [{"main": FLAGS + ["predict", MODEL, paths["mix"], str(bgzf), str(twobit)] + tsv("files") + gff3("files")},
            {"main": FLAGS + ["predict", MODEL, "-"] + tsv("stdin") + gff3("stdin") + ["--bed_gzip"]},
            {"main": ["-vv"] + FLAGS + ["predict", MODEL, paths["mix"]] + tsv("vv") + gff3("vv")},
            {"main": ["-vv"] + FLAGS + ["predict", MODEL, paths["mix"]] + tsv("vvgz") + gff3("vvgz") + ["--bed_gzip", "--bed_index"]},
            {"main": FLAGS + ["predict", MODEL, paths["mix"], "-m"] + tsv("m") + gff3("m")},
            {"main": FLAGS + ["predict", MODEL, paths["mix"], "--fast"] + tsv("fast") + gff3("fast")}]
    _child(tmp_path, jobs, stdin=_read(paths["mix"]))
    assert sorted(os.listdir(out["files"])) == ["mix.2bit.gff3", "mix.fa.gff3", "mix.fa.gz.gff3"]
    for f in os.listdir(out["files"]):
        assert _read(out["files"] / f) == want, f
    assert os.listdir(out["stdin"]) == ["stdin.gff3.gz"] and _inflate(_read(out["stdin"] / "stdin.gff3.gz")) == want
    assert _read(out["vv"] / "mix.fa.gff3") == want
    data = _read(out["vvgz"] / "mix.fa.gff3.gz")
    assert _inflate(data) == want and _inflate(_read(out["vvgz"] / "mix.fa.gff3.gz.tbi")) == gff.reference_index(data)
    assert gff.read_index(gff.reference_index(data))["names"] == [b"m1", b"m2", b"m3"]
    for k in ("m", "fast"):
        want_k, lines_k = _state(composed["mix_" + k])
        assert lines_k > 0 and _read(out[k] / "mix.fa.gff3") == want_k, k
    mine = b"".join(ln + b"\n" for ln in _read(tmp_path / "files.tsv").split(b"\n")[:-1] if ln.startswith(paths["mix"].encode() + b"\t"))
    assert _read(tmp_path / "vv.tsv") == _read(tmp_path / "vvgz.tsv") == mine and mine.count(b"\n") == lines


def test_an_all_n_record_leaves_no_file(tmp_path, inputs):
    """The record raises as it does without the flag: the finished input has its files, the other one nothing."""
    paths, composed, mix_recs = inputs
    bad = tmp_path / "bad.fa"
    bad.write_bytes(_fasta([mix_recs[0], (b"allN", b"N" * 40), mix_recs[2]]))
    d = tmp_path / "out"
    _child(tmp_path, [{"main": FLAGS + ["predict", MODEL, paths["mix"], str(bad), "--output", str(tmp_path / "o.tsv"), "--bed_dir", str(d),
                                        "--bed_gff3", "--bed_gzip", "--bed_index"]}], fails="negative dimensions")
    assert sorted(os.listdir(d)) == ["mix.fa.gff3.gz", "mix.fa.gff3.gz.tbi"]
    assert _inflate(_read(d / "mix.fa.gff3.gz")) == _state(composed["mix"])[0]
