"""predict --bed_dir --bed_gzip --bed_index end to end, each run in a child process: on a file of one long record (the record path)
and on a file of a few hundred short records (the batch path), at --gzip_level 0 and 1, the inflated `.bed.gz` is the `.bed` of a run
without --bed_gzip, the `.tbi` is tabix.reference_index of the `.bed.gz`, tabix.query finds the lines a scan finds, the TSV is the
same with and without the flags, --bed_min_score filters both forms alike, and a record name that comes back after another name
leaves the `.bed.gz`, one warning and no `.tbi`."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from deepgrp_amd import gz, tabix  # noqa: E402

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
CHILD = "import json, sys; from deepgrp_amd.__main__ import main; [main(a) for a in json.loads(sys.argv[1])]"


def _fasta(recs):
    return b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bedgz_in")
    rng = np.random.default_rng(41)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    one = d / "one.fa"
    one.write_bytes(_fasta([(b"long one record", b"NNN" + seq(300_000))]))             # above runner.SMALL_RECORD: on its own
    many = d / "many.fa"
    recs = [(b"ctg%d some words" % i, seq(int(rng.integers(60, 900)))) for i in range(300)]
    recs[17] = (b"ctg16 the name of its predecessor", recs[17][1])                    # consecutive records of one name: one sequence
    many.write_bytes(_fasta(recs))
    back = d / "back.fa"
    back.write_bytes(_fasta([(b"a 1", seq(2000)), (b"b", seq(1500)), (b"a 2", seq(1800))]))
    return str(one), str(many), str(back)


def _child(argvs):
    """The commands one after the other in ONE child process -> its stderr."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(argvs)], cwd=ROOT, env=env, capture_output=True, timeout=300)
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


def _check_index(data, tbi, regions):
    payload = _inflate(tbi)
    assert payload == tabix.reference_index(data)
    ix = tabix.read_index(payload)
    lines = [ln.split(b"\t") for ln in _inflate(data).split(b"\n")[:-1]]
    found = 0
    for name, beg, end in regions:
        scan = [b"\t".join(f) for f in lines if f[0] == name and int(f[1]) < end and int(f[2]) > beg]
        assert tabix.query(ix, data, name, beg, end) == scan, (name, beg, end)
        found += len(scan)
    assert found > 0
    return ix


@pytest.mark.parametrize("level", [0, 1])
def test_gzip_and_index_at_both_levels(tmp_path, inputs, level):
    one, many, _back = inputs
    base = FLAGS + ["predict", MODEL, one, many]
    plain, packed = tmp_path / "plain", tmp_path / "packed"
    _child([base + ["--output", str(tmp_path / "plain.tsv"), "--bed_dir", str(plain)],
            base + ["--output", str(tmp_path / "packed.tsv"), "--bed_dir", str(packed), "--bed_gzip", "--bed_index", "--gzip_level", str(level)]])
    assert _read(tmp_path / "plain.tsv") == _read(tmp_path / "packed.tsv")
    assert sorted(os.listdir(plain)) == ["many.fa.bed", "one.fa.bed"]
    assert sorted(os.listdir(packed)) == ["many.fa.bed.gz", "many.fa.bed.gz.tbi", "one.fa.bed.gz", "one.fa.bed.gz.tbi"]
    for stem in ("one.fa", "many.fa"):
        text, data = _read(plain / (stem + ".bed")), _read(packed / (stem + ".bed.gz"))
        assert text.count(b"\n") > 50 and data.endswith(gz.BGZF_EOF)
        assert _inflate(data) == text
    ix = _check_index(_read(packed / "one.fa.bed.gz"), _read(packed / "one.fa.bed.gz.tbi"),
                      [(b"long", 0, 1 << 29), (b"long", 16_000, 17_000), (b"long", 150_000, 150_500), (b"long", 299_000, 400_000), (b"long", 3, 4)])
    assert ix["names"] == [b"long"] and len(ix["linear"][0]) > 15
    ix = _check_index(_read(packed / "many.fa.bed.gz"), _read(packed / "many.fa.bed.gz.tbi"),
                      [(b"ctg0", 0, 1000), (b"ctg16", 0, 1000), (b"ctg16", 100, 101), (b"ctg150", 200, 400), (b"ctg299", 0, 1 << 29)])
    assert 50 < len(ix["names"]) <= 299 and b"ctg17" not in ix["names"]


def test_min_score_filters_both_forms_alike(tmp_path, inputs):
    """--bed_min_score 600, and the median of the scores this model gives (on random sequence few rows reach 600, so the second
    threshold is the one that is sure to keep some lines and drop others)."""
    one, many, _back = inputs
    full = tmp_path / "full"
    _child([FLAGS + ["predict", MODEL, one, many, "--output", str(tmp_path / "full.tsv"), "--bed_dir", str(full)]])
    every = {stem: _read(full / (stem + ".bed")).split(b"\n")[:-1] for stem in ("one.fa", "many.fa")}
    distinct = sorted({int(ln.split(b"\t")[4]) for lines in every.values() for ln in lines})
    assert len(distinct) > 1, "every row has the same score: the filter cannot be told from no filter"
    lows = [600, distinct[len(distinct) // 2]]
    cmds = []
    for low in lows:
        cmds.append(FLAGS + ["predict", MODEL, one, many, "--bed_min_score", str(low), "--output", str(tmp_path / f"plain{low}.tsv"), "--bed_dir",
                             str(tmp_path / f"plain{low}")])
        # the README form: the flags in front of the model
        cmds.append(["--bed_gzip", "--bed_index", "--bed_dir", str(tmp_path / f"packed{low}"), "--bed_min_score", str(low)] + FLAGS
                    + [MODEL, one, many, "--output", str(tmp_path / f"packed{low}.tsv")])
    _child(cmds)
    for low in lows:
        assert _read(tmp_path / f"plain{low}.tsv") == _read(tmp_path / f"packed{low}.tsv") == _read(tmp_path / "full.tsv")     # the TSV is not filtered
        for stem in ("one.fa", "many.fa"):
            text, data = _read(tmp_path / f"plain{low}" / (stem + ".bed")), _read(tmp_path / f"packed{low}" / (stem + ".bed.gz"))
            kept = [ln for ln in every[stem] if int(ln.split(b"\t")[4]) >= low]
            assert text == b"".join(ln + b"\n" for ln in kept) and _inflate(data) == text and data.endswith(gz.BGZF_EOF)
            assert _inflate(_read(tmp_path / f"packed{low}" / (stem + ".bed.gz.tbi"))) == tabix.reference_index(data)
            if low != 600:
                assert 0 < len(kept) < len(every[stem])


def test_a_name_that_comes_back_leaves_no_index(tmp_path, inputs):
    _one, many, back = inputs
    plain, packed = tmp_path / "plain", tmp_path / "packed"
    os.makedirs(packed)
    (packed / "back.fa.bed.gz.tbi").write_bytes(b"left by an earlier run")
    err = _child([FLAGS + ["predict", MODEL, back, "--output", str(tmp_path / "plain.tsv"), "--bed_dir", str(plain)],
                  FLAGS + ["predict", MODEL, back, many, "--output", str(tmp_path / "packed.tsv"), "--bed_dir", str(packed), "--bed_gzip",
                           "--bed_index"]])
    assert sorted(os.listdir(packed)) == ["back.fa.bed.gz", "many.fa.bed.gz", "many.fa.bed.gz.tbi"]
    text = _read(plain / "back.fa.bed")
    assert _inflate(_read(packed / "back.fa.bed.gz")) == text
    assert text.startswith(b"a\t") and {ln.split(b"\t")[0] for ln in text.split(b"\n")[:-1]} <= {b"a", b"b"}
    warnings = [ln for ln in err.split("\n") if "no tabix index is written (--bed_index)" in ln]
    assert len(warnings) == 1 and "back.fa" in warnings[0] and "reappears" in warnings[0]
