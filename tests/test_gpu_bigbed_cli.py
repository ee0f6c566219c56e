"""predict --bed_dir --bed_bigbed end to end, each run in a child process: on a file of one long record (the record path) and on a
file of a few hundred short records (the batch path), at --gzip_level 0 and 1 and once through the staged path of -vv, the items of
the `.bb`, read by the independent reader and printed as lines, are the bytes of the `.bed` of a run without the flag -- under
--bed_min_score as well --, the reader's check_all passes, R-tree queries find what a scan finds, the TSV is the same with and
without the flag, and an input with two records of one name gets one warning and no `.bb`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bigbed_reader import BigBed
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
CHILD = "import json, sys; from deepgrp_amd.__main__ import main; [main(a) for a in json.loads(sys.argv[1])]"


def _fasta(recs):
    return b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bigbed_in")
    rng = np.random.default_rng(41)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    one = d / "one.fa"
    one.write_bytes(_fasta([(b"long one record", b"NNN" + seq(300_000))]))             # above runner.SMALL_RECORD: on its own
    many = d / "many.fa"
    recs = [(b"ctg%d some words" % i, seq(int(rng.integers(60, 900)))) for i in range(300)]
    many.write_bytes(_fasta(recs))
    dup = d / "dup.fa"
    dup.write_bytes(_fasta([(b"a 1", seq(2000)), (b"b", seq(1500)), (b"a 2", seq(1800))]))
    return str(one), str(many), str(dup)


def _child(argvs):
    """The commands one after the other in ONE child process -> its stderr."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(argvs)], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    return r.stderr.decode("utf-8", "replace")


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _check(bb_path, bed_path, regions, nchrom):
    """The `.bb` against the `.bed`: lines, invariants, queries."""
    r = BigBed(_read(bb_path))
    text = _read(bed_path)
    items, _zooms = r.check_all()
    assert r.lines() == text and len(items) == text.count(b"\n")
    assert len(r.chroms) == nchrom and (r.field_count, r.defined_fields) == (9, 6)
    found = 0
    for name, beg, end in regions:
        cid = r.find_chrom(name)[0]
        scan = [it for it in items if it[0] == cid and it[1] < end and it[2] > beg]
        assert r.query(cid, beg, end) == scan, (name, beg, end)
        found += len(scan)
    return r, found


ONE_REGIONS = [(b"long", 0, 1 << 31), (b"long", 16_000, 17_000), (b"long", 150_000, 150_500), (b"long", 299_000, 400_000), (b"long", 3, 4)]
MANY_REGIONS = [(b"ctg0", 0, 1000), (b"ctg16", 0, 1000), (b"ctg16", 100, 101), (b"ctg150", 200, 400), (b"ctg299", 0, 1 << 31)]


@pytest.mark.parametrize("level,vv", [(0, False), (1, False), (1, True)])
def test_bigbed_items_are_the_bed_lines(tmp_path, inputs, level, vv):
    one, many, _dup = inputs
    base = FLAGS + ["predict", MODEL, one, many]
    pre = ["-vv"] if vv else []
    cmds = []
    for low in (None, 600):
        tail = [] if low is None else ["--bed_min_score", str(low)]
        cmds.append(base + tail + ["--output", str(tmp_path / f"plain{low}.tsv"), "--bed_dir", str(tmp_path / f"plain{low}")])
        cmds.append(pre + base + tail + ["--output", str(tmp_path / f"big{low}.tsv"), "--bed_dir", str(tmp_path / f"big{low}"), "--bed_bigbed",
                                         "--gzip_level", str(level)])
    _child(cmds)
    for low in (None, 600):
        plain, big = tmp_path / f"plain{low}", tmp_path / f"big{low}"
        assert _read(tmp_path / f"plain{low}.tsv") == _read(tmp_path / f"big{low}.tsv") == _read(tmp_path / "plainNone.tsv")
        assert sorted(os.listdir(plain)) == ["many.fa.bed", "one.fa.bed"] and sorted(os.listdir(big)) == ["many.fa.bb", "one.fa.bb"]
        r, found = _check(big / "one.fa.bb", plain / "one.fa.bed", ONE_REGIONS, 1)
        assert r.chroms == [(b"long", 0, 300_003)]
        r, found_many = _check(big / "many.fa.bb", plain / "many.fa.bed", MANY_REGIONS, 300)
        assert r.find_chrom(b"ctg100")[0] == 100 and r.find_chrom(b"ctg299")[0] == 299
        if low is None:
            assert found > 0 and found_many > 0 and _read(plain / "one.fa.bed").count(b"\n") > 50 and r.nzoom == 0
            assert BigBed(_read(big / "one.fa.bb")).nzoom == 5             # 1024 * 4^4 < 300003 <= 1024 * 4^5


def test_two_records_of_one_name_leave_no_bigbed(tmp_path, inputs):
    _one, many, dup = inputs
    plain, big = tmp_path / "plain", tmp_path / "big"
    os.makedirs(big)
    (big / "dup.fa.bb").write_bytes(b"left by an earlier run")
    err = _child([FLAGS + ["predict", MODEL, dup, many, "--output", str(tmp_path / "plain.tsv"), "--bed_dir", str(plain)],
                  FLAGS + ["predict", MODEL, dup, many, "--output", str(tmp_path / "big.tsv"), "--bed_dir", str(big), "--bed_bigbed"]])
    assert _read(tmp_path / "plain.tsv") == _read(tmp_path / "big.tsv")
    assert sorted(os.listdir(big)) == ["many.fa.bb"]                     # no `.bb`, no temporary file, and the stale one is gone
    assert BigBed(_read(big / "many.fa.bb")).lines() == _read(plain / "many.fa.bed")
    warnings = [ln for ln in err.split("\n") if "no bigBed file is written (--bed_bigbed)" in ln]
    assert len(warnings) == 1 and "dup.fa" in warnings[0] and "two records have the name 'a'" in warnings[0]
