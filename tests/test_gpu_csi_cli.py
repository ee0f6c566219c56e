"""predict --index_format csi end to end, the runs in one child process (tests/gff_cli_child.py): with --track_gzip --track_index and
with --bed_gzip --bed_index, for BED and for GFF3, every index is `<file>.gz.csi` and no `.tbi`, it inflates to
tabix.index_file's payload tabix.csi_reference_index of its `.gz`, tabix.csi_query finds what a scan of the lines finds, the `.gz`
and the TSV are the bytes of the run without the flag, and an index of the other format planted beforehand is gone."""
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

from deepgrp_amd import gff, gz, tabix  # noqa: E402

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
CHILD = os.path.join(ROOT, "tests", "gff_cli_child.py")
STALE = b"an index of an earlier run"


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


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Five runs of one three-record input in one child process -> the directory."""
    d = tmp_path_factory.mktemp("csi_cli")
    rng = np.random.default_rng(41)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    recs = [(b"m1 a", seq(1500)), (b"m2", b"NN" + seq(900) + b"N"), (b"m3", seq(2500))]
    fa = d / "in.fa"
    fa.write_bytes(b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs))
    for sub, stale in (("csi", ["in.fa.class1.bedGraph.gz.tbi", "in.fa.bed.gz.tbi"]), ("gcsi", ["in.fa.gff3.gz.tbi"]), ("tbi", ["in.fa.bed.gz.csi"])):
        os.makedirs(d / sub)
        for f in stale:
            (d / sub / f).write_bytes(STALE)
    base = FLAGS + ["predict", MODEL, str(fa)]
    out = lambda k: ["--output", str(d / (k + ".tsv"))]
    both = lambda k: ["--track_dir", str(d / k), "--track_gzip", "--bed_dir", str(d / k), "--bed_gzip"]
    jobs = [{"main": base + out("plain") + both("plain")},
            {"main": base + out("csi") + both("csi") + ["--track_index", "--bed_index", "--index_format", "csi"]},
            {"main": base + out("gplain") + ["--bed_dir", str(d / "gplain"), "--bed_gzip", "--bed_gff3"]},
            {"main": ["--index_format", "csi", "--bed_index", "--bed_gff3", "--bed_gzip", "--bed_dir", str(d / "gcsi")] + FLAGS
                     + [MODEL, str(fa)] + out("gcsi")},                                               # the README form
            {"main": base + out("tbi") + ["--bed_dir", str(d / "tbi"), "--bed_gzip", "--bed_index", "--index_format", "tbi"]}]
    spec = d / "jobs.json"
    spec.write_text(json.dumps(jobs))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, CHILD, str(spec)], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    assert "no tabix index" not in r.stderr.decode("utf-8", "replace")
    return d


def _check(data, csi, preset, names):
    """The `.csi` is the reference index of `data`; queries agree with a scan -> lines found"""
    assert gz.walk_members(csi).kind == "bgzf" and csi.endswith(gz.BGZF_EOF)
    pl = _inflate(csi)
    assert pl == tabix.csi_reference_index(data, preset) and tabix.index_file(pl) == csi
    ix = tabix.read_csi(pl)
    assert ix["depth"] == 6 and ix["preset"] == preset
    one_based = preset != tabix.PRESET_BED
    lines = [ln.split(b"\t") for ln in _inflate(data).split(b"\n")[:-1] if not ln.startswith(b"#")]
    assert ix["names"] == list(dict.fromkeys(f[0] for f in lines)) and set(ix["names"]) <= set(names)
    cols = (0, 3, 4) if one_based else (0, 1, 2)
    found = 0
    rng = np.random.default_rng(len(lines))
    regions = [(nm, 0, 1 << 32) for nm in names] + [(nm, 0, 1) for nm in names] + [(b"m3", 2499, 2500), (b"m3", 2500, 2600), (b"none", 0, 100)]
    for _ in range(40):
        beg = int(rng.integers(0, 2600))
        regions.append((names[int(rng.integers(0, len(names)))], beg, beg + int(rng.choice([1, 10, 300]))))
    for nm, beg, end in regions:
        want = [b"\t".join(f) for f in lines if f[cols[0]] == nm and int(f[cols[1]]) - one_based < end and int(f[cols[2]]) > beg]
        assert tabix.csi_query(ix, data, nm, beg, end) == want, (nm, beg, end)
        found += len(want)
    return found


def test_tracks(runs):
    assert _read(runs / "csi.tsv") == _read(runs / "plain.tsv") != b""
    gzs = [f"in.fa.class{c}.bedGraph.gz" for c in (1, 2, 3, 4)]
    have = sorted(f for f in os.listdir(runs / "csi") if "bedGraph" in f)
    assert have == sorted(gzs + [n + ".csi" for n in gzs])              # no .tbi: the planted one is gone
    found = 0
    for n in gzs:
        data = _read(runs / "csi" / n)
        assert data == _read(runs / "plain" / n)
        found += _check(data, _read(runs / "csi" / (n + ".csi")), tabix.PRESET_BED, [b"m1", b"m2", b"m3"])
    assert found > 0
    assert not any(f.endswith(".csi") or f.endswith(".tbi") for f in os.listdir(runs / "plain"))


def test_bed(runs):
    have = sorted(f for f in os.listdir(runs / "csi") if f.startswith("in.fa.bed."))
    assert have == ["in.fa.bed.gz", "in.fa.bed.gz.csi"]
    data = _read(runs / "csi" / "in.fa.bed.gz")
    assert data == _read(runs / "plain" / "in.fa.bed.gz") and _inflate(data).count(b"\n") > 0
    assert _check(data, _read(runs / "csi" / "in.fa.bed.gz.csi"), tabix.PRESET_BED, [b"m1", b"m2", b"m3"]) > 0


def test_gff3(runs):
    assert _read(runs / "gcsi.tsv") == _read(runs / "gplain.tsv") == _read(runs / "plain.tsv")
    assert sorted(os.listdir(runs / "gcsi")) == ["in.fa.gff3.gz", "in.fa.gff3.gz.csi"]
    data = _read(runs / "gcsi" / "in.fa.gff3.gz")
    assert data == _read(runs / "gplain" / "in.fa.gff3.gz") and _inflate(data).startswith(gff.HEADER)
    assert _check(data, _read(runs / "gcsi" / "in.fa.gff3.gz.csi"), gff.PRESET, [b"m1", b"m2", b"m3"]) > 0


def test_the_default_format_removes_a_stale_csi(runs):
    assert sorted(os.listdir(runs / "tbi")) == ["in.fa.bed.gz", "in.fa.bed.gz.tbi"]
    data = _read(runs / "tbi" / "in.fa.bed.gz")
    assert data == _read(runs / "plain" / "in.fa.bed.gz")
    assert _inflate(_read(runs / "tbi" / "in.fa.bed.gz.tbi")) == tabix.reference_index(data)
