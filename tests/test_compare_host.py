"""`compare` without a GPU: the sniffing of the three PREDICTED forms, the host statement of the TSV, the refusals that come before any
device work (in a child process, without a traceback), the two new symbols, and the numpy statement of the flattening rule."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from compare_cases import FOREIGN, FOREIGN_SPAN, SEG, boundary_profile, rows, table_text, tsv_text
from conftest import ROOT

OUT_LINE = "  463   1.3  0.6  1.7  chr1     10001   10468 (248945954) +  (TAACCC)n      Simple_repeat     1  471    (0)      1\n"
RMSK_LINE = "585\t463\t13\t6\t17\tchr1\t10000\t10468\t-248945954\t+\t(TAACCC)n\tSimple_repeat\tSimple_repeat\t1\t471\t0\t1\n"


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text if isinstance(text, bytes) else text.encode())
    return str(p)


# ---------------------------------------------------------------- sniffing
@pytest.mark.parametrize("text,want", [
    ("f.fa\t1\t100\t200\t1\n", "tsv"),                                   # also a table line: tsv is tried first
    ("genome.fa\tchr1 a header\twith a tab\t100\t200\t3\n\ngenome.fa\tchr1\t300\t400\t1\n", "tsv"),
    ("chr1\t100\t200\t1\n", "table"),                                    # four fields
    ("chr1 100 200 1 AluY SINE/Alu\n", "table"),
    ("# comment\nchr1\t100\t200\t1\tAluY\tSINE/Alu\n", "table"),          # the last three are not all digits
    ("f.fa\tchr1\t100\t200\t1\nchr1\t5\t9\t2\n", "table"),               # every sniffed line has to be a tsv line
    ("   SW   perc perc\nscore   div. del.\n\n" + OUT_LINE, "repeatmasker"),
    (RMSK_LINE, "repeatmasker"),
    ("", "table"),
])
def test_sniffing(tmp_path, text, want):
    from deepgrp_amd.compare import resolve_predicted_format, sniff_predicted
    p = _write(tmp_path, "p.txt", text)
    assert sniff_predicted(p) == want
    assert resolve_predicted_format(p, "auto") == want
    assert resolve_predicted_format(p, "table") == "table"
    with pytest.raises(ValueError):
        resolve_predicted_format(p, "bed")


def test_sniffing_gzip(tmp_path):
    import gzip

    from deepgrp_amd.compare import sniff_predicted
    p = tmp_path / "p.tsv.gz"
    with gzip.open(p, "wb") as fh:
        fh.write(b"genome.fa\tchr1\t100\t200\t1\n" * 10)
    assert sniff_predicted(str(p)) == "tsv"


# ---------------------------------------------------------------- the host statement of the TSV
def test_tsv_name_rule():
    from deepgrp_amd.compare import tsv_name
    assert tsv_name("genome.fa", "chr1 assembled by hand") == "chr1"
    assert tsv_name("genome.fa", "  chr4\tx") == "chr4"
    assert tsv_name("genome.fa", "") == ""
    assert tsv_name("data/run1/chrA.fa.gz.npz", "chrA.fa.gz") == "chrA"       # the file need not exist, unlike record_name's rule
    assert tsv_name("/abs/chrB.npz", "anything else") == "chrB"
    assert tsv_name("x.npz.fa", "h w") == "h"


def test_tsv_host_statement(tmp_path):
    from deepgrp_amd.compare import tsv_flat_host
    text = ("genome.fa\tchr1 with words\t10\t20\t1\r\n"
            "genome.fa\tchr1 with words\t30\t40\t2\n"
            "\n"
            "genome.fa\tchr3\twith\ttabs in it\t5\t6\t3\n"
            "d/chrA.fa.gz.npz\tchrA.fa.gz\t7\t9\t4\n"
            "other.fa\t\t1\t2\t1")
    flat = tsv_flat_host(_write(tmp_path, "p.tsv", text))
    assert flat.lines == 6 and flat.route == "host"
    assert flat.begin.tolist() == [10, 30, 5, 7, 1] and flat.end.tolist() == [20, 40, 6, 9, 2] and flat.number.tolist() == [1, 2, 3, 4, 1]
    assert flat.line.tolist() == [1, 2, 4, 5, 6]
    assert flat.run_first.tolist() == [0, 2, 3, 4, 5]
    assert flat.run_names == ["chr1", "chr3", "chrA", ""]
    assert flat.run_files == ["genome.fa", "genome.fa", "d/chrA.fa.gz.npz", "other.fa"]


@pytest.mark.parametrize("text,line,why", [
    ("f\th\t1\t2\t3\nf\th\t1\t2\n", 2, "expected file, header"),
    ("f\th\t1\tx\t3\n", 1, "end 'x' is not an integer"),
    ("f\th\t1\t2\t99999999999999999999\n", 1, "label '99999999999999999999' is not an integer"),
])
def test_tsv_host_statement_errors(tmp_path, text, line, why):
    from deepgrp_amd.compare import tsv_flat_host
    from deepgrp_amd.evaluation import AnnotationError
    p = _write(tmp_path, "p.tsv", text)
    with pytest.raises(AnnotationError) as e:
        tsv_flat_host(p)
    assert str(e.value).startswith(f"{p}:{line}: ") and why in str(e.value)


def test_read_predicted_tsv_on_the_host(tmp_path):
    from deepgrp_amd.compare import read_predicted
    from deepgrp_amd.evaluation import AnnotationError
    text = tsv_text(1)
    got = read_predicted(_write(tmp_path, "p.tsv", text), "auto", 5, device=False)
    assert got.format == "tsv" and got.route == "host" and got.rows_dropped == 0
    assert set(got) == {"chr1", "chr2", "chr3", "chr4", "chrA", "chrB", "", "stdin_rec"}
    assert got.rows_read == sum(len(v) for v in got.values()) == sum(1 for ln in text.split(b"\n") if ln.strip(b"\r"))
    for name, r in got.items():
        assert r.dtype == SEG and (np.diff(got.lines[name]) > 0).all()
    # a label outside 1..C-1 names file and line
    p = _write(tmp_path, "q.tsv", "f.fa\tchr1\t1\t2\t1\nf.fa\tchr1\t5\t9\t5\n")
    with pytest.raises(AnnotationError) as e:
        read_predicted(p, "tsv", 5, device=False)
    assert str(e.value).startswith(f"{p}:2: label 5 is not a class of 1..4") and "'f.fa\\tchr1\\t5\\t9\\t5'" in str(e.value)
    assert len(read_predicted(p, "tsv", 6, device=False)["chr1"]) == 2
    p = _write(tmp_path, "r.tsv", "f.fa\tchr1\t1\t2\t0\n")
    with pytest.raises(AnnotationError, match="r.tsv:1: label 0"):
        read_predicted(p, "tsv", 5, device=False)
    p = _write(tmp_path, "s.tsv", "f.fa\tchr1\t9\t2\t1\n")
    with pytest.raises(AnnotationError, match="s.tsv:1: end below begin"):
        read_predicted(p, "tsv", 5, device=False)


def test_two_files_one_name_is_refused(tmp_path):
    from deepgrp_amd.compare import read_predicted
    from deepgrp_amd.evaluation import AnnotationError
    p = _write(tmp_path, "p.tsv", "a.fa\tchr1 x\t1\t2\t1\nb.fa\tchr2\t1\t2\t1\nb.fa\tchr1 y\t5\t6\t1\n")
    with pytest.raises(AnnotationError) as e:
        read_predicted(p, "tsv", 5, device=False)
    assert "'chr1'" in str(e.value) and "'a.fa'" in str(e.value) and "'b.fa'" in str(e.value)
    # one file, the name in two runs: fine
    p = _write(tmp_path, "q.tsv", "a.fa\tchr1 x\t1\t2\t1\na.fa\tchr2\t1\t2\t1\na.fa\tchr1 y\t5\t6\t1\n")
    got = read_predicted(p, "tsv", 5, device=False)
    assert got["chr1"]["start"].tolist() == [1, 5] and got.lines["chr1"].tolist() == [1, 3]


def test_read_predicted_table_on_the_host_drops_and_counts(tmp_path):
    from deepgrp_amd.compare import read_predicted
    from deepgrp_amd.evaluation import AnnotationError
    p = _write(tmp_path, "t.bed", "# c\nchr1 1 5 1\nchr1 7 9 0\nchr2 1 2 7\nchr1 20 30 4 extra\n")
    got = read_predicted(p, "auto", 5, device=False)
    assert got.format == "table" and got.rows_read == 4 and got.rows_dropped == 2
    assert list(got) == ["chr1"] and got["chr1"]["label"].tolist() == [1, 4]
    p = _write(tmp_path, "u.bed", "chr1 1 5 1\nchr1 -7 9 1\n")
    with pytest.raises(AnnotationError, match="u.bed:2: negative begin"):
        read_predicted(p, "table", 5, device=False)
    with pytest.raises(ValueError, match="classes must lie in 2..64"):
        read_predicted(p, "table", 65, device=False)


def test_the_seeded_texts_meet_the_boundaries():
    for text in (table_text(0), tsv_text(0)):
        on_chunk, on_tile, straddle = boundary_profile(text)
        assert 95_000 < len(text) < 110_000 and on_chunk > 100 and on_tile >= 1 and straddle >= 1
        assert b"\r\n" in text and not text.endswith(b"\n")


# ---------------------------------------------------------------- refusals before any device work
def _cli(args, env_extra=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = ""        # no device: whatever reaches for one fails
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "deepgrp_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags,env,want", [
    (["--curves", "PFX"], None, r"--curves needs the probabilities"),
    (["--curve_elements"], None, r"--curve_elements needs the probabilities"),
    ([], {"WORLD_SIZE": "2"}, r"compare runs in one process"),
    (["--classes", "1"], None, r"--classes must lie in 2\.\.64, not 1"),
    (["--classes", "65"], None, r"--classes must lie in 2\.\.64, not 65"),
    (["--repeats", "1,5"], None, r"--repeats: 5 is not a repeat class of --classes 5 \(1\.\.4\)"),
    (["--classes", "3", "--repeats", "0"], None, r"--repeats: 0 is not a repeat class"),
    (["--min_overlap", "0"], None, r"--min_overlap must lie in \(0, 1\]"),
    (["--strata_div", "5"], None, r"--strata_div needs --strata"),
])
def test_cli_refusals_before_device_work(tmp_path, flags, env, want):
    # none of the three files exists: a refusal that came after reading one would not be the text looked for
    r = _cli(["compare", str(tmp_path / "p.tsv"), str(tmp_path / "a.bed"), str(tmp_path / "g.fa")] + flags, env)
    assert r.returncode != 0 and r.stdout == ""
    assert re.search(want, r.stderr), r.stderr
    assert "Traceback" not in r.stderr


def test_cli_refuses_predict_outputs(tmp_path):
    r = _cli(["--bed_dir", str(tmp_path), "compare", "p.tsv", "a.bed", "g.fa"])
    assert r.returncode != 0 and "belongs to predict" in r.stderr and "Traceback" not in r.stderr


# ---------------------------------------------------------------- the symbols
def test_the_two_symbols_are_exported_and_declared():
    from deepgrp_amd._lib import exported_symbols
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for sym in ("dgrp_rows_parse", "dgrp_rows_parse_workspace_bytes"):
        assert sym in exported_symbols()
        assert re.search(r"^int(64_t)? %s\(" % sym, header, re.M)
    assert "#define DGRP_ABI_VERSION 1\n" in header
    src = open(os.path.join(ROOT, "deepgrp_amd", "csrc", "rows_parse_kernels.hip")).read()
    assert src.count("DGRP_EXPORT") == 2 and "rows_parse_kernels.o" in open(os.path.join(ROOT, "deepgrp_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the flattening rule in numpy
@pytest.mark.parametrize("case", sorted(FOREIGN))
def test_flatten_reference_on_hand_made_rows(case):
    from deepgrp_amd.compare import flatten_reference
    given, want = FOREIGN[case]
    got = flatten_reference(*FOREIGN_SPAN, given)
    assert got.dtype == SEG
    assert got[["start", "end", "label"]].tolist() == want[["start", "end", "label"]].tolist()
    # flattening what is flat already changes nothing, whatever the order of the rows
    again = flatten_reference(*FOREIGN_SPAN, got[::-1])
    assert again.tolist() == got.tolist()


def test_flatten_reference_gives_ascending_disjoint_rows():
    from deepgrp_amd.compare import flatten_reference
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 300):
        o = int(rng.integers(0, 1000))
        s = rng.integers(o - 20, o + n + 20, 60)
        given = rows(*[(int(a), int(a) + int(rng.integers(0, 40)), int(rng.integers(1, 5))) for a in s])
        got = flatten_reference(o, n, given)
        track = np.zeros(n, np.int64)
        for a, e, lab, _c in got.tolist():
            assert o <= a < e <= o + n and (track[a - o:e - o] == 0).all()
            track[a - o:e - o] = lab
        assert (got["start"][1:] >= got["end"][:-1]).all()
        want = np.full(n, 99, np.int64)
        for a, e, lab, _c in given.tolist():
            a, e = max(a - o, 0), min(e - o, n)
            if e > a:
                want[a:e] = np.minimum(want[a:e], lab)
        assert track.tolist() == np.where(want == 99, 0, want).tolist()
        # abutting rows of one label exist only at the last base
        same = (got["start"][1:] == got["end"][:-1]) & (got["label"][1:] == got["label"][:-1])
        assert all(int(got["end"][k + 1]) == o + n and int(got["start"][k + 1]) == o + n - 1 for k in np.flatnonzero(same))
    assert len(flatten_reference(5, 0, rows((1, 9, 1)))) == 0
