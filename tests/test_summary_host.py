"""`predict --summary_dir` on the CPU: the numpy statement of the counts on a hand-written body, its sums over the corpus, N50, the
file byte for byte, the symbol's declaration and binding, and every refusal of the flags by a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import summary_cases as sc
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_H5 = os.path.join(GOLDEN, "model_u60_T342_att.h5")
SEG = sc.SEG


def _rows(*rows):
    return np.array([(s, e, lab, 0) for s, e, lab in rows], SEG)


# the sequence ACGTacgtNNnnRY: [0, 2) label 1, [2, 6) label 2, [13, 14) label 1
CHUNK = b">r1 first record\nACGTacgtNN\r\nnnRY\n"
ROWS = ((0, 2, 1), (2, 6, 2), (13, 14, 1))


def _r1():
    from deepgrp_amd.masking import sequence_byte_offsets
    (header, offs), = sequence_byte_offsets(CHUNK)
    assert header == "r1 first record" and bytes(CHUNK[i] for i in offs) == b"ACGTacgtNNnnRY"
    return offs


# ------------------------------------------------------------------------- the statement
def test_count_host_on_a_hand_written_body():
    from deepgrp_amd import summary
    counts = summary.count_host(CHUNK, _r1(), _rows(*ROWS), 3)
    assert counts.shape == (3, 5, 2) and counts.dtype == np.int64
    #            A      C      G      T      other      (upper, lower)
    want = [[[0, 0], [0, 0], [0, 1], [0, 1], [3, 2]],           # g t N N n n R
            [[1, 0], [1, 0], [0, 0], [0, 0], [1, 0]],           # A C Y
            [[0, 1], [0, 1], [1, 0], [1, 0], [0, 0]]]           # G T a c
    assert counts.tolist() == want
    assert summary.count_host(CHUNK, _r1(), _rows(), 3)[0].sum() == 14


def test_bins_host_on_a_hand_written_body():
    from deepgrp_amd import summary
    bins = summary.bins_host(CHUNK, _r1(), _rows(*ROWS), 3, 4)
    assert bins.tolist() == [[4, 2, 2], [4, 0, 2], [0, 0, 0], [0, 1, 0]] and bins.dtype == np.int64
    assert summary.bins_host(CHUNK, _r1(), _rows(*ROWS), 3, 1).shape == (14, 3)
    assert summary.bins_host(CHUNK, _r1(), _rows(*ROWS), 3, 100).tolist() == [[8, 3, 4]]
    assert summary.format_density(b"r1", bins, 14, 4) == b"r1\t0\t4\t4\t2\t2\nr1\t4\t8\t4\t0\t2\nr1\t8\t12\t0\t0\t0\nr1\t12\t14\t0\t1\t0\n"
    assert summary.density_header(3, [b"LINE", b"SINE"]) == b"#record\tstart\tend\tacgt\tLINE\tSINE\n"
    assert summary.density_header(3) == b"#record\tstart\tend\tacgt\tclass1\tclass2\n"


@pytest.mark.parametrize("what,rows", [("label", ((0, 2, 3),)), ("label", ((0, 2, -1),)), ("empty", ((3, 3, 1),)),
                                       ("order", ((0, 5, 1), (4, 6, 1))), ("beyond", ((10, 15, 1),)), ("negative", ((-1, 2, 1),))])
def test_count_host_refuses_a_bad_row(what, rows):
    from deepgrp_amd import summary
    with pytest.raises(ValueError, match="row 0 "):
        summary.count_host(CHUNK, _r1(), _rows(*rows), 3)
    assert summary.bad_row(_rows(*rows), 14, 3) == 0 and summary.bad_row(_rows(*ROWS), 14, 3) == -1


@pytest.mark.parametrize("C", [2, 5, 16])
def test_the_sums_of_a_table_over_the_corpus(C):
    """A record's table sums to its sequence length; its labels > 0 to the lengths of their rows; every bin table to the same."""
    from deepgrp_amd import summary
    buf, offs, lens, rowsets = sc.corpus(C)
    rows, row_off = sc.seg_array(rowsets)
    for k in range(len(offs)):
        pos = sc.positions(buf, int(offs[k]), int(lens[k]))
        rk = rows[row_off[k]:row_off[k + 1]]
        counts = summary.count_host(buf, pos, rk, C)
        assert counts.sum() == pos.size
        per_label = np.bincount(rk["label"], weights=rk["end"] - rk["start"], minlength=C).astype(np.int64)
        assert counts[1:].sum(axis=(1, 2)).tolist() == per_label[1:].tolist()
        bins = summary.bins_host(buf, pos, rk, C, 7)
        assert bins.shape == ((pos.size + 6) // 7, C)
        assert bins[:, 0].sum() == counts[:, :4].sum() and bins[:, 1:].sum(axis=0).tolist() == per_label[1:].tolist()


def test_n50_and_row_stats():
    from deepgrp_amd import summary
    assert summary.n50([]) == -1
    assert summary.n50([7]) == 7                                         # one row
    assert summary.n50([5, 5, 5, 5]) == 5                                # equal lengths
    assert summary.n50([2, 8, 6, 4]) == 6                                # 8 + 6 = 14 of 20: past half at the second
    assert summary.n50([10, 6, 4]) == 10                                 # an even split: the first reaches half exactly
    assert summary.n50([4, 6, 5, 5]) == 5                                # 6 + 5 = 11 of 20
    assert summary.n50([6, 4, 5, 5, 0]) == 5
    st = summary.row_stats(_rows((0, 10, 1), (10, 16, 1), (20, 24, 2), (30, 31, 0)), 4)
    assert st.tolist() == [[1, 1, 1, 1, 1], [2, 16, 6, 10, 10], [1, 4, 4, 4, 4], [0, 0, -1, -1, -1], [3, 20, 4, 10, 10]]
    assert summary.row_stats(_rows(), 2).tolist() == [[0, 0, -1, -1, -1]] * 3


WANT = (b"#record\tlabel\trows\tbases\tA\tC\tG\tT\tother\tlower\tmin\tmax\tN50\tfrac_record\tfrac_acgt\tgc\tmask_recall\tmask_precision\n"
        b"r1\tclass0\t0\t7\t0\t0\t1\t1\t5\t4\t.\t.\t.\t0.500000\t0.250000\t0.500000\t.\t.\n"
        b"r1\tLINE\t2\t3\t1\t1\t0\t0\t1\t0\t1\t2\t2\t0.214286\t0.250000\t0.500000\t.\t.\n"
        b"r1\tSINE\t1\t4\t1\t1\t1\t1\t0\t2\t4\t4\t4\t0.285714\t0.500000\t0.500000\t.\t.\n"
        b"r1\tall\t3\t7\t2\t2\t1\t1\t1\t2\t1\t4\t4\t0.500000\t0.750000\t0.500000\t0.333333\t0.285714\n"
        b"e\tclass0\t0\t2\t0\t0\t0\t0\t2\t0\t.\t.\t.\t1.000000\t.\t.\t.\t.\n"
        b"e\tLINE\t0\t0\t0\t0\t0\t0\t0\t0\t.\t.\t.\t0.000000\t.\t.\t.\t.\n"
        b"e\tSINE\t0\t0\t0\t0\t0\t0\t0\t0\t.\t.\t.\t0.000000\t.\t.\t.\t.\n"
        b"e\tall\t0\t0\t0\t0\t0\t0\t0\t0\t.\t.\t.\t0.000000\t.\t.\t.\t.\n"
        b"u\tclass0\t0\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\n"
        b"u\tLINE\t1\t.\t.\t.\t.\t.\t.\t.\t3\t3\t3\t.\t.\t.\t.\t.\n"
        b"u\tSINE\t0\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\n"
        b"u\tall\t1\t.\t.\t.\t.\t.\t.\t.\t3\t3\t3\t.\t.\t.\t.\t.\n"
        b"*\tclass0\t0\t9\t0\t0\t1\t1\t7\t4\t.\t.\t.\t0.562500\t0.250000\t0.500000\t.\t.\n"
        b"*\tLINE\t3\t3\t1\t1\t0\t0\t1\t0\t1\t3\t3\t0.187500\t0.250000\t0.500000\t.\t.\n"
        b"*\tSINE\t1\t4\t1\t1\t1\t1\t0\t2\t4\t4\t4\t0.250000\t0.500000\t0.500000\t.\t.\n"
        b"*\tall\t4\t7\t2\t2\t1\t1\t1\t2\t1\t4\t3\t0.437500\t0.750000\t0.500000\t0.333333\t0.285714\n")


def test_format_summary_byte_for_byte():
    """Three records: the hand-written one; `e` = NN without rows (no ACGT, no lower case, no predicted base: `.` for every empty
    denominator); `u`, whose bytes cannot be counted (`.` in every base-level column, its row still counted)."""
    from deepgrp_amd import summary
    r1 = summary.count_host(CHUNK, _r1(), _rows(*ROWS), 3)
    e = summary.count_host(b"NN", np.arange(2), _rows(), 3)
    records = [(b"r1", r1, _rows(*ROWS)), (b"e", e, _rows()), (b"u", None, _rows((5, 8, 1)))]
    assert summary.format_summary(records, 3, [b"LINE", b"SINE"]) == WANT
    plain = summary.format_summary(records, 3)
    assert plain == WANT.replace(b"\tLINE\t", b"\tclass1\t").replace(b"\tSINE\t", b"\tclass2\t")
    with pytest.raises(ValueError, match="names"):
        summary.format_summary(records, 3, [b"LINE"])
    # a name is written as it is: one that would break the columns is refused, in either file
    for bad in ([b"LI\tNE", b"SINE"], [b"LINE", b"SI\nNE"], [b"LINE", b""]):
        assert summary.names_refusal(bad) is not None
        with pytest.raises(ValueError, match="--bed_names"):
            summary.format_summary(records, 3, bad)
        with pytest.raises(ValueError, match="--bed_names"):
            summary.density_header(3, bad)
    assert summary.names_refusal([b"LINE/L1", "S\u00e9 ne".encode()]) is None      # blanks and non-ASCII bytes keep the columns
    assert summary.format_summary([], 2).count(b"\n") == 4                  # header and the totals of nothing


def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_repeat_summary_workspace_bytes", "dgrp_repeat_summary_batch"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    q = _lib.lib().dgrp_repeat_summary_workspace_bytes
    sizes = [q(3, 1 << 20, n) for n in (0, 1, 100, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and q(-1, 5, 5) == 0 and q(1, -5, 5) == 0 and q(1, 5, -5) == 0
    assert q(3, 1 << 30, 0) > q(3, 1 << 20, 0)
    assert "summary_kernels.o" in open(os.path.join(ROOT, "deepgrp_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------------- command line
def test_flags_parse_on_predict_and_in_the_short_form(tmp_path):
    from deepgrp_amd import summary
    from deepgrp_amd.__main__ import CommandLineParser
    a = CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--summary_dir", "d", "--summary_bin", "1000", "--bed_names", "x,y"]).args
    assert a.summary_dir == "d" and a.summary_bin == 1000 and a.bed_names == "x,y"
    b = CommandLineParser().parse_args(["--summary_dir", "d", "--summary_bin", "5", "m.h5", "a.fa"]).args
    assert b.command == "predict" and b.summary_dir == "d" and b.summary_bin == 5 and b.FASTA == ["a.fa"]
    c = CommandLineParser().parse_args(["predict", "m.h5", "a.fa"]).args
    assert getattr(c, "summary_dir", None) is None and summary.plan(c) is None
    fa = tmp_path / "a.fa"
    fa.write_text(">x\nACGT\n")
    d = CommandLineParser().parse_args(["predict", "m.h5", str(fa), "--summary_dir", str(tmp_path / "o"), "--summary_bin", "9"]).args
    plan = summary.plan(d)
    assert plan._asdict() == dict(files={str(fa): (str(tmp_path / "o" / "a.fa.summary.tsv"), str(tmp_path / "o" / "a.fa.density.tsv"))}, bin=9, names=None)
    e = CommandLineParser().parse_args(["predict", "m.h5", str(fa), "--summary_dir", str(tmp_path / "o"), "--bed_names", "L,S"]).args
    assert summary.plan(e).names == (b"L", b"S")
    assert summary.plan(e).files[str(fa)][1] is None


CHILD = ("import sys\n"
         "from deepgrp_amd.__main__ import main\n"
         "try:\n"
         "    main(sys.argv[1:])\n"
         "except SystemExit as e:\n"
         "    import deepgrp_amd._lib as l\n"
         "    print('LOADED' if (l._lib is not None or 'torch' in sys.modules or 'h5py' in sys.modules) else 'CLEAN')\n"
         "    raise\n")


def _refused(tmp_path, argv, env=None, stdin=None):
    full = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    full.pop("WORLD_SIZE", None)
    full.update(env or {})
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([sys.executable, "-c", CHILD] + argv, env=full, capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                       input=stdin)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stdout.strip() == "CLEAN", r.stdout                          # before the model is read or the device touched
    assert sorted(os.listdir(tmp_path)) == before                           # nothing written, no directory made
    return r.stderr


def test_every_refusal_names_the_flag_and_writes_nothing(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">x\nACGT\n")
    other = tmp_path / "sub"
    other.mkdir()
    (other / "a.fa").write_text(">y\nACGT\n")
    npz = tmp_path / "b.fa.gz.npz"
    npz.write_bytes(b"PK\x03\x04")
    out = str(tmp_path / "out")
    base = ["predict", MODEL_H5]
    err = _refused(tmp_path, base + [str(fa), "--summary_bin", "100"])
    assert "--summary_bin needs --summary_dir" in err
    err = _refused(tmp_path, base + [str(fa), "--summary_dir", out, "--summary_bin", "0"])
    assert "--summary_bin must be at least 1" in err
    err = _refused(tmp_path, base + ["-", "--summary_dir", out], stdin=">x\nACGT\n")
    assert "--summary_dir" in err and "standard input" in err
    err = _refused(tmp_path, base + [str(npz), "--summary_dir", out])
    assert "--summary_dir" in err and ".npz" in err
    err = _refused(tmp_path, base + [str(fa), str(other / "a.fa"), "--summary_dir", out])
    assert "--summary_dir" in err and "same file name a.fa.summary.tsv" in err
    clash = tmp_path / "a.fa.summary.tsv"
    clash.write_text(">z\nACGT\n")
    err = _refused(tmp_path, base + [str(fa), str(clash), "--summary_dir", str(tmp_path)])
    assert "--summary_dir" in err and "would overwrite the input" in err
    dens = tmp_path / "a.fa.density.tsv"
    dens.write_text(">z\nACGT\n")
    err = _refused(tmp_path, base + [str(fa), str(dens), "--summary_dir", str(tmp_path), "--summary_bin", "10"])
    assert "--summary_dir" in err and "would overwrite the input" in err and "density" in err
    err = _refused(tmp_path, base + [str(fa), "--summary_dir", out], env={"WORLD_SIZE": "2"})
    assert "--summary_dir" in err and "WORLD_SIZE" in err
    err = _refused(tmp_path, base + [str(fa), "--summary_dir", out, "--split_contigs"])
    assert "--summary_dir" in err and "--split_contigs" in err
    err = _refused(tmp_path, base + [str(fa), "--summary_dir", out, "--bed_names", "a,,b"])
    assert "--bed_names" in err
    for bad in ("LINE\tL1,SINE", "LINE,SI\nNE", "a\rb,c", "a,b\x7f"):
        err = _refused(tmp_path, base + [str(fa), "--summary_dir", out, "--bed_names", bad])
        assert "--bed_names" in err and "control character" in err and "--summary_dir" in err
    err = _refused(tmp_path, base + [str(fa), "--bed_names", "a,b"])
    assert "--bed_names needs --bed_gff3" in err                          # without --summary_dir the names still have no use
    ann = tmp_path / "ann.bed"
    ann.write_text("x\t0\t2\t1\n")
    err = _refused(tmp_path, ["--summary_dir", out, "evaluate", MODEL_H5, str(ann), str(fa)])
    assert "--summary_dir belongs to predict" in err
    err = _refused(tmp_path, ["--summary_bin", "5", "evaluate", MODEL_H5, str(ann), str(fa)])
    assert "--summary_dir belongs to predict" in err


def test_write_summary_checks_its_arguments_before_any_work(tmp_path):
    from deepgrp_amd import summary
    rows = _rows()
    with pytest.raises(ValueError, match="classes"):
        summary.write_summary("a.fa", str(tmp_path / "s"), rows, 1)
    with pytest.raises(ValueError, match="classes"):
        summary.write_summary("a.fa", str(tmp_path / "s"), rows, 65)
    with pytest.raises(ValueError, match="density"):
        summary.write_summary("a.fa", str(tmp_path / "s"), rows, 3, bin=5)
    with pytest.raises(ValueError, match="names"):
        summary.write_summary("a.fa", str(tmp_path / "s"), rows, 3, names=[b"one"])
    assert os.listdir(tmp_path) == []
