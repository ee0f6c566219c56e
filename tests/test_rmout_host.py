"""predict --bed_rmout without a GPU: rmout.reference_lines against a hand-written line; the statement's text read back by the
project's own readers (parse_rm.read_repeatmasker, annotation.read_listing on the host, annotation.sniff) row for row; the
`repeat#class/family` names through parse_rm.parse_line; rmout.reference_ids on hand-made rows; every field grown past its width; every
refusal of the command line in a child process that sees no device, before any file is read and without a traceback (the label
counts: right after the model is read); the two entry points declared, exported and bound, and their host refusals; BedFiles in
listing form on fake writes: the header first, the IDs carried from write to write, no file for a record name with a blank, nothing
left behind on abort."""
import argparse
import json
import logging
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from deepgrp_amd import bed, gz, rmout
from deepgrp_amd._scripts import parse_rm
from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE

ONE = 1 << 24
EINVAL = -1
TEN = rmout.pairs_of_repeats(range(1, 11))


def segs(rows):
    a = np.zeros(len(rows), SEGMENT_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def scores_of(rows):
    a = np.zeros(len(rows), ROW_SCORE_DTYPE)
    for i, (s, b, g, m) in enumerate(rows):
        a[i] = (s, b, g, m, 0)
    return a


def full(n):
    """n rows of score 1000"""
    return scores_of([(7 * ONE, 7, 7, ONE)] * n)


# ---- the statements ------------------------------------------------------------------------------------------------------------------
def test_the_example_of_the_format():
    rows = segs([(99, 350, 3, 0), (1000, 1010, 1, 0), (0, 5, 4, 1)])
    sc = scores_of([(int(0.93 * ONE) * 251, 251, 240, int(0.41 * ONE)), (ONE * 10, 10, 10, ONE), (int(0.5004 * ONE) * 5, 5, 3, ONE // 2)])
    text, lines, ids = rmout.reference_lines([b"chr1", b"scaf2"], True, rows, sc, 0, [2000, 5], TEN[:4], None, 8)
    assert (lines, ids) == (3, 3)
    got = text.split(b"\n")
    assert got[0] == b"  930   0.0  0.0  0.0  chr1                   100       350      (1650) +  Alu          SINE/Alu              1    251    (0)      9"
    assert got[1] == b" 1000   0.0  0.0  0.0  chr1                  1001      1010       (990) +  HSATII       Satellite             1     10    (0)     10"
    assert got[2] == b"  500   0.0  0.0  0.0  scaf2                    1         5         (0) +  L1           LINE/L1               1      5    (0)     11"
    assert got[3] == b"" and len(got) == 4


def test_the_header_stands_over_the_columns():
    one, two, blank = rmout.HEADER.split(b"\n")[:3]
    assert rmout.HEADER.count(b"\n") == 3 and blank == b""
    assert one.startswith(b"   SW   perc perc perc  query") and two.startswith(b"score   div. del. ins.  sequence")
    line = rmout.LINE % (1, b"0.0", b"0.0", b"0.0", b"n" * 16, 1, 1, b"(1)", b"r" * 12, b"f" * 16, 1, 1, b"(0)", 1)
    # the fields of a line of minimum widths: where each one begins and ends
    left = lambda word, ln: ln.index(word)
    right = lambda word, ln: ln.rindex(word) + len(word)
    assert left(b"sequence", two) == line.index(b"n" * 16) + 1                        # (a column to the right, as RepeatMasker has it)
    assert right(b"begin", two[:60]) == 49 and right(b" end", two[:60]) == 59 and right(b"(left)", two[:75]) == 71
    assert left(b"repeat", two) == line.index(b"r" * 12) == left(b"matching", one)
    assert left(b"class/family", two) == line.index(b"f" * 16) == left(b"repeat", one[80:]) + 80
    assert right(b"begin", two) == 111 and right(b" end", two) == 118 and right(b"(left)", two) == 125 and right(b"ID", two) == 132 == len(line) - 1
    for ln in (one, two):                                                             # no reader of the project takes a title line for a row
        assert parse_rm.parse_line(ln.decode()).ctg is None


@pytest.fixture(scope="module")
def corpus():
    """300 seeded rows over 3 records, all ten families, coordinates of 1 to 11 digits, names of 1 and 255 bytes."""
    rng = np.random.default_rng(20)
    names = [b"x", b"n" * 255, b"chr7_random"]
    ends = [40, 5_000_000, 30_000_000_000]
    repeats = [int(n) for n in rng.permutation(10) + 1]
    rows = np.zeros(300, SEGMENT_DTYPE)
    rows["contig"] = np.sort(rng.integers(0, 3, 300))
    rows["contig"][:3] = 0
    for r in range(3):
        sel = np.flatnonzero(rows["contig"] == r)
        digits = rng.integers(1, len(str(ends[r])) + 1, len(sel))
        start = np.sort([min(int(rng.integers(10 ** (d - 1) - (d == 1), 10 ** d)), ends[r] - 2) for d in digits])
        rows["start"][sel] = start
        rows["end"][sel] = [min(int(s) + 1 + int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), ends[r]) for s in start]
    rows["label"] = rng.permutation(np.arange(300) % 10) + 1
    sc = np.zeros(300, ROW_SCORE_DTYPE)
    sc["bases"] = rng.integers(1, 1000, 300)
    sc["sum"] = [int(b) * int(rng.integers(0, ONE + 1)) for b in sc["bases"]]
    sc["agree"], sc["qmin"] = sc["bases"], 0
    assert {len(str(int(e))) for e in rows["end"]} >= set(range(1, 12)) and int(rows["start"].min()) == 0
    return names, ends, repeats, rows, sc


@pytest.mark.parametrize("join", [None, 1000])
def test_round_trip_through_the_readers(tmp_path, corpus, join):
    from deepgrp_amd import annotation
    names, ends, repeats, rows, sc = corpus
    text, lines, ids = rmout.reference_lines(names, True, rows, sc, 0, ends, rmout.pairs_of_repeats(repeats), join, 0)
    assert lines == 300 and (ids == 300) == (join is None)
    path = tmp_path / "pred.out"
    path.write_bytes(rmout.HEADER + text)
    want = [(names[int(r["contig"])].decode(), int(r["start"]), int(r["end"]), repeats[int(r["label"]) - 1]) for r in rows]
    back = list(parse_rm.read_repeatmasker(*parse_rm.pentamer_sets(), (rmout.HEADER + text).decode().splitlines(True)))
    assert [(r.ctg, r.start, r.end, r.typ) for r in back] == want
    assert annotation.sniff(str(path)) == "repeatmasker"
    lst = annotation.read_listing(str(path), device=False)
    ctg_names, ctg_of = lst.contigs()
    assert lst.route == "host" and len(lst) == 300
    assert [(ctg_names[int(c)], int(b), int(e), int(n)) for c, b, e, n in zip(ctg_of, lst.begin, lst.end, lst.number)] == want
    assert (lst.millidiv == 0).all()                                                  # (written 0.0: not a prediction, see rmout.py)


def test_names_in_library_form_come_back_through_parse_line():
    cn = (b"LTR-1#LTR/Gypsy", b"AluY#SINE/Alu", b"odd|name.3#Unknown")
    assert rmout.names_refusal(cn) is None
    pairs = rmout.pairs_of_names(cn)
    assert pairs == ((b"LTR-1", b"LTR/Gypsy"), (b"AluY", b"SINE/Alu"), (b"odd|name.3", b"Unknown"))
    text, lines, _ids = rmout.reference_lines([b"c"], False, segs([(5, 9, 1, 0), (20, 30, 3, 0), (40, 50, 2, 0)]), full(3), 0, [50], pairs)
    back = [parse_rm.parse_line(ln.decode()) for ln in text.split(b"\n")[:-1]]
    assert [(r.rep, r.fam, r.typ) for r in back] == [("LTR-1", "LTR/Gypsy", 10), ("odd|name.3", "Unknown", 0), ("AluY", "SINE/Alu", 3)]
    for n in range(1, 11):                                                            # and the default pairs to their numbers
        rep, fam = rmout.pair_of_repeat(n)
        line = rmout.LINE % (0, b"0.0", b"0.0", b"0.0", b"c", 1, 2, b"(0)", rep, fam, 1, 2, b"(0)", 1)
        assert parse_rm.parse_line(line.decode()).typ == n
    assert TEN[0] == (b"HSATII", b"Satellite") and TEN[1] == (b"ALR/Alpha", b"Satellite/centr") and TEN[8] == (b"ERVL-MaLR", b"LTR/ERVL-MaLR")
    for bad, words in (((b"noseparator",), "exactly one '#'"), ((b"a#b#c",), "exactly one '#'"), ((b"ok#x", b"#fam"), "label 2 has an empty side"),
                       ((b"rep#",), "empty side"), ((b"a b#c",), "blank"), ((b"a#c\x7f",), "blank"), ((b"a\t#c",), "blank"),
                       ((b"a#" + b"b" * 254,), "has 256 bytes, above 255")):
        assert words in rmout.names_refusal(bad), bad
    assert rmout.names_refusal((b"a#" + b"b" * 253,)) is None


def test_reference_ids():
    rows = segs([(0, 10, 1, 0), (15, 20, 1, 0), (26, 30, 1, 0), (30, 40, 2, 0), (45, 50, 1, 0), (50, 60, 1, 1), (61, 70, 1, 1)])
    every = [True] * len(rows)
    # gaps in record 0: 5 (rows 0-1), 6 (rows 1-2), another label, then label 1 again; rows 4-5 cross a record edge with gap 0
    assert rmout.reference_ids(rows, every, True, None, 0) == ([1, 2, 3, 4, 5, 6, 7], 7)
    assert rmout.reference_ids(rows, every, True, -1, 3) == ([4, 5, 6, 7, 8, 9, 10], 7)
    assert rmout.reference_ids(rows, every, True, 0, 0) == ([1, 2, 3, 4, 5, 6, 7], 7)
    assert rmout.reference_ids(rows, every, True, 1, 0) == ([1, 2, 3, 4, 5, 6, 6], 6)
    assert rmout.reference_ids(rows, every, True, 5, 0) == ([1, 1, 2, 3, 4, 5, 5], 5)                # a gap of exactly G joins, G + 1 does not
    assert rmout.reference_ids(rows, every, True, 6, 0) == ([1, 1, 1, 2, 3, 4, 4], 4)
    # 10^9: still no join across another label (rows 2-3-4) nor across the record edge (rows 4-5)
    assert rmout.reference_ids(rows, every, True, 10 ** 9, 7) == ([8, 8, 8, 9, 10, 11, 11], 4)
    assert rmout.reference_ids(rows, every, False, 10 ** 9, 0) == ([1, 1, 1, 2, 3, 3, 3], 3)         # (one record: the edge is none)
    # a filtered row in between neither joins nor breaks: rows 0 and 2 are 16 apart; the other label filtered joins rows 2 and 4
    assert rmout.reference_ids(rows, [True, False, True, True, True, True, True], True, 16, 0) == ([1, 1, 2, 3, 4, 4], 4)
    assert rmout.reference_ids(rows, [True, False, True, True, True, True, True], True, 15, 0) == ([1, 2, 3, 4, 5, 5], 5)
    assert rmout.reference_ids(rows, [True, True, True, False, True, True, True], True, 15, 0) == ([1, 1, 1, 1, 2, 2], 2)
    assert rmout.reference_ids(rows, [False] * len(rows), True, 5, 9) == ([], 0)
    assert rmout.reference_ids(rows[:0], [], True, 5, 9) == ([], 0)
    with pytest.raises(ValueError):
        rmout.reference_ids(rows, every, True, -2, 0)
    # the lines carry them, and the count of IDs is what the file advances by
    text, lines, ids = rmout.reference_lines([b"a", b"b"], True, rows, full(7), 0, [60, 70], TEN[:2], 5, 40)
    assert (lines, ids) == (7, 5) and [int(ln.split()[-1]) for ln in text.split(b"\n")[:-1]] == [41, 41, 42, 43, 44, 45, 45]


def test_every_field_grows_past_its_width():
    """Against the `%` expression, written out once more here with the fields of this very row."""
    name, rep, fam = b"s" * 17, b"r" * 13, b"f" * 17
    start, end, rec_end, id0 = 10 ** 9, 10 ** 10 + 10 ** 9, 10 ** 11, 10 ** 6 - 1
    text, lines, ids = rmout.reference_lines([name], False, segs([(start, end, 1, 0)]), full(1), 0, [rec_end], [(rep, fam)], None, id0)
    want = b"%5d %5s %4s %4s  %-16s %9d %9d %11s +  %-12s %-16s %6d %6d %6s %6d\n" % (
        1000, b"0.0", b"0.0", b"0.0", name, start + 1, end, b"(%d)" % (rec_end - end), rep, fam, 1, end - start, b"(0)", id0 + 1)
    assert text == want and (lines, ids) == (1, 1)
    assert text.split() == [b"1000", b"0.0", b"0.0", b"0.0", name, b"1000000001", b"11000000000", b"(89000000000)", b"+", rep, fam, b"1",
                            b"10000000000", b"(0)", b"1000000"]
    assert b" " + name + b" 1000000001 11000000000 (89000000000) +  " + rep + b" " + fam + b"      1 10000000000    (0) 1000000\n" in text
    short, _l, _i = rmout.reference_lines([b"s"], False, segs([(0, 1, 1, 0)]), scores_of([(0, 3, 0, 0)]), 0, [1], [(b"r", b"f")])
    assert len(short) == 133 and len(text) > len(short)
    with pytest.raises(ValueError, match="outside its record"):
        rmout.reference_lines([b"s"], False, segs([(0, 5, 1, 0)]), full(1), 0, [4], [(b"r", b"f")])
    with pytest.raises(ValueError, match="label 2 outside"):
        rmout.reference_lines([b"s"], False, segs([(0, 5, 2, 0)]), full(1), 0, [9], [(b"r", b"f")])


def test_min_score_filters_lines_not_ids_of_neighbours():
    rows = segs([(0, 10, 1, 0), (12, 20, 1, 0), (22, 30, 1, 0)])
    sc = scores_of([(7 * ONE, 7, 7, ONE), (0, 7, 0, 0), (7 * ONE, 7, 7, ONE)])
    text, lines, ids = rmout.reference_lines([b"a"], False, rows, sc, 1, [30], TEN, 12, 0)
    assert (lines, ids) == (2, 1) and [ln.split()[-1] for ln in text.split(b"\n")[:-1]] == [b"1", b"1"]
    assert rmout.reference_lines([b"a"], False, rows, sc, 0, [30], TEN, 2, 0)[1:] == (3, 1)


# ---- the library -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


NEW = ("dgrp_rmout_text_workspace_bytes", "dgrp_rmout_text_batch")


def test_symbols_declared_exported_and_bound(L):
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in NEW:
        assert name in _lib.exported_symbols() and hasattr(L, name) and name + "(" in header, name
        assert getattr(L, name).argtypes is not None


def test_the_host_refusals_come_before_any_device_work(L):
    """NULL or descending tables, id0 and join_gap out of range, no class names, record ends outside 1..2^62, too many rows: DGRP_EINVAL
    from the host checks, with no device pointer ever read (they are NULL or made up here)."""
    import ctypes as C
    wq = L.dgrp_rmout_text_workspace_bytes
    assert wq(0, 1, 0, 1, 0, 1) > 0 and wq(5000, 3, 40, 4, 30, 3) >= 5000 * 48 + 40 + 30 + 4 * 8 + 9 * 8 + 3 * 8
    for bad in ((-1, 1, 0, 1, 0, 1), (10, 0, 0, 1, 0, 1), (10, 1, -1, 1, 0, 1), ((1 << 31) - 256, 1, 0, 1, 0, 1), (10, 1, 0, 0, 0, 1),
                (10, 1, 0, 1, -1, 1), (10, 1, 0, 1, 0, 0), (10, 1, 0, 1, 0, 1 << 31)):
        assert wq(*bad) == 0, bad
    got = [C.c_int64(-7) for _ in range(3)]
    off, coff = np.array([0, 3], np.int64), np.array([0, 2, 5, 5, 9], np.int64)
    bogus = 0xdead0000

    def call(names=b"abc", name_off=off, cnames=b"L1LTRLINE", cname_off=coff, ncnames=2, nrows=0, ends=(100,), nrec=None, by_contig=0, join=-1,
             id0=0, rows=None, outs=(True, True, True)):
        e = np.array(ends, np.int64)
        for g in got:
            g.value = -7
        ptr = [C.byref(g) if o else None for g, o in zip(got, outs)]
        return L.dgrp_rmout_text_batch(names, name_off.ctypes.data, 1, by_contig, cnames, None if cname_off is None else cname_off.ctypes.data,
                                       ncnames, rows, rows, nrows, 0, len(e) if nrec is None else nrec, e.ctypes.data, join, id0, None, 0,
                                       ptr[0], ptr[1], ptr[2], None, 0, None)
    assert call() == 0 and [g.value for g in got] == [0, 0, 0]
    assert call(ends=(1 << 62,), id0=1 << 62, join=1 << 62) == 0
    assert call(names=None) == EINVAL
    assert call(name_off=np.array([3, 0], np.int64)) == EINVAL and b"ascend" in L.dgrp_last_error()
    assert call(cname_off=np.array([0, 2, 5, 4, 9], np.int64)) == EINVAL and b"class-name offsets must ascend" in L.dgrp_last_error()
    assert call(cnames=None) == EINVAL and call(cname_off=None) == EINVAL
    assert call(ncnames=0) == EINVAL and b"class-name count" in L.dgrp_last_error()
    assert call(id0=-1) == EINVAL and b"id0" in L.dgrp_last_error()
    assert call(id0=(1 << 62) + 1) == EINVAL and b"id0" in L.dgrp_last_error()
    assert call(join=-2) == EINVAL and b"join_gap" in L.dgrp_last_error()
    assert call(join=-2, nrows=4, rows=bogus) == EINVAL and b"join_gap" in L.dgrp_last_error()      # before the rows are looked at
    assert call(ends=(0,)) == EINVAL and b"2^62" in L.dgrp_last_error()
    assert call(ends=((1 << 62) + 1,)) == EINVAL and b"2^62" in L.dgrp_last_error()
    assert call(ends=(100, 100)) == EINVAL and b"nrec must be 1" in L.dgrp_last_error()
    assert call(ends=(100, -5), by_contig=1) == EINVAL and b"record 1" in L.dgrp_last_error()
    assert call(nrec=0) == EINVAL
    for k in range(3):
        assert call(outs=tuple(j != k for j in range(3))) == EINVAL
    assert call(nrows=-1) == EINVAL
    assert call(nrows=(1 << 31) - 256, rows=bogus) == EINVAL and b"too many rows" in L.dgrp_last_error()
    assert call(nrows=4) == EINVAL                                                                  # rows without arrays
    assert call(nrows=4, rows=bogus) != 0 and b"workspace" in L.dgrp_last_error()                    # made-up pointers are never read


# ---- the command line ----------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
from deepgrp_amd.__main__ import main
out = []
for argv in json.load(open(sys.argv[1])):
    try:
        main(argv)
        out.append(None)
    except SystemExit as e:
        out.append(e.code if isinstance(e.code, str) else "exit %r" % (e.code,))
print(json.dumps(out))
"""


def test_cli_refusals_in_a_child_without_a_device(tmp_path):
    """Neither the model nor an input exists: a refusal that read one would be another error."""
    model, fa, out = str(tmp_path / "no_such_model.h5"), str(tmp_path / "no_such.fa"), str(tmp_path / "beds")
    base = ["predict", model, fa]
    rm = base + ["--bed_dir", out, "--bed_rmout"]
    cases = [
        (base + ["--bed_rmout"], "--bed_rmout needs --bed_dir"),
        (["--bed_rmout", model, fa], "--bed_rmout needs --bed_dir"),                                # the README form
        (rm + ["--bed_bigbed"], "they do not go together"),
        (rm + ["--bed_gff3"], "they do not go together"),
        (rm + ["--bed_gzip", "--bed_index"], "--bed_rmout does not go with --bed_index: the listing is blank-separated"),
        (rm + ["--bed_index"], "--bed_index needs --bed_gzip"),                                     # today's message comes first
        (["--bed_rmout", "--bed_dir", out, "evaluate", model, str(tmp_path / "ann.bed"), fa], "--bed_dir belongs to predict"),
        (["--bed_rmout", "evaluate", model, str(tmp_path / "ann.bed"), fa], "--bed_rmout belongs to predict"),
        (["--bed_rmout", "compare", str(tmp_path / "p.tsv"), str(tmp_path / "ann.bed"), fa], "--bed_rmout belongs to predict"),
        (["--rmout_join", "5", "evaluate", model, str(tmp_path / "ann.bed"), fa], "belong to predict"),
        (["--rmout_repeats", "1", "compare", str(tmp_path / "p.tsv"), str(tmp_path / "ann.bed"), fa], "belong to predict"),
        (base + ["--bed_dir", out, "--rmout_repeats", "1,2"], "--rmout_repeats needs --bed_rmout"),
        (["--rmout_repeats", "1,2", "--bed_dir", out, model, fa], "--rmout_repeats needs --bed_rmout"),      # README form: it takes a value
        (rm + ["--rmout_repeats", "1,2,2"], "must be distinct"),
        (rm + ["--rmout_repeats", "0,1"], "0 lies outside 1..10"),
        (rm + ["--rmout_repeats", "3,11"], "11 lies outside 1..10"),
        (rm + ["--rmout_repeats", "1,x"], "not a comma-separated list of numbers"),
        (rm + ["--rmout_repeats", ""], "not a comma-separated list of numbers"),
        (rm + ["--rmout_repeats", "1,2", "--bed_names", "a#b,c#d"], "--rmout_repeats and --bed_names"),
        (base + ["--bed_dir", out, "--rmout_join", "5"], "--rmout_join needs --bed_rmout"),
        (rm + ["--rmout_join", "-1"], "--rmout_join must be 0 or more, not -1"),
        (rm + ["--bed_names", "a#b,plain"], "the name of label 2 must be repeat#class/family with exactly one '#'"),
        (rm + ["--bed_names", "a#b#c"], "exactly one '#'"),
        (rm + ["--bed_names", "#b"], "empty side"),
        (rm + ["--bed_names", "a#"], "empty side"),
        (rm + ["--bed_names", "a x#b"], "blank"),
        (rm + ["--bed_names", "a#b\x7f"], "blank"),
        (rm + ["--bed_names", "a#" + "b" * 254], "has 256 bytes, above 255"),
        (base + ["--bed_dir", out, "--bed_names", "a#b"], "--bed_names needs --bed_gff3"),          # word for word what it was
        (rm + ["--bed_min_score", "1001"], "--bed_min_score must lie in 0..1000"),
        (rm + ["--split_contigs"], "--bed_dir runs in one process"),
        (["predict", model, "-", "-", "--bed_dir", out, "--bed_rmout"], "given twice"),
    ]
    spec = tmp_path / "argvs.json"
    spec.write_text(json.dumps([argv for argv, _m in cases]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="",
               ROCR_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(spec)], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert r.returncode == 0 and b"Traceback" not in r.stderr, r.stderr.decode("utf-8", "replace")[-3000:]
    said = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert len(said) == len(cases)
    for (argv, words), got in zip(cases, said):
        assert got is not None and words in got, (argv, got)
    assert not os.path.exists(out)                                                   # no refusal left a directory behind


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_the_label_counts_are_checked_behind_the_model(monkeypatch, tmp_path):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import CommandLineParser
    classes = [5]
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", lambda *a, **k: {"ff_kernel": np.zeros((16, classes[0]), np.float32)})

    def no_device(*_a, **_k):
        raise AssertionError("the device was reached before the refusal")
    monkeypatch.setattr(dgmodel, "device_model", no_device)
    monkeypatch.setattr(dgmodel, "load_model", no_device)
    monkeypatch.setattr(CommandLineParser, "_pipeline", staticmethod(no_device))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    fa = tmp_path / "a.fa"
    fa.write_text(">r\nACGT\n")
    rm = ["predict", "m.h5", str(fa), "--bed_dir", str(tmp_path / "o"), "--bed_rmout"]
    _refused(rm + ["--rmout_repeats", "1,2,3"], "--rmout_repeats gives 3 numbers, but the model has 4 repeat classes")
    _refused(rm + ["--bed_names", "a#b,c#d"], "--bed_names gives 2 names, but the model has 4 repeat classes")
    classes[0] = 12
    _refused(rm, "--bed_rmout: the model has 11 repeat classes, more than the 10 numbered families")
    _refused(rm + ["--rmout_repeats", "1,2,3,4,5,6,7,8,9,10"], "--rmout_repeats gives 10 numbers, but the model has 11")


def test_plan_and_from_plan(tmp_path):
    d = str(tmp_path / "out")
    ns = lambda **k: argparse.Namespace(bed_dir=d, FASTA=["-", str(tmp_path / "x.fa")], bed_rmout=True, **k)
    p = bed.plan(ns())
    assert p.rmout and p.on_device and p.gzip_level is None and not p.gff3 and not p.bigbed and not p.index
    assert (p.rmout_repeats, p.rmout_join, p.rmout_pairs, p.class_names) == (None, -1, None, None)
    assert p.paths == {"-": os.path.join(d, "stdin.out"), str(tmp_path / "x.fa"): os.path.join(d, "x.fa.out")}
    assert bed.from_plan(p, 5).plan.rmout_pairs == TEN[:4]
    p = bed.plan(ns(bed_gzip=True, rmout_repeats="4,3,2,1", rmout_join=0, bed_min_score=7))
    assert (p.gzip_level, p.rmout_repeats, p.rmout_join, p.min_score) == (1, (4, 3, 2, 1), 0, 7)
    assert p.paths["-"] == os.path.join(d, "stdin.out.gz")
    assert bed.from_plan(p, 5).plan.rmout_pairs == (TEN[3], TEN[2], TEN[1], TEN[0])
    p = bed.plan(ns(bed_names="LTR-1#LTR/Gypsy,A#B/C", gzip_level=0, bed_gzip=True))
    assert p.gzip_level == 0 and bed.from_plan(p, 3).plan.rmout_pairs == ((b"LTR-1", b"LTR/Gypsy"), (b"A", b"B/C"))
    # the fields are new and last: a plan made the old way is what it was
    old = bed.BedPlan(d, 0, {}, None, False, False, True, None)
    assert not old.rmout and old.rmout_join == -1 and old.on_device and bed.BedPlan._fields[:8] == (
        "directory", "min_score", "paths", "gzip_level", "index", "bigbed", "gff3", "class_names")


# ---- BedFiles on fake writes -----------------------------------------------------------------------------------------------------
def _fake_write(p, names, by_contig, rows, scores, rec_end, texts):
    def render(id0):
        text, lines, ids = rmout.reference_lines(names, by_contig, rows, scores, p.min_score, rec_end, p.rmout_pairs, p.rmout_join, id0)
        texts.append((id0, text))
        return rmout.RmoutText(text if p.gzip_level is None else gz.bgzf_compress(text, eof=False), lines, ids)
    return rmout.RmoutWrite(list(names), render if len(rows) else None)


def _plan(tmp_path, gzip, join=-1, low=500):
    final = str(tmp_path / "out" / ("in.fa.out" + (".gz" if gzip else "")))
    return bed.BedPlan(str(tmp_path / "out"), low, {"in.fa": final}, 1 if gzip else None, rmout=True, rmout_join=join, rmout_pairs=TEN[:4])


def _inflate(data):
    out, off = [], 0
    while off < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[off:]))
        off = len(data) - len(d.unused_data)
    return b"".join(out)


@pytest.mark.parametrize("gzip", [False, True])
def test_the_header_only_file(tmp_path, gzip):
    p = _plan(tmp_path, gzip)
    files = bed.BedFiles(p, "in.fa")
    files.write([b"r"], False, None, rmout.RmoutWrite([b"r"]))                        # a record without a row
    files.commit()
    data = open(p.paths["in.fa"], "rb").read()
    if gzip:
        assert data == rmout.header_member(1) + gz.BGZF_EOF and _inflate(data) == rmout.HEADER
    else:
        assert data == rmout.HEADER
    assert os.listdir(p.directory) == [os.path.basename(p.paths["in.fa"])]


@pytest.mark.parametrize("gzip", [False, True])
def test_bedfiles_counts_the_ids_not_the_lines(tmp_path, caplog, gzip):
    p = _plan(tmp_path, gzip, join=10)
    files = bed.BedFiles(p, "in.fa")
    texts = []
    rows1 = segs([(0, 10, 1, 0), (15, 20, 1, 0), (40, 50, 1, 0), (52, 60, 2, 0), (61, 70, 2, 0)])           # IDs 1 1 2 3 3
    sc1 = full(5)
    rows2 = segs([(0, 10, 2, 0), (11, 20, 2, 0), (0, 10, 2, 1), (30, 40, 2, 1), (41, 50, 2, 1), (0, 9, 3, 3)])   # 4 4 5 6 (filtered) 7
    sc2 = full(6)
    sc2["sum"][4] = 0
    w = [_fake_write(p, [b"A"], False, rows1, sc1, [100], texts),
         _fake_write(p, [b"b0", b"b1", b"norows", b"b3"], True, rows2, sc2, [50, 50, 50, 50], texts),
         _fake_write(p, [b"c"], False, segs([(1, 2, 1, 0)]), scores_of([(0, 3, 0, 0)]), [5], texts),       # every line filtered
         _fake_write(p, [b"d"], False, segs([(1, 2, 4, 0)]), full(1), [5], texts)]
    for x in w:
        files.write(x.names, len(x.names) > 1, None, x)
    assert [i for i, _t in texts] == [0, 3, 7, 7] and (files.ids, files.lines) == (8, 11)
    assert os.listdir(p.directory) != [os.path.basename(p.paths["in.fa"])]            # still temporary
    with caplog.at_level(logging.WARNING):
        files.commit()
    assert not caplog.records
    data = open(p.paths["in.fa"], "rb").read()
    want = rmout.HEADER + b"".join(t for _i, t in texts)
    if gzip:
        assert data.startswith(rmout.header_member(1)) and data.endswith(gz.BGZF_EOF)
        data = _inflate(data)
    assert data == want
    assert [int(ln.split()[-1]) for ln in want.split(b"\n")[3:-1]] == [1, 1, 2, 3, 3, 4, 4, 5, 6, 7, 8]
    assert os.listdir(p.directory) == [os.path.basename(p.paths["in.fa"])]


@pytest.mark.parametrize("gzip", [False, True])
@pytest.mark.parametrize("name", [b"", b"two words", b"tab\there", b"del\x7f"])
def test_a_record_name_with_a_blank_leaves_no_file(tmp_path, caplog, gzip, name):
    """One warning that names file and record, no `.out[.gz]`; what an earlier run left is removed; later writes are not rendered."""
    p = _plan(tmp_path, gzip)
    os.makedirs(p.directory)
    open(p.paths["in.fa"], "wb").write(b"left by an earlier run")
    files = bed.BedFiles(p, "in.fa")
    rows, sc, texts = segs([(5, 90, 1, 0), (100, 200, 2, 1), (300, 400, 3, 2)]), full(3), []
    with caplog.at_level(logging.WARNING):
        files.write([b"a"], False, None, _fake_write(p, [b"a"], False, rows, sc, [1000], texts))
        files.write([b"a", name, b"c"], True, None, _fake_write(p, [b"a", name, b"c"], True, rows, sc, [1000] * 3, texts))
        files.write([b"d"], False, None, _fake_write(p, [b"d"], False, rows, sc, [1000], texts))
        files.write([name], False, None, rmout.RmoutWrite([name]))
        files.commit()
    assert len(caplog.records) == 1 and len(texts) == 1 and os.listdir(p.directory) == []
    said = caplog.records[0].getMessage()
    assert said.startswith("in.fa: no RepeatMasker listing is written (--bed_rmout): ")
    assert ("empty name" in said) if not name else (repr(name.decode()) in said)


def test_abort_and_the_wrong_kind_of_write(tmp_path):
    from deepgrp_amd import gff
    p = _plan(tmp_path, True)
    rows, sc = segs([(5, 90, 1, 0), (100, 200, 1, 0)]), full(2)
    files = bed.BedFiles(p, "in.fa")
    files.write([b"a"], False, None, _fake_write(p, [b"a"], False, rows, sc, [1000], []))
    assert len(os.listdir(p.directory)) == 1
    files.abort()
    assert os.listdir(p.directory) == []
    for wrong in (sc, bed.BedWrite(b"", [b"a"]), gff.GffWrite([b"a"])):
        f2 = bed.BedFiles(p, "in.fa")
        try:
            with pytest.raises(ValueError, match="RmoutWrite"):
                f2.write([b"a"], False, rows, wrong)
        finally:
            f2.abort()
    assert os.listdir(p.directory) == []
