"""RepeatMasker listings as annotation, the half that needs no GPU: the format sniffer, the host path of deepgrp_amd/annotation.py
against parse_rm + read_annotation on the reference's own fixture pair, the tables the device numbers with, the command line's flag
and refusals, and the argument checks of dgrp_rm_parse (they come before any device call).  Expected rows are always those of
_scripts/parse_rm.read_repeatmasker (tests/rm_cases.py)."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import rm_cases

LISTING = os.path.join(GOLDEN, "parse_rm_input.out.gz")
TABLE = os.path.join(GOLDEN, "parse_rm_expect.bed")
EINVAL, ENOMEM = -1, -3
P = 0x10000                    # a non-NULL pointer value that is never dereferenced: an earlier check fails


def test_sniff_on_the_golden_pair():
    from deepgrp_amd.annotation import sniff
    assert sniff(LISTING) == "repeatmasker"
    assert sniff(TABLE) == "table"


def test_sniff_on_plain_listings_and_rmsk(tmp_path):
    from deepgrp_amd.annotation import sniff
    p = tmp_path / "a.out"
    p.write_bytes(gzip.open(LISTING).read())
    assert sniff(str(p)) == "repeatmasker"
    p.write_text(rm_cases.HEADER + rm_cases.out_line(fam="DNA/hAT") + "\n")           # a line that matches, numbered or not
    assert sniff(str(p)) == "repeatmasker"
    p.write_text(rm_cases.rmsk_line() + "\n")
    assert sniff(str(p)) == "repeatmasker"
    p.write_text("#" + rm_cases.out_line() + "\n" + "chr1\t0\t10\t1\n" * 20 + rm_cases.out_line() + "\n")   # past the 16 lines looked at
    assert sniff(str(p)) == "table"
    p.write_text("")
    assert sniff(str(p)) == "table"


@pytest.mark.parametrize("text", [
    "# header\n\nchr1\t10\t20\t1\tL1\tLINE\n   \n  # indented comment\nchr2 5 5 2\nchr1\t0\t3\t4\n#chr1\t0\t9\t1\nchr3\t7\t9\t3\tname with spaces\tfam\n",
    "# x\nchr1\t0\t4\t1\n\nchr1\t-1\t5\t1\nchr1\t8\t9\t2\n",
    "# x\nchr1\t0\t4\t1\n\nchr1\t9\t5\t1\nchr1\t8\t9\t2\n",
    "# x\nchr1\t0\t4\t1\n\nchr1\t1.5\t5\t1\nchr1\t8\t9\t2\n",
    "# x\nchr1\t0\t4\t1\n\nchr1\t5\nchr1\t8\t9\t2\n",
    "chr1\t0\t10\t1\n",
    "chr1\t0\t10\t1\nchr1\t20\t10\t2\n",
    "".join(f"chr{k % 3}\t{k * 10}\t{k * 10 + 7}\t{k % 4 + 1}\tn\tf\n" for k in range(2000)),
])
def test_sniff_takes_the_tables_of_the_evaluate_tests_for_tables(tmp_path, text):
    from deepgrp_amd.annotation import sniff
    p = tmp_path / "a.bed"
    p.write_text(text)
    assert sniff(str(p)) == "table"


def test_sniff_takes_synthetic_tables_for_tables(tmp_path):
    from deepgrp_amd import synthetic
    from deepgrp_amd.annotation import sniff
    p = tmp_path / "s.bed"
    p.write_text("# synthetic truth\n" + "".join(synthetic.synthetic_annotation(50_000, contig=4, name="chrS", flank=2000)))
    assert sniff(str(p)) == "table"


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_host_rows_of_the_golden_listing_equal_the_golden_table():
    from deepgrp_amd.annotation import read_rows
    from deepgrp_amd.evaluation import read_annotation
    got = read_rows(LISTING, device=False)
    want = read_annotation(TABLE, None)
    assert got.route == "host" and sum(len(v) for v in want.values()) == 658
    _same(got, want)
    # the lines are those of the listing
    text = gzip.open(LISTING, "rt").read().split("\n")
    for ctg, rows in got.items():
        for row, ln in list(zip(rows, got.lines[ctg]))[:40]:
            tok = text[int(ln) - 1].split()
            assert tok[4] == ctg and int(tok[5]) - 1 == row["start"] and int(tok[6]) == row["end"]
    # a table through read_rows is read_annotation itself
    _same(read_rows(TABLE), want)
    _same(read_rows(LISTING, fmt="repeatmasker", device=False), want)


@pytest.mark.parametrize("name,data", rm_cases.small_cases() + rm_cases.contig_cases() + rm_cases.fallback_cases(),
                         ids=lambda x: x if isinstance(x, str) else "")
def test_host_path_equals_the_table_route(tmp_path, name, data):
    """Listing -> parse_rm's table -> read_annotation(None) against read_rows(device=False), lines included."""
    from deepgrp_amd._scripts import parse_rm
    from deepgrp_amd.annotation import read_rows
    from deepgrp_amd.evaluation import read_annotation
    p, t = tmp_path / "l.out", tmp_path / "l.bed"
    p.write_bytes(data)
    parse_rm.main([str(p), "-o", str(t)])
    got = read_rows(str(p), fmt="repeatmasker", device=False)
    _same(got, read_annotation(str(t), None))
    want = rm_cases.grouped(rm_cases.port_rows(data))
    assert {k: [int(x) for x in v] for k, v in got.lines.items()} == {k: [r[3] for r in v] for k, v in want.items()}


def test_evaluation_rows_checks_and_filters_like_read_annotation(tmp_path):
    from deepgrp_amd._scripts import parse_rm
    from deepgrp_amd.annotation import evaluation_rows
    from deepgrp_amd.evaluation import AnnotationError, read_annotation
    p, t = tmp_path / "l.out", tmp_path / "l.bed"
    for repeats in (None, [1, 3], [4], [9, 10]):
        _same(evaluation_rows(LISTING, repeats, device=False), read_annotation(TABLE, repeats))
    for name, why in (("begin_zero", "negative begin"), ("end_below_begin", "end below begin")):
        data = rm_cases.HEADER.encode() + dict(rm_cases.value_cases())[name]
        p.write_bytes(data)
        parse_rm.main([str(p), "-o", str(t)])
        with pytest.raises(AnnotationError, match=why):
            read_annotation(str(t), [5])                                     # (checked before the filter)
        with pytest.raises(AnnotationError) as err:
            evaluation_rows(str(p), [5], device=False)
        bad = 5 if name == "begin_zero" else 4
        line = data.decode().split("\n")[bad - 1]
        assert str(err.value) == f"{p}:{bad}: {why}: {line.rstrip()!r}"


def test_truth_rows_follow_read_truth_rows(tmp_path):
    from deepgrp_amd._scripts import parse_rm
    from deepgrp_amd.annotation import read_listing
    from deepgrp_amd.training import read_truth_rows
    p, t = tmp_path / "l.out", tmp_path / "l.bed"
    lines = [rm_cases.out_line(ctg=c, begin=b, end=e, fam=f) for c, b, e, f in (
        ("chr1", 11, 50, "SINE/Alu"), ("chr2", 5, 9, "LINE/L1"), ("chr1", 60, 60, "HSATII"), ("chr1", 70, 69, "HSATII"),
        ("chr1", 80, 79, "HSATII"), ("chr3", 1, 5, "LTR/Gypsy"), ("chr1", 100, 120, "LTR/Gypsy"), ("chr1", 7, 8, "HSATII"))]
    p.write_text(rm_cases.HEADER + "\n".join(lines) + "\n")
    parse_rm.main([str(p), "-o", str(t)])
    listing = read_listing(str(p), device=False)
    for names, rts in ((["chr1", "chr2"], [1, 2, 3, 4]), (["chr2", "chrNone"], [4, 3, 2, 1]), (["chr1"], [1])):
        _same(listing.truth_rows(names, rts), read_truth_rows(str(t), names, rts))
    # a kept number without a truth row, and a negative coordinate: the listing's line is named
    with pytest.raises(ValueError, match=re.escape(f"{t}:7: repeat number 10 has no row")):
        read_truth_rows(str(t), ["chr1"], [1, 10])
    with pytest.raises(ValueError, match=re.escape(f"{p}:10: repeat number 10 has no row in a truth of 3 classes")):
        listing.truth_rows(["chr1"], [1, 10])
    p.write_text(rm_cases.out_line(begin=0, end=5) + "\n")
    with pytest.raises(ValueError, match=re.escape(f"{p}:1: negative coordinate: ")):
        read_listing(str(p), device=False).truth_rows(["chr1"], [1, 2, 3])


def test_tables_state_the_ports_numbering():
    from deepgrp_amd._scripts import parse_rm
    from deepgrp_amd.annotation import tables
    blob, off, pent, unit = tables()
    names = [bytes(blob[off[k]:off[k + 1]]).decode() for k in range(len(off) - 1)]
    assert names == list(parse_rm.REPEATS) and unit == parse_rm.NUMBER["HSATII"] == 1
    exact, one_off = parse_rm.pentamer_sets()
    assert len(exact) == 10 and len(one_off) == 150 and not set(exact) & set(one_off)
    assert pent.shape == (1024,) and int((pent == 1).sum()) == 10 and int((pent == 2).sum()) == 150
    for code in range(1024):
        word = "".join("ACGT"[(code >> (2 * (4 - k))) & 3] for k in range(5))
        assert pent[code] == (1 if word in exact else 2 if word in one_off else 0)


def test_the_flag_parses_on_all_three_commands():
    from deepgrp_amd.__main__ import CommandLineParser
    parse = lambda argv: CommandLineParser().parse_args(argv).args
    assert parse(["evaluate", "m.h5", "a.out.gz", "x.fa"]).annotation_format == "auto"
    assert parse(["evaluate", "m.h5", "a.out.gz", "x.fa", "--annotation_format", "repeatmasker"]).annotation_format == "repeatmasker"
    assert parse(["train", "p.toml", "t.fa", "v.fa", "a.out", "--annotation_format", "table"]).annotation_format == "table"
    assert parse(["train", "p.toml", "t.fa", "v.fa", "a.out"]).annotation_format == "auto"
    assert parse(["optimize", "s.toml", "p.toml", "t.npz", "v.npz", "a.bed", "--annotation_format", "repeatmasker"]).annotation_format == "repeatmasker"
    with pytest.raises(SystemExit):
        parse(["evaluate", "m.h5", "a.out.gz", "x.fa", "--annotation_format", "gff"])


def test_symbols_are_declared_exported_and_bound():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    L = _lib.lib()
    for name in ("dgrp_rm_parse_workspace_bytes", "dgrp_rm_parse"):
        assert re.search(r"\b" + name + r"\(", header) and name in _lib.exported_symbols() and hasattr(L, name)
    from deepgrp_amd import annotation
    assert int(re.search(r"#define DGRP_RM_TILE_BYTES (\d+)", header).group(1)) == annotation.TILE_BYTES


def _args(text=P, n=1000, names=P, name_off=P, nnames=10, pent=P, unit=1, outs=P, cap=100, counts="own", work=P, work_bytes=1 << 40):
    counts = (C.c_int64 * 4)(7, 7, 7, 7) if counts == "own" else counts
    return (text, n, names, name_off, nnames, pent, unit, outs, outs, outs, outs, outs, outs, outs, cap, counts, work, work_bytes, None), counts


@pytest.mark.parametrize("kw,code,word", [
    (dict(text=None), EINVAL, "NULL text"), (dict(n=-1), EINVAL, "negative size"), (dict(names=None), EINVAL, "NULL table"),
    (dict(name_off=None), EINVAL, "NULL table"), (dict(pent=None), EINVAL, "NULL table"), (dict(counts=None), EINVAL, "NULL counts"),
    (dict(outs=None), EINVAL, "NULL output"), (dict(cap=-1), EINVAL, "negative capacity"), (dict(nnames=0), EINVAL, "names"),
    (dict(work=None), EINVAL, "workspace"), (dict(work=P + 8), EINVAL, "aligned"), (dict(work_bytes=1000), ENOMEM, "workspace too small"),
])
def test_the_entry_refuses_before_any_device_call(kw, code, word):
    from deepgrp_amd._lib import lib
    L = lib()
    args, counts = _args(**kw)
    assert L.dgrp_rm_parse(*args) == code
    assert word in L.dgrp_last_error().decode()
    if counts is not None:
        assert list(counts) == [0, 0, 0, 0]


def test_the_workspace_query_and_an_empty_text():
    from deepgrp_amd._lib import lib
    L = lib()
    assert L.dgrp_rm_parse_workspace_bytes(-1) == 0
    sizes = [L.dgrp_rm_parse_workspace_bytes(n) for n in (0, 1, 32768, 32769, 10**6, 10**9)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] < 10**9                                                 # well below the text itself
    args, counts = _args(text=None, n=0, work=None, work_bytes=0)
    assert L.dgrp_rm_parse(*args) == 0 and list(counts) == [0, 0, 0, 0]


def _npz_side(tmp_path):
    np.savez(tmp_path / "chrA.fa.gz.npz", fwd=np.eye(5, dtype=np.int8)[:, np.arange(400) % 5])
    toml = tmp_path / "p.toml"
    toml.write_text("units = 4\nvecsize = 20\nbatch_size = 8\nn_batches = 2\nn_epochs = 1\n")
    listing = tmp_path / "rm.out"
    listing.write_text(rm_cases.HEADER + rm_cases.out_line(ctg="chrA", begin=5, end=90) + "\n")
    return str(toml), str(tmp_path / "chrA.fa.gz.npz"), str(listing)


def test_train_on_npz_sides_refuses_a_listing_by_name(tmp_path):
    from deepgrp_amd.__main__ import main
    toml, npz, listing = _npz_side(tmp_path)
    model = tmp_path / "model.hdf5"
    for extra in ([], ["--annotation_format", "repeatmasker"]):
        with pytest.raises(SystemExit) as err:
            main(["train", toml, npz, npz, listing, "--logdir", str(tmp_path / "log"), "--modelfile", str(model)] + extra)
        msg = str(err.value.code)
        assert err.value.code not in (0, None) and "parse_rm" in msg and listing in msg and "sequence files" in msg
    assert not model.exists() and not (tmp_path / "log").exists()


def test_optimize_refuses_a_listing_by_name(tmp_path):
    from deepgrp_amd.__main__ import main
    toml, npz, listing = _npz_side(tmp_path)
    space = tmp_path / "s.toml"
    space.write_text('[space]\ngru_units = ["qnormal", 34, 5, 2]\n')
    with pytest.raises(SystemExit) as err:
        main(["optimize", str(space), toml, npz, npz, listing, "--project_root_dir", str(tmp_path / "root")])
    assert "parse_rm" in str(err.value.code) and listing in str(err.value.code) and not (tmp_path / "root").exists()
