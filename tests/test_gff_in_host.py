"""Reading GFF3 without a GPU: the host statement of the grammar (gffin.features_host) on the corpus against hand-written
expectations; the %XX rule; the sniffer; the names flag; every refusal of the command line before the model is read; the two new
symbols; and `predict`'s own GFF3 text (gff.reference_lines) read back to the rows it was written from."""
import gzip
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gff_in_cases import CASES, DEFAULT4, KEY, NAMES4, TILE, UNDECIDED, feature, gff_of_table

from deepgrp_amd import gffin
from deepgrp_amd.evaluation import AnnotationError


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def rows_of_flat(flat):
    """[(line, name, begin, end, number)] of a Flat."""
    names = np.repeat(np.array(flat.run_names, object), np.diff(flat.run_first)).tolist() if len(flat.begin) else []
    return list(zip(flat.line.tolist(), names, flat.begin.tolist(), flat.end.tolist(), flat.number.tolist()))


# ---------------------------------------------------------------- the statement on the corpus
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_statement_on_the_corpus(tmp_path, name):
    case = CASES[name]
    p = _write(tmp_path, "x.gff3", case.text)
    if case.want == UNDECIDED:
        return                                                      # (what the device leaves to the host; its rule is below)
    if case.want[0] == "malformed":
        with pytest.raises(AnnotationError) as e:
            gffin.features_host(p, case.names, case.key)
        assert str(e.value).startswith(f"{p}:{case.want[1]}: {gffin.REASON}: ")
        return
    lines, end_at, rows = case.want
    flat, got_end = gffin.features_of_bytes(p, case.text, case.names, case.key)
    assert (flat.lines, got_end, flat.route, flat.run_files) == (lines, end_at, "host", None)
    assert rows_of_flat(flat) == [(ln, gffin.decode(s).decode(), b, e, n) for ln, s, b, e, n in rows]
    raw = [r[1] for r in rows]
    assert flat.run_first.tolist() == [i for i in range(len(raw)) if i == 0 or raw[i] != raw[i - 1]] + [len(raw)]
    assert gffin.features_host(p, case.names, case.key).begin.tolist() == flat.begin.tolist()


def test_the_corpus_meets_the_edges():
    for n in (0, 1, 127, 128, 129, TILE - 1, TILE, TILE + 1):
        assert len(CASES[f"size {n}"].text) == n
    assert CASES["##FASTA at a chunk edge"].text[384:392] == b"##FASTA\n" and CASES["##FASTA at a tile edge"].text[TILE:TILE + 8] == b"##FASTA\n"
    assert CASES["> at the second tile edge"].text[2 * TILE - 1:2 * TILE + 1] == b"\n>"
    text = CASES["straddles"].text
    for edge, what in zip((384, 896, 1408, TILE, 2 * TILE, 3 * TILE), (b"scaffold_000123", b"123456789", b"Satellite") * 2):
        at = text.rindex(what, 0, edge + len(what))
        assert at < edge < at + len(what), (edge, what)
    lines, _end, rows = CASES["bulk"].want
    assert lines == 4001 and len(rows) > 3800 and len({r[1] for r in rows}) == 4 and len(CASES["bulk"].text) > 8 * TILE
    assert {gffin.decode(r[1]) for r in rows} == {b"chr1", b"chr2", b"chr|3"} and {r[4] for r in rows} == {0, 1, 2, 3, 4}


def test_the_host_route_words_the_rest(tmp_path):
    # what the device does not decide: 19 digits that fit int64 are read, what does not is an error with its line
    p = _write(tmp_path, "a.gff3", feature(start=5, end=b"1" * 19) + b"\n")
    assert gffin.features_host(p, NAMES4, KEY).end.tolist() == [1111111111111111111]
    for tok, what in ((b"9" * 19, "end"), (b"x", "end"), (b"", "end")):
        p = _write(tmp_path, "b.gff3", feature() + b"\n" + feature(start=5, end=tok) + b"\n")
        with pytest.raises(AnnotationError) as e:
            gffin.features_host(p, NAMES4, KEY)
        assert str(e.value).startswith(f"{p}:2: {what} {tok.decode()!r} is not an integer: ")
    # the checks of read_features on the host route: file, line and the line's text
    for case, why in (("start 0", "negative begin"), ("end below begin", "end below begin")):
        p = _write(tmp_path, "c.gff3", b"# one\n" + CASES[case].text)
        with pytest.raises(AnnotationError) as e:
            gffin.read_features(p, NAMES4, KEY, device=False)
        assert str(e.value).startswith(f"{p}:2: {why}: 'chr1\\tdeepgrp")
    assert len(gffin.read_features(_write(tmp_path, "d.gff3", CASES["empty row"].text), NAMES4, KEY, device=False).begin) == 1
    # gzip on the host route, and two spellings of one seqid in one record
    p = tmp_path / "e.gff3.gz"
    with gzip.open(p, "wb") as fh:
        fh.write(CASES["escaped seqid"].text)
    got = gffin.read_annotation(str(p), NAMES4, KEY, [3], device=False)
    assert list(got) == ["chr|3"] and len(got["chr|3"]) == 3 and got.lines["chr|3"].tolist() == [1, 2, 3] and got.route == "host"
    pred = gffin.read_predicted(_write(tmp_path, "f.gff3", CASES["bulk"].text), NAMES4, KEY, 4, device=False)
    numbers = [r[4] for r in CASES["bulk"].want[2]]
    assert pred.format == "gff3" and pred.rows_read == len(numbers) and pred.rows_dropped == sum(1 for x in numbers if not 1 <= x < 4)
    assert sum(len(v) for v in pred.values()) == pred.rows_read - pred.rows_dropped and set(pred) == {"chr1", "chr2", "chr|3"}


def test_decode():
    d = gffin.decode
    assert d(b"") == b"" and d(b"plain") == b"plain" and d(b"a%2Fb") == b"a/b" == d(b"a%2fb") and d(b"%41%6c%75") == b"Alu"
    assert d(b"100%") == b"100%" and d(b"%4") == b"%4" and d(b"%zz") == b"%zz" and d(b"%4g") == b"%4g" and d(b"%g4") == b"%g4"
    assert d(b"%%41") == b"%A" and d(b"%2541") == b"%41" and d(b"%00%ff%FF") == b"\x00\xff\xff" and d(b"x%") == b"x%" and d(b"%2") == b"%2"
    from deepgrp_amd import gff
    every = bytes(range(256))
    assert d(gff.escape_seqid(every)) == every and d(gff.escape_value(every)) == every


# ---------------------------------------------------------------- the sniffer
def test_sniffing(tmp_path):
    from deepgrp_amd import annotation
    from deepgrp_amd.compare import resolve_predicted_format, sniff_predicted
    body = feature() + b"\n"
    with_line = _write(tmp_path, "a.gff3", b"##gff-version 3\n" + body)
    assert annotation.sniff(with_line) == "gff3" == sniff_predicted(with_line) == annotation.resolve_format(with_line, "auto")
    assert annotation.sniff(_write(tmp_path, "v.gff3", b"##gff-version 3.1.26\n" + body)) == "gff3"
    assert annotation.sniff(_write(tmp_path, "h.gff3", b"##gff-version 3\n")) == "gff3"
    without = _write(tmp_path, "b.gff3", body)
    assert annotation.sniff(without) == "table" == sniff_predicted(without)          # as before: the form is explicit there
    assert annotation.sniff(_write(tmp_path, "c.gff3", b"\n##gff-version 3\n" + body)) == "table"      # the FIRST line
    assert annotation.sniff(_write(tmp_path, "d.gff", b"##gff-version 2\n" + body)) == "table"
    assert annotation.resolve_format(without, "gff3") == "gff3" == resolve_predicted_format(without, "gff3")
    p = tmp_path / "z.gff3.gz"
    with gzip.open(p, "wb") as fh:
        fh.write(b"##gff-version 3\n" + body * 50)
    assert annotation.sniff(str(p)) == "gff3" == sniff_predicted(str(p))
    assert "gff3" in annotation.FORMATS and "gff3" in __import__("deepgrp_amd.compare").compare.PREDICTED_FORMATS


def test_every_text_of_the_compare_sniffing_test_gives_what_it_gave(tmp_path):
    import test_compare_host as t
    from deepgrp_amd.compare import sniff_predicted
    params = [m for m in t.test_sniffing.pytestmark if m.name == "parametrize"][0].args[1]
    assert len(params) == 9
    for k, (text, want) in enumerate(params):
        assert sniff_predicted(_write(tmp_path, f"p{k}.txt", text.encode())) == want


# ---------------------------------------------------------------- names
def test_names():
    assert gffin.parse_names(None, 5) == DEFAULT4 == gffin.default_names(5)
    assert gffin.parse_names("LTR|ERV1|ERVK,LINE|L1,Alu,Satellite", 5) == [[b"LTR", b"ERV1", b"ERVK"], [b"LINE", b"L1"], [b"Alu"], [b"Satellite"]]
    for spec, classes, words in (("a,,b", 4, "empty alternative in the entry of label 2"), ("a|,b", 3, "empty alternative in the entry of label 1"),
                                 ("", 2, "empty alternative"), ("a,b", 4, "2 entries for the labels 1..3"), ("a,b|a", 3, "'a' stands under two labels, 1 and 2"),
                                 ("a," + "b" * 256, 3, "256 bytes, above 255"),
                                 (",".join("|".join(f"n{4 * i + j}" for i in range(1025)) for j in range(4)), 5, "4100 alternatives, above 4096")):
        with pytest.raises(ValueError) as e:
            gffin.parse_names(spec, classes, "--x_names")
        assert str(e.value).startswith("--x_names: ") and words in str(e.value)
    assert len(gffin.parse_names("a,b,c", None)) == 3                                    # (evaluate before its model is read)
    blob, off, number, count = gffin.names_table(NAMES4)
    alts = [blob[off[k]:off[k + 1]].tobytes() for k in range(count)]
    assert alts == sorted(a for e in NAMES4 for a in e) and count == 10
    assert [int(number[alts.index(a)]) for a in (b"LTR", b"L1", b"Alu", b"x;y")] == [1, 2, 3, 4]
    assert gffin.names_table([])[3] == 0
    assert gffin.check_key(None, False) == b"Name" and gffin.check_key("class", False) == b"class" and gffin.check_key(None, True) is None
    for key, by_type in (("Name", True), ("", False), ("a=b", False), ("k" * 256, False)):
        with pytest.raises(ValueError):
            gffin.check_key(key, by_type)


# ---------------------------------------------------------------- refusals before anything is read
@pytest.fixture
def no_model(monkeypatch):
    from deepgrp_amd import model as dgmodel

    def read(*_a, **_k):
        raise AssertionError("the model was read before the refusal")
    monkeypatch.setattr(dgmodel, "load_model", read)
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", read)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _refused(argv, message):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert isinstance(e.value.code, str) and message in e.value.code, e.value.code


def test_cli_refusals(no_model, tmp_path):
    missing = [str(tmp_path / "no.gff3"), str(tmp_path / "no.bed"), str(tmp_path / "no.fa")]     # nothing exists: nothing can be read
    cmp_ = ["compare"] + missing
    ev = ["evaluate", "no_model.h5"] + missing[1:]
    for base, flag in ((cmp_, "--predicted_names"), (cmp_, "--annotation_names"), (ev, "--annotation_names")):
        fmt = flag.replace("names", "format")
        _refused(base + [fmt, "gff3", flag, "a,,b"], f"{flag}: an empty alternative in the entry of label 2")
        _refused(base + [fmt, "gff3", flag, "a," + "b" * 256], f"{flag}: an alternative of label 2 has 256 bytes, above 255")
        _refused(base + [fmt, "gff3", flag, "a|b,c|a"], f"{flag}: the alternative 'a' stands under two labels, 1 and 2")
        _refused(base + [fmt, "gff3", flag, ",".join("|".join(f"n{4 * i + j}" for i in range(1025)) for j in range(4))], "4100 alternatives, above 4096")
        _refused(base + [fmt, "table", flag, "a,b,c,d"], f"{flag} names the labels of a GFF3 file: {fmt} table has numbers")
        _refused(base + [fmt, "repeatmasker", flag, "a,b,c,d"], f"{flag} names the labels of a GFF3 file")
        _refused(base + ["--gff_by_type", "--gff_key", "Name"], "--gff_by_type takes the label from column 3: it excludes --gff_key")
        _refused(base + ["--gff_key", ""], "--gff_key: a tag of 1..255 bytes")
    _refused(cmp_ + ["--predicted_format", "tsv", "--predicted_names", "a,b,c,d"], "--predicted_format tsv has numbers")
    # the number of entries: compare knows its classes from the flag, evaluate from the model (checked right behind it)
    _refused(cmp_ + ["--predicted_format", "gff3", "--predicted_names", "a,b,c"], "--predicted_names: 3 entries for the labels 1..4")
    _refused(cmp_ + ["--classes", "3", "--annotation_format", "gff3", "--annotation_names", "a,b,c"], "--annotation_names: 3 entries for the labels 1..2")
    assert os.listdir(tmp_path) == []


def test_names_flag_with_auto_is_refused_once_the_file_is_sniffed(no_model, tmp_path):
    table = _write(tmp_path, "a.bed", b"chr1 1 5 1\n")
    _refused(["evaluate", "no_model.h5", table, str(tmp_path / "no.fa"), "--annotation_names", "a,b,c,d"],
             "--annotation_names names the labels of a GFF3 file: --annotation_format auto found table")
    _refused(["compare", table, table, str(tmp_path / "no.fa"), "--predicted_names", "a,b,c,d"], "--predicted_format auto found table")
    gff3 = _write(tmp_path, "a.gff3", b"##gff-version 3\n" + feature() + b"\n")
    _refused(["evaluate", "no_model.h5", gff3, str(tmp_path / "no.fa"), "--offtarget", str(tmp_path / "o")],
             "holds the rows of the modelled classes only")
    _refused(["compare", gff3, gff3, str(tmp_path / "no.fa"), "--offtarget", str(tmp_path / "o")], "holds the rows of the modelled classes only")


def test_the_entry_count_is_checked_behind_the_model(monkeypatch, tmp_path):
    from deepgrp_amd import model as dgmodel
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", lambda *a, **k: {"ff_kernel": np.zeros((16, 5), np.float32)})
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **k: pytest.fail("the device model was made before the refusal"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gff3 = _write(tmp_path, "a.gff3", b"##gff-version 3\n" + feature() + b"\n")
    _refused(["evaluate", "m.h5", gff3, str(tmp_path / "no.fa"), "--annotation_names", "a,b,c"], "--annotation_names: 3 entries for the labels 1..4")


def test_optimize_refuses_gff3_by_name(no_model, tmp_path):
    files = {k: _write(tmp_path, k, b"x = 1\n") for k in ("p.toml", "t.fa", "v.fa", "space.toml")}
    gff3 = _write(tmp_path, "a.gff3", b"##gff-version 3\n" + feature() + b"\n")
    plain = _write(tmp_path, "b.gff3", feature() + b"\n")
    for bed, flags in ((gff3, []), (plain, ["--annotation_format", "gff3"])):
        _refused(["optimize", files["space.toml"], files["p.toml"], files["t.fa"], files["v.fa"], bed] + flags, f"optimize: {bed} is GFF3")


# ---------------------------------------------------------------- the symbols
def test_the_two_symbols_are_exported_and_declared():
    from deepgrp_amd._lib import _SIGNATURES, exported_symbols
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for sym in ("dgrp_gff_parse", "dgrp_gff_parse_workspace_bytes"):
        assert sym in exported_symbols() and sym in _SIGNATURES
        assert re.search(r"^int(64_t)? %s\(" % sym, header, re.M)
    assert len(_SIGNATURES["dgrp_gff_parse"][1]) == 20
    src = open(os.path.join(ROOT, "deepgrp_amd", "csrc", "gff_parse_kernels.hip")).read()
    make = open(os.path.join(ROOT, "deepgrp_amd", "csrc", "Makefile")).read()
    assert src.count("DGRP_EXPORT") == 2 and "gff_parse_kernels.o" in make and "gff_line.h" in make
    assert "#define DGRP_ABI_VERSION 1\n" in header
    assert gffin.MIN_LINE_BYTES == int(re.search(r"#define GFF_MIN_LINE (\d+)", open(os.path.join(ROOT, "deepgrp_amd", "csrc", "gff_line.h")).read()).group(1))


# ---------------------------------------------------------------- predict's own text read back
def _written(class_names):
    from deepgrp_amd import gff
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE
    one = 1 << 24
    spans = [(99, 350, 3, 0), (1000, 1010, 1, 0), (2000, 2500, 4, 0), (0, 5, 4, 1), (7, 9, 2, 1), (40, 90, 1, 2)]
    rows = np.zeros(len(spans), SEGMENT_DTYPE)
    for i, r in enumerate(spans):
        rows[i] = r
    sc = np.zeros(len(spans), ROW_SCORE_DTYPE)
    for i, (a, e, _l, _c) in enumerate(spans):
        sc[i] = (int(0.9 * one) * (e - a), e - a, e - a, one // 2, 0)
    record_names = [b"chr1", "scaf;x=1", b"chr 3|a"]
    text, lines = gff.reference_lines(record_names, True, rows, sc, 0, class_names, 0)
    assert lines == len(spans)
    return gff.HEADER + text, spans, ["chr1", "scaf;x=1", "chr 3|a"]


@pytest.mark.parametrize("class_names", [None, [b"HSATII", b"(GAATG)n;x", b"SINE/Alu, old=1", b"100% sat&co"]], ids=("default", "escaped"))
def test_predicts_own_text_reads_back(tmp_path, class_names):
    text, spans, record_names = _written(class_names)
    names = gffin.default_names(5) if class_names is None else [[n] for n in class_names]
    if class_names is not None:
        assert b"%3B" in text and b"%2C" in text and b"%25" in text and b"%26" in text and b"scaf%3Bx%3D1" in text
    got = gffin.read_predicted(_write(tmp_path, "x.fa.gff3", text), names, KEY, 5, device=False)
    assert got.rows_read == len(spans) and got.rows_dropped == 0 and sorted(got) == sorted(record_names)
    for c, name in enumerate(record_names):
        assert got[name][["start", "end", "label"]].tolist() == [(a, e, l) for a, e, l, cc in spans if cc == c]
    # the label attribute carries the number itself: the key `label` with the numbers as names reads the same rows
    by_label = gffin.read_predicted(_write(tmp_path, "y.gff3", text), [[b"%d" % k] for k in range(1, 5)], b"label", 5, device=False)
    assert {k: v.tolist() for k, v in by_label.items()} == {k: v.tolist() for k, v in got.items()}
    # by type: every row is a repeat_region
    typed = gffin.read_predicted(_write(tmp_path, "z.gff3", text), [[b"repeat_region"]], None, 2, device=False)
    assert typed.rows_read == len(spans) and all((v["label"] == 1).all() for v in typed.values())


def test_gff_of_table_round_trip(tmp_path):
    rows = [("chr1", 5, 9, 2), ("chr1", 20, 30, 1), ("chr2", 0, 4, 4)]
    p = _write(tmp_path, "t.gff3", gff_of_table(rows, NAMES4))
    got = gffin.read_annotation(p, NAMES4, KEY, [1, 2], device=False)
    assert list(got) == ["chr1"] and got["chr1"][["start", "end", "label"]].tolist() == [(5, 9, 2), (20, 30, 1)]
