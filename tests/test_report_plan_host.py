"""The refusals the four reports of `evaluate` share (outfiles.plan_prefix, reached through each module's `plan`), character for
character: a prefix that is a directory, WORLD_SIZE > 1, a directory that does not exist, an output that is an input -- and the two
things --curves does not refuse."""
import argparse
import os

import pytest

import rm_cases

HISTOGRAMS = "the histograms are summed on the rank that holds the merged probabilities"
COUNTS = "the counts are summed on the rank that holds the predicted rows"
# module, flag, the sentence behind "WORLD_SIZE > 1 is not supported:", the suffixes of its files
REPORTS = [("curves", "--curves", HISTOGRAMS, (".bases.tsv", ".rows.tsv")),
           ("strata", "--strata", HISTOGRAMS, (".strata.tsv", ".strata.bases.tsv")),
           ("offtarget", "--offtarget", COUNTS, (".offtarget.tsv", ".offtarget.rows.tsv")),
           ("boundaries", "--boundaries", COUNTS, (".boundaries.tsv", ".fragments.tsv"))]


def _plan(name, tmp_path, prefix, fasta=None, annotation=None, model=None):
    import importlib
    module = importlib.import_module("deepgrp_amd." + name)
    if annotation is None:
        annotation = tmp_path / "rm.out"
        annotation.write_bytes(rm_cases.text([rm_cases.out_line()]))
    args = argparse.Namespace(FASTA=[str(fasta or tmp_path / "x.fa")], annotation=str(annotation), model=str(model or tmp_path / "m.h5"),
                              annotation_format="auto", **{name: prefix})
    return module.plan(args)


def _said(*a, **k):
    with pytest.raises(SystemExit) as e:
        _plan(*a, **k)
    return str(e.value)


@pytest.mark.parametrize("name,flag,why,suffixes", REPORTS)
def test_the_four_refusals_word_for_word(monkeypatch, tmp_path, name, flag, why, suffixes):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for prefix in ("", "sub" + os.sep):
        assert _said(name, tmp_path, prefix) == f"{flag} takes a file name prefix, not the directory {prefix!r}"
    assert _said(name, tmp_path, "missing_dir/run") == f"{flag}: the directory missing_dir does not exist"
    assert _said(name, tmp_path, str(tmp_path / "no" / "run")) == f"{flag}: the directory {tmp_path / 'no'} does not exist"
    for suffix in suffixes:                              # a FASTA input that is one of the outputs, under another name too
        fasta = tmp_path / ("in" + suffix)
        fasta.write_text(">a\nACGT\n")
        assert _said(name, tmp_path, "in", fasta=fasta) == f"{flag}: the file in{suffix} would overwrite the input {fasta}"
        os.symlink(str(fasta), str(tmp_path / ("link" + suffix)))
        assert _said(name, tmp_path, "link", fasta=fasta) == f"{flag}: the file link{suffix} would overwrite the input {fasta}"
    assert _plan(name, tmp_path, "run", fasta="-").prefix == "run"           # standard input is no file to overwrite
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert _said(name, tmp_path, "run") == f"{flag} runs in one process (WORLD_SIZE > 1 is not supported: {why})"
    assert _said(name, tmp_path, "sub" + os.sep).startswith(f"{flag} takes a file name prefix")      # the prefix is looked at first
    assert "WORLD_SIZE" in _said(name, tmp_path, "missing_dir/run")                                   # and the directory last
    assert sorted(p.name for p in tmp_path.iterdir() if not p.name.startswith(("in.", "link."))) == ["rm.out"]


@pytest.mark.parametrize("name,flag,why,suffixes", REPORTS)
def test_curves_alone_takes_a_directory_name_and_guards_only_the_fasta(monkeypatch, tmp_path, name, flag, why, suffixes):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "sub").mkdir()
    listing = tmp_path / ("a" + suffixes[0])             # the annotation and the model under the names of the outputs
    listing.write_bytes(rm_cases.text([rm_cases.out_line()]))
    model = tmp_path / ("m" + suffixes[1])
    model.write_bytes(b"\x89HDF")
    if name == "curves":
        p = _plan(name, tmp_path, "sub")
        assert p.prefix == "sub" and p.bases_path == "sub.bases.tsv" and p.rows_path == "sub.rows.tsv"
        assert _plan(name, tmp_path, "a", annotation=listing).bases_path == "a.bases.tsv"
        assert _plan(name, tmp_path, "m", model=model).rows_path == "m.rows.tsv"
    else:
        assert _said(name, tmp_path, "sub") == f"{flag} takes a file name prefix, not the directory 'sub'"
        assert _said(name, tmp_path, "a", annotation=listing) == f"{flag}: the file a{suffixes[0]} would overwrite the input {listing}"
        assert _said(name, tmp_path, "m", model=model) == f"{flag}: the file m{suffixes[1]} would overwrite the input {model}"
