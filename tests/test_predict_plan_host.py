"""The refusals of `predict`'s five outputs (--mask_dir, --track_dir, --bed_dir, --seq_dir, --summary_dir), character for character:
what each plan refuses before the model file is opened, driven through `main` so that the test does not depend on where the code
lives; the `belongs to predict, not evaluate` lines of `evaluate`; and the five refusals that need the model's class count, through
each module's `from_plan`.  No GPU, and the model file `m.h5` never exists."""
import argparse
import gzip
import os

import pytest

SEVERAL = "(WORLD_SIZE > 1, --split_contigs)"


def _said(argv):
    from deepgrp_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main([str(a) for a in argv])
    return str(e.value)


@pytest.fixture
def files(tmp_path, monkeypatch):
    """in/x.fa and other/x.fa (one basename, two directories), the output directory `out` (not made) and `held`, an output
    directory that exists."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for sub in ("in", "other", "held"):
        (tmp_path / sub).mkdir()
    fa, other = tmp_path / "in" / "x.fa", tmp_path / "other" / "x.fa"
    fa.write_bytes(b">a\nACGT\n")
    other.write_bytes(b">b\nAC\n")
    return argparse.Namespace(fa=str(fa), other=str(other), out=str(tmp_path / "out"), held=str(tmp_path / "held"), root=tmp_path)


def _predict(files, *rest, inputs=None):
    return _said(["predict", "m.h5"] + list(inputs if inputs is not None else [files.fa]) + list(rest))


def _linked(files, name):
    """held/<name>, a symbolic link to the input: the output of that name is the input."""
    link = os.path.join(files.held, name)
    os.symlink(files.fa, link)
    return link


def _several(files, monkeypatch, want, *flags):
    """The same words for WORLD_SIZE=2 and for --split_contigs."""
    assert _predict(files, *flags, "--split_contigs") == want
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert _predict(files, *flags) == want
    monkeypatch.delenv("WORLD_SIZE")


def test_mask_dir(files, monkeypatch):
    d = ("--mask_dir", files.out)
    assert _predict(files, "--mask_twobit") == "--mask_twobit needs --mask_dir"
    for flag in (("--mask", "hard"), ("--mask_classes", "1,3"), ("--mask_gzip",)):
        assert _predict(files, *flag) == "--mask, --mask_classes and --mask_gzip need --mask_dir"
    assert _said(["--mask_gzip", "m.h5", files.fa]) == "--mask, --mask_classes and --mask_gzip need --mask_dir"      # the README form
    assert _predict(files, *d, "--mask_twobit", "--mask_gzip") == ("--mask_twobit and --mask_gzip exclude each other: a 2bit file is a binary "
                                                                   "format of its own and is not compressed")
    _several(files, monkeypatch, "--mask_gzip: a compressed masked copy cannot be written by several ranks " + SEVERAL + ": they share a file "
             "out by byte ranges, and a compressed file has none; run in one process", *d, "--mask_gzip")
    _several(files, monkeypatch, "--mask_twobit: a 2bit masked copy cannot be written by several ranks " + SEVERAL + ": they share a file out "
             "by byte ranges, and a 2bit file has none of the input's; run in one process", *d, "--mask_twobit")
    assert _predict(files, *d, inputs=["-"]) == "--mask_dir: standard input cannot be masked (give a FASTA file)"
    assert _predict(files, *d, inputs=["y.gz.npz"]) == "--mask_dir: y.gz.npz is a one-hot .npz, not a FASTA file; it cannot be masked"
    packed = files.root / "in" / "p.fa.gz"
    packed.write_bytes(gzip.compress(b">a\nACGT\n"))
    assert _predict(files, *d, inputs=[packed]) == (f"--mask_dir: {packed} is gzip-compressed; the masked copy is written by byte offsets of "
                                                   "the input, so give the uncompressed FASTA or pass --mask_gzip")
    assert _predict(files, *d, inputs=[files.fa, files.other]) == (f"--mask_dir: the masked copies of {files.fa} and {files.other} have the "
                                                                  "same file name x.fa; they would collide")
    assert _predict(files, *d, "--mask_gzip", inputs=[files.fa, files.other]) == (
        f"--mask_dir: the masked copies of {files.fa} and {files.other} have the same file name x.fa.gz; they would collide")
    assert _predict(files, *d, inputs=[files.fa, files.fa]) == "--mask_dir: an input file is given twice"
    assert not os.path.exists(files.out)
    link = _linked(files, "x.fa")
    assert _predict(files, "--mask_dir", files.held) == f"--mask_dir: the masked copy {link} would overwrite the input {files.fa}"
    assert _predict(files, "--mask_dir", os.path.dirname(files.fa)) == f"--mask_dir: the masked copy {files.fa} would overwrite the input {files.fa}"


def test_seq_dir(files, monkeypatch):
    d = ("--seq_dir", files.out)
    for flag in (("--seq_classes", "1"), ("--seq_flank", "5"), ("--seq_width", "70"), ("--seq_gzip",), ("--seq_fai",)):
        assert _predict(files, *flag) == "--seq_classes, --seq_flank, --seq_width, --seq_gzip and --seq_fai need --seq_dir"
    assert _predict(files, *d, "--seq_fai", "--seq_gzip") == ("--seq_fai and --seq_gzip exclude each other: a .fai states offsets of the "
                                                              "uncompressed file, a BGZF FASTA would also need a .gzi index, which is not written")
    _several(files, monkeypatch, "--seq_dir: the repeat sequences of an input are written by one process, in TSV order; they cannot be written "
             "by several ranks " + SEVERAL + "; run in one process", *d)
    assert _predict(files, *d, "--seq_width", "0") == "--seq_width must lie in 1..2^30, not 0"
    assert _predict(files, *d, "--seq_width", str((1 << 30) + 1)) == f"--seq_width must lie in 1..2^30, not {(1 << 30) + 1}"
    assert _predict(files, *d, "--seq_flank", "-1") == "--seq_flank must not be negative, got -1"
    assert _predict(files, *d, inputs=["-"]) == "--seq_dir: standard input cannot be read a second time for the sequences (give a FASTA file)"
    assert _predict(files, *d, inputs=["y.gz.npz"]) == ("--seq_dir: y.gz.npz is a one-hot .npz, not a FASTA file; it holds no sequence bytes "
                                                        "to write")
    assert _predict(files, *d, inputs=[files.fa, files.other]) == (f"--seq_dir: the repeat sequences of {files.fa} and {files.other} have the "
                                                                  "same file name x.fa.repeats.fa; they would collide")
    assert _predict(files, *d, "--seq_gzip", inputs=[files.fa, files.other]) == (
        f"--seq_dir: the repeat sequences of {files.fa} and {files.other} have the same file name x.fa.repeats.fa.gz; they would collide")
    assert _predict(files, *d, inputs=[files.fa, files.fa]) == "--seq_dir: an input file is given twice"
    assert not os.path.exists(files.out)
    link = _linked(files, "x.fa.repeats.fa.fai")
    assert _predict(files, "--seq_dir", files.held, "--seq_fai") == f"--seq_dir: the output {link} would overwrite the input {files.fa}"
    link = _linked(files, "x.fa.repeats.fa")
    assert _predict(files, "--seq_dir", files.held) == f"--seq_dir: the output {link} would overwrite the input {files.fa}"
    # every input is looked at, not only the output's own
    assert _predict(files, "--seq_dir", files.held, inputs=[files.other, files.fa]) == f"--seq_dir: the output {link} would overwrite the input {files.fa}"


def test_summary_dir(files, monkeypatch):
    d = ("--summary_dir", files.out)
    assert _predict(files, "--summary_bin", "100") == "--summary_bin needs --summary_dir"
    assert _predict(files, *d, "--summary_bin", "0") == "--summary_bin must be at least 1, not 0"
    _several(files, monkeypatch, "--summary_dir: the repeat content of an input is counted by one process, from all of its rows; it cannot be "
             "counted by several ranks " + SEVERAL + "; run in one process", *d)
    assert _predict(files, *d, "--bed_names", "LINE,,SINE") == "--bed_names: the name of label 2 is empty"
    assert _predict(files, *d, "--bed_names", "LINE,S\tINE") == ("--bed_names: the name of label 2 holds a tab, a line end or another control "
                                                                "character, which the tab-separated files of --summary_dir cannot hold")
    assert _predict(files, *d, inputs=["-"]) == "--summary_dir: standard input cannot be read a second time for the counts (give a FASTA file)"
    assert _predict(files, *d, inputs=["y.gz.npz"]) == ("--summary_dir: y.gz.npz is a one-hot .npz, not a FASTA file; it holds no sequence "
                                                        "bytes to count")
    assert _predict(files, *d, inputs=[files.fa, files.other]) == (f"--summary_dir: the summaries of {files.fa} and {files.other} have the same "
                                                                  "file name x.fa.summary.tsv; they would collide")
    assert _predict(files, *d, inputs=[files.fa, files.fa]) == "--summary_dir: an input file is given twice"
    assert not os.path.exists(files.out)
    link = _linked(files, "x.fa.density.tsv")
    assert _predict(files, "--summary_dir", files.held, "--summary_bin", "9") == f"--summary_dir: the output {link} would overwrite the input {files.fa}"
    link = _linked(files, "x.fa.summary.tsv")
    assert _predict(files, "--summary_dir", files.held) == f"--summary_dir: the output {link} would overwrite the input {files.fa}"
    assert _predict(files, "--summary_dir", files.held, inputs=[files.other, files.fa]) == (
        f"--summary_dir: the output {link} would overwrite the input {files.fa}")


def test_bed_dir(files, monkeypatch):
    d = ("--bed_dir", files.out)
    assert _predict(files, "--bed_gff3") == "--bed_gff3 needs --bed_dir"
    assert _predict(files, *d, "--bed_gff3", "--bed_bigbed") == ("--bed_gff3 and --bed_bigbed each write their file instead of the BED text: "
                                                                 "they do not go together")
    assert _predict(files, *d, "--bed_names", "a,b") == "--bed_names needs --bed_gff3"
    assert _predict(files, *d, "--bed_gff3", "--bed_names", "a,,b") == "--bed_names: the name of label 2 is empty"
    assert _predict(files, *d, "--bed_gff3", "--bed_names", "a," + "b" * 256) == "--bed_names: the name of label 2 has 256 bytes, above 255"
    assert _predict(files, "--bed_bigbed") == "--bed_bigbed needs --bed_dir"
    for flag in ("--bed_gzip", "--bed_index"):
        assert _predict(files, *d, "--bed_bigbed", "--bed_gzip", flag) == ("--bed_bigbed writes a bigBed file instead of BED text: it does not "
                                                                           "go with --bed_gzip or --bed_index")
    assert _predict(files, "--bed_gzip") == "--bed_gzip needs --bed_dir"
    assert _predict(files, *d, "--bed_index") == "--bed_index needs --bed_gzip"
    assert _predict(files, "--bed_min_score", "5") == "--bed_min_score needs --bed_dir"
    assert _predict(files, *d, "--bed_min_score", "1001") == "--bed_min_score must lie in 0..1000, not 1001"
    assert _predict(files, *d, "--bed_min_score", "-1") == "--bed_min_score must lie in 0..1000, not -1"
    want = ("--bed_dir runs in one process (WORLD_SIZE > 1 and --split_contigs are not supported: the scores are summed on the rank that "
            "holds the merged probabilities)")
    _several(files, monkeypatch, want, *d)
    for flags, name in (((), "x.fa.bed"), (("--bed_gzip",), "x.fa.bed.gz"), (("--bed_bigbed",), "x.fa.bb"), (("--bed_gff3",), "x.fa.gff3")):
        assert _predict(files, *d, *flags, inputs=[files.fa, files.other]) == (
            f"--bed_dir: the BED files of {files.fa} and {files.other} have the same file name {name}; they would collide")
    assert _predict(files, *d, inputs=[files.fa, files.fa]) == "--bed_dir: an input file is given twice"
    assert _predict(files, *d, inputs=["-", "-"]) == "--bed_dir: an input file is given twice"      # standard input is an input here
    link = _linked(files, "x.fa.bed")
    assert _predict(files, "--bed_dir", files.held) == f"--bed_dir: the BED file {link} would overwrite the input {files.fa}"
    assert not os.path.exists(files.out)


def test_track_dir(files, monkeypatch):
    d = ("--track_dir", files.out)
    assert _predict(files, "--track_gzip") == "--track_gzip needs --track_dir"
    assert _predict(files, "--track_bigwig") == "--track_bigwig needs --track_dir"
    assert _predict(files, *d, "--track_bigwig", "--track_gzip") == ("--track_bigwig writes bigWig files instead of bedGraph: it does not go "
                                                                     "with --track_gzip or --track_index")
    assert _predict(files, *d, "--track_index") == "--track_index needs --track_gzip (a tabix index belongs to a BGZF file)"
    assert _predict(files, *d, "--gzip_level", "1") == "--gzip_level needs --mask_gzip or --track_gzip or --bed_gzip"
    assert _predict(files, *d, "--track_gzip", "--gzip_level", "2") == "--gzip_level must be 0 (literals only) or 1 (with matches), not 2"
    for flag in (("--track_classes", "1"), ("--track_digits", "3"), ("--track_bin", "10")):
        assert _predict(files, *flag) == "--track_classes, --track_digits and --track_bin need --track_dir"
    assert _predict(files, *d, "--track_digits", "0") == "--track_digits must lie in 1..4, not 0"
    assert _predict(files, *d, "--track_digits", "5") == "--track_digits must lie in 1..4, not 5"
    assert _predict(files, *d, "--track_bin", "0") == "--track_bin must be at least 1, not 0"
    assert _predict(files, *d, inputs=[files.fa, files.other]) == (f"--track_dir: {files.fa} and {files.other} have the same file name; their "
                                                                  "tracks would collide")
    assert _predict(files, *d, inputs=[files.fa, files.fa]) == f"--track_dir: {files.fa} and {files.fa} have the same file name; their tracks would collide"
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert _predict(files, *d) == "--track_dir runs in one process (WORLD_SIZE > 1 is not supported for probability tracks)"
    assert not os.path.exists(files.out)


BELONGS = [("--mask_twobit", ["--mask_twobit"]),
           ("--mask_dir", ["--mask_dir", "d"]), ("--mask_dir", ["--mask_gzip"]),
           ("--track_dir", ["--track_dir", "d"]), ("--track_dir", ["--track_gzip"]), ("--track_dir", ["--track_index"]),
           ("--track_dir", ["--track_bigwig"]),
           ("--gzip_level", ["--gzip_level", "1"]),
           ("--seq_dir", ["--seq_dir", "d"]), ("--seq_dir", ["--seq_classes", "1"]), ("--seq_dir", ["--seq_flank", "3"]),
           ("--seq_dir", ["--seq_width", "70"]), ("--seq_dir", ["--seq_gzip"]), ("--seq_dir", ["--seq_fai"]),
           ("--summary_dir", ["--summary_dir", "d"]), ("--summary_dir", ["--summary_bin", "7"]),
           ("--bed_bigbed", ["--bed_bigbed"]), ("--bed_gff3", ["--bed_gff3"]), ("--bed_names", ["--bed_names", "a,b"]),
           ("--bed_dir", ["--bed_dir", "d"]), ("--bed_dir", ["--bed_min_score", "3"]), ("--bed_dir", ["--bed_gzip"]),
           ("--bed_dir", ["--bed_index"])]


@pytest.mark.parametrize("named,flags", BELONGS, ids=[" ".join(f) for _n, f in BELONGS])
def test_evaluate_sends_predicts_flags_back(files, monkeypatch, named, flags):
    assert _said(flags + ["evaluate", "m.h5", "rm.out", files.fa]) == f"{named} belongs to predict, not evaluate"
    monkeypatch.setenv("WORLD_SIZE", "2")                 # the process count is looked at first
    assert _said(flags + ["evaluate", "m.h5", "rm.out", files.fa]) == "evaluate runs in one process on one GPU; it cannot be sharded (WORLD_SIZE > 1)"


def test_evaluate_keeps_what_it_never_refused(files):
    """--mask soft|hard and --mask_classes and --track_classes, --track_digits, --track_bin have no line of their own on `evaluate`: the
    first refusal behind them speaks."""
    for flags in (["--mask", "hard"], ["--mask_classes", "1"], ["--track_classes", "1"], ["--track_digits", "2"], ["--track_bin", "4"]):
        assert _said(flags + ["evaluate", "m.h5", "rm.out", files.fa, "--min_overlap", "0"]) == "--min_overlap must lie in (0, 1], not 0.0"


# ---- the refusals that need the model's class count: each module's from_plan(plan, classes), five classes
def _args(files, **kw):
    return argparse.Namespace(FASTA=[files.fa], **kw)


def _bound(module, files, **kw):
    import importlib
    m = importlib.import_module("deepgrp_amd." + module)
    plan = m.plan(_args(files, **kw))
    with pytest.raises(SystemExit) as e:
        m.from_plan(plan, 5)
    return str(e.value)


def test_the_class_count_refusals(files):
    assert _bound("tracks", files, track_dir=files.out, track_classes=(1, 5)) == ("--track_classes: label 5 is not a class of this model "
                                                                                 "(labels 0..4)")
    assert _bound("repeatseq", files, seq_dir=files.out, seq_classes=(1, 5)) == ("--seq_classes: label 5 is not a repeat class of this model "
                                                                                "(labels 1..4)")
    assert _bound("repeatseq", files, seq_dir=files.out, seq_classes=(0,)) == ("--seq_classes: label 0 is not a repeat class of this model "
                                                                              "(labels 1..4)")
    assert _bound("masking", files, mask_dir=files.out, mask_classes=(1, 5)) == ("--mask_classes: label 5 is not a repeat class of this model "
                                                                                "(labels 1..4)")
    three = "--bed_names gives 3 names, but the model has 4 repeat classes (labels 1..4)"
    assert _bound("bed", files, bed_dir=files.out, bed_gff3=True, bed_names="a,b,c") == three
    assert _bound("summary", files, summary_dir=files.out, bed_names="a,b,c") == three
    import importlib
    summary = importlib.import_module("deepgrp_amd.summary")
    plan = summary.plan(_args(files, summary_dir=files.out))
    for classes in (summary.MIN_CLASSES - 1, summary.MAX_CLASSES + 1):
        with pytest.raises(SystemExit) as e:
            summary.from_plan(plan, classes)
        assert str(e.value) == f"--summary_dir: the model has {classes} classes; the summary takes {summary.MIN_CLASSES}..{summary.MAX_CLASSES}"


def test_from_plan_takes_what_the_model_has(files):
    """Labels inside the model, the right number of names, and no plan at all."""
    from deepgrp_amd import bed, masking, repeatseq, summary, tracks
    for m in (bed, masking, repeatseq, summary, tracks):
        assert m.plan(_args(files)) is None
    assert tracks.from_plan(tracks.plan(_args(files, track_dir=files.out, track_classes=(0, 4))), 5).spec.classes == (0, 4)
    assert tracks.from_plan(tracks.plan(_args(files, track_dir=files.out)), 5).spec.classes == (1, 2, 3, 4)
    for m, kw in ((repeatseq, dict(seq_dir=files.out, seq_classes=(1, 4))), (masking, dict(mask_dir=files.out, mask_classes=(4,))),
                  (bed, dict(bed_dir=files.out, bed_gff3=True, bed_names="a,b,c,d")), (summary, dict(summary_dir=files.out, bed_names="a,b,c,d"))):
        out = m.from_plan(m.plan(_args(files, **kw)), 5)
        assert callable(out.open)
