"""The five outputs of `predict` side by side: one call with --track_dir, --bed_dir, --mask_dir, --seq_dir and --summary_dir
writes, file by file, the bytes that the same input gives when each output is asked for alone -- on a handful of short records (the
batch path), a record above runner.SMALL_RECORD (on its own) and a record without a base -- and again under -vv (record by record
down the runner's own path).  When the last committer fails, what was committed before it stays, nothing temporary is left and the
exception reaches the caller."""
import logging
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")
FLAGS = ["-s", "4", "-b", "7"]
# per form and output: its directory flag with its options
FORMS = {
    "text": {"tracks": ["--track_dir", "--track_bin", "3"], "bed": ["--bed_dir", "--bed_min_score", "1"], "mask": ["--mask_dir", "--mask", "hard"],
             "seq": ["--seq_dir", "--seq_flank", "5", "--seq_fai"], "summary": ["--summary_dir", "--summary_bin", "1000"]},
    "packed": {"tracks": ["--track_dir", "--track_gzip", "--track_index"], "bed": ["--bed_dir", "--bed_gzip", "--bed_index"],
               "mask": ["--mask_dir", "--mask_gzip"], "seq": ["--seq_dir", "--seq_gzip"], "summary": ["--summary_dir"]},
}
EXPECTED = {"tracks": 4, "bed": 1, "mask": 1, "seq": 2, "summary": 2}          # files per output in the text form


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    from deepgrp_amd import runner
    rng = np.random.default_rng(58)
    seq = lambda n: rng.choice(list(b"ACGTacgt"), size=n).astype(np.uint8).tobytes()
    recs = [(b"s%d some words" % i, seq(int(rng.integers(40, 700)))) for i in range(6)]
    recs.insert(3, (b"none no sequence at all", b""))
    recs.append((b"big one record", b"NN" + seq(runner.SMALL_RECORD + 4321) + b"N"))
    recs.append((b"tail", seq(333)))
    path = tmp_path_factory.mktemp("outputs_in") / "in.fa"
    path.write_bytes(b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs))
    return str(path)


def _files(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def _run(fasta, where, form, outputs, top=()):
    """`predict` with these outputs, each into where/<output>.  -> (TSV, {output: {file: bytes}})"""
    from deepgrp_amd.__main__ import main
    os.makedirs(where)
    argv = list(top) + FLAGS + ["predict", MODEL, fasta, "--output", os.path.join(where, "o.tsv")]
    for out in outputs:
        flags = FORMS[form][out]
        argv += [flags[0], os.path.join(where, out)] + flags[1:]
    try:
        main(argv)
    finally:
        logging.getLogger("deepgrp_amd.__main__").setLevel(logging.WARNING)      # -vv sets the module's level for the process
    return open(os.path.join(where, "o.tsv"), "rb").read(), {out: _files(os.path.join(where, out)) for out in outputs}


@pytest.fixture(scope="module")
def alone(fasta, tmp_path_factory):
    """Every output asked for alone, per form: computed once."""
    got = {}
    for form in FORMS:
        d = tmp_path_factory.mktemp("alone_" + form)
        got[form] = {out: _run(fasta, str(d / out), form, [out]) for out in FORMS[form]}
    return got


@pytest.mark.parametrize("form,top", [("text", ()), ("text", ("-vv",)), ("packed", ())], ids=["text", "text-vv", "packed"])
def test_together_is_each_alone(fasta, alone, tmp_path, form, top):
    tsv, files = _run(fasta, str(tmp_path / "all"), form, list(FORMS[form]), top)
    assert tsv.count(b"\n") > 10
    for out, (tsv_alone, files_alone) in alone[form].items():
        assert tsv_alone == tsv, out
        assert sorted(files[out]) == sorted(files_alone[out]), out
        for name, data in files_alone[out].items():
            assert files[out][name] == data, (out, name)
        assert any(files_alone[out].values()), out                 # (a class without a probability above 0 has an empty track)
        if form == "text":
            assert len(files[out]) == EXPECTED[out], (out, sorted(files[out]))


def test_a_failing_last_committer_leaves_what_was_committed(fasta, alone, tmp_path, monkeypatch):
    from deepgrp_amd import summary

    def fails(*_a, **_k):
        raise RuntimeError("the summary could not be written")
    monkeypatch.setattr(summary, "write_summary", fails)
    where = tmp_path / "all"
    with pytest.raises(RuntimeError, match="the summary could not be written"):
        _run(fasta, str(where), "text", list(FORMS["text"]))
    for out in ("tracks", "bed", "mask", "seq"):                  # committed in front of the summary: complete, as when asked for alone
        assert _files(where / out) == alone["text"][out][1][out], out
    assert os.listdir(where / "summary") == []
    assert open(where / "o.tsv", "rb").read() == alone["text"]["summary"][0]
