"""The `train` command on sequence files, on the GPU: one record as FASTA, gzip, BGZF and .2bit trains to the bytes of its
`.fa.gz.npz`; records picked with --train_contigs / --valid_contigs.  Child processes run one after another."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import twobit_corpus as tbc

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", np.uint8)
TOML = "units = 4\nvecsize = 20\nbatch_size = 8\nn_batches = 3\nn_epochs = 2\nattention = true\ndropout = 0.25\n"


def _indices(n, contig):
    from deepgrp_amd import synthetic
    return synthetic.synthetic_truth(n, contig=contig, flank=50)[0]


def _fasta(records):
    return b"".join(b">" + name + b"\n" + b"\n".join(LETTERS[idx].tobytes()[o:o + 60] for o in range(0, idx.size, 60)) + b"\n"
                    for name, idx in records)


def _twobit(records):
    recs = []
    for name, idx in records:
        codes = np.array([2, 1, 3, 0, 0], np.uint8)[idx]                 # T=0 C=1 A=2 G=3; any two bits under an N block
        edge = np.flatnonzero(np.diff(np.concatenate(([0], (idx == 4).astype(np.int8), [0]))))
        recs.append(tbc.Rec(name.split()[0], codes, [(int(a), int(b - a)) for a, b in zip(edge[::2], edge[1::2])], [], [0, 0, 0]))
    return tbc.write(recs)


def _write(path, data):
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def _annotation(path, named):
    from deepgrp_amd import synthetic
    with open(path, "w") as fh:
        for name, n, contig in named:
            fh.writelines(synthetic.synthetic_annotation(n, contig=contig, name=name, flank=50))
    return path


def _train(tmp, run, trainfile, validfile, bed, flags=()):
    logdir, model = os.path.join(tmp, run), os.path.join(tmp, run + ".hdf5")
    cmd = [sys.executable, "-m", "deepgrp_amd", "train", os.path.join(tmp, "p.toml"), trainfile, validfile, bed, "--logdir", logdir,
           "--modelfile", model, "--seed", "1"] + list(flags)
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    files = {f: open(os.path.join(logdir, f), "rb").read() for f in sorted(os.listdir(logdir))}
    return open(model, "rb").read(), files


@pytest.fixture(scope="module")
def one_record(tmp_path_factory):
    """The two records (training, validation) in every form, and what `train` writes from the .npz pair."""
    from deepgrp_amd import gz
    tmp = str(tmp_path_factory.mktemp("forms"))
    _write(os.path.join(tmp, "p.toml"), TOML.encode())
    sides = {"chrA": _indices(3000, 3), "chrB": _indices(2500, 4)}
    bed = _annotation(os.path.join(tmp, "rm.bed"), [("chrA", 3000, 3), ("chrB", 2500, 4)])
    paths = {}
    for name, idx in sides.items():
        text = _fasta([(name.encode() + b" synthetic", idx)])
        fwd = np.zeros((5, idx.size), np.int8)
        fwd[idx, np.arange(idx.size)] = 1
        np.savez(os.path.join(tmp, f"{name}.fa.gz.npz"), fwd=fwd)
        paths[name] = {
            "npz": os.path.join(tmp, f"{name}.fa.gz.npz"),
            "fasta": _write(os.path.join(tmp, f"{name}.fa"), text),
            "gzip": _write(os.path.join(tmp, f"{name}.fa.gz"), gzip.compress(text)),
            "bgzf": _write(os.path.join(tmp, f"{name}.fa.bgz"), gz.bgzf_compress(text)),
            "twobit": _write(os.path.join(tmp, f"{name}.2bit"), _twobit([(name.encode(), idx)])),
        }
    want = _train(tmp, "npz", paths["chrA"]["npz"], paths["chrB"]["npz"], bed)
    assert set(want[1]) >= {"history.tsv"} and len(want[1]["history.tsv"].splitlines()) == 3
    return tmp, paths, bed, want


@pytest.mark.parametrize("form", ["fasta", "gzip", "bgzf", "twobit"])
def test_a_sequence_file_trains_to_the_bytes_of_its_npz(one_record, form):
    tmp, paths, bed, want = one_record
    model, files = _train(tmp, form, paths["chrA"][form], paths["chrB"][form], bed)
    assert files["history.tsv"] == want[1]["history.tsv"]
    assert model == want[0]
    assert files == want[1]                                               # the best epochs' files as well


def test_contig_selection(tmp_path, capsys):
    from deepgrp_amd.__main__ import main
    tmp = str(tmp_path)
    _write(os.path.join(tmp, "p.toml"), TOML.encode())
    recs = {b"chr1": _indices(3000, 1), b"chr2": _indices(2000, 2), b"chr3": _indices(2500, 3), b"chr4": _indices(1500, 4)}
    trainfile = _write(os.path.join(tmp, "train.fa"), _fasta([(b"chr1 a", recs[b"chr1"]), (b"chr2", recs[b"chr2"])]))
    validfile = _write(os.path.join(tmp, "valid.2bit"), _twobit([(b"chr4", recs[b"chr4"]), (b"chr3", recs[b"chr3"]), (b"chr1", recs[b"chr1"])]))
    bed = _annotation(os.path.join(tmp, "rm.bed"), [("chr1", 3000, 1), ("chr2", 2000, 2), ("chr3", 2500, 3), ("chr4", 1500, 4)])
    first = _train(tmp, "first", trainfile, validfile, bed, ["--train_contigs", "chr1,chr2", "--valid_contigs", "chr3"])
    assert len(first[1]["history.tsv"].splitlines()) == 3

    def again(run, flags):
        logdir, model = os.path.join(tmp, run), os.path.join(tmp, run + ".hdf5")
        main(["train", os.path.join(tmp, "p.toml"), trainfile, validfile, bed, "--logdir", logdir, "--modelfile", model, "--seed", "1"] + flags)
        return open(model, "rb").read(), {f: open(os.path.join(logdir, f), "rb").read() for f in sorted(os.listdir(logdir))}

    assert again("second", ["--train_contigs", "chr1,chr2", "--valid_contigs", "chr3"]) == first
    assert again("swapped", ["--train_contigs", "chr2,chr1", "--valid_contigs", "chr3"]) == first     # file order, not the flag's
    other = again("other", ["--train_contigs", "chr2", "--valid_contigs", "chr3"])
    assert other[1]["history.tsv"] != first[1]["history.tsv"]                                         # the selection matters
    main(["predict", os.path.join(tmp, "first.hdf5"), trainfile])                                     # predict loads the model
    capsys.readouterr()
