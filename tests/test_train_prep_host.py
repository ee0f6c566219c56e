"""Host side of `train` from a sequence file (no GPU): the numpy statement of truth, class sets and the uniform map against the
reference's host functions for one record, the rank sampler against fetch_batch, the host scan of record names, and the refusals
of the command, which come before torch or the library is loaded."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import train_prep_oracle as tpo
import twobit_corpus as tbc
from deepgrp_amd import preprocessing, synthetic, training
from deepgrp_amd.model import Options

LETTERS = np.frombuffer(b"ACGTN", np.uint8)


def _onehot(idx):
    fwd = np.zeros((5, idx.size), np.int8)
    fwd[idx, np.arange(idx.size)] = 1
    return fwd


def _record(n, lead, trail, seed):
    """Class indices of a record: `lead` / `trail` N at the ends, n bases between them that begin and end with a non-N base."""
    rng = np.random.default_rng(seed)
    body = rng.integers(0, 5, n).astype(np.uint8)
    body[0], body[-1] = 1, 2
    return np.concatenate([np.full(lead, 4, np.uint8), body, np.full(trail, 4, np.uint8)])


@pytest.mark.parametrize("T", [1, 2, 5, 7, 40])
@pytest.mark.parametrize("extra", [0, 1, 2, 30])
def test_statement_equals_the_reference_functions_for_one_record(tmp_path, T, extra):
    """preprocess_y + drop_start_end_n + onehot_to_index + _calc_indices on the whole record against the statement on the device
    ingest's view of it (startpos, kept length); kept span of T, T + 1, T + 2 and T + 30 bases; runs shorter and longer than T, a
    row clipped at either end of the span, a row in the N flank, two classes on one base, an unwanted number."""
    lead, trail = 9, 4
    n = T + extra                                                       # bases of the training span
    idx = _record(n + 1, lead, trail, seed=T * 100 + extra)             # kept length n + 1: the span drops its last base
    total = idx.size
    rows = [("chrQ", 0, lead + 2, 1), ("chrQ", lead + n - 1, total, 2), ("chrQ", 2, 5, 3), ("chrQ", lead + 3, lead + 4, 3),
            ("chrQ", lead + 3, lead + 3 + T + 3, 1), ("chrQ", lead + 5, lead + 6, 9), ("chrZ", lead, lead + 3, 2),
            ("chrQ", lead + n // 2, lead + n // 2 + 2, 2)]
    bed = tmp_path / "rm.bed"
    bed.write_text("".join(f"{c}\t{b}\t{e}\t{k}\tx\ty\n" for c, b, e, k in rows))
    repeats = [1, 2, 3]
    y = preprocessing.preprocess_y(bed, "chrQ", total, repeats)
    fwd, y = preprocessing.drop_start_end_n(_onehot(idx), y)
    want_idx = training.onehot_to_index(fwd)
    # the device ingest's view: startpos = leading N, kept length from the first to the last non-N base
    keep = np.flatnonzero(idx != 4)
    startpos, length = int(keep[0]), int(keep[-1]) + 1 - int(keep[0])
    assert (startpos, length) == (lead, n + 1)
    got_rows = training.read_truth_rows(bed, ["chrQ"], repeats)["chrQ"]
    triples = [(int(q["start"]), int(q["end"]), int(q["label"])) for q in got_rows]
    got = tpo.truth(4, n, [0], [n], [startpos], [triples])
    assert np.array_equal(got, y) and got.dtype == y.dtype
    assert np.array_equal(idx[startpos:startpos + n], want_idx)
    for c in (1, 2, 3):
        assert np.array_equal(tpo.class_starts(got[c], [0], [n], T), training._calc_indices(y[c], T)), c
    W = n - T
    assert int(tpo.window_prefix([n], T)[-1]) == max(W, 0)
    for k in range(W):
        assert tpo.uniform_start(k, [0], [n], T) == k                   # rng.integers(0, length - vecsize) is the start itself


def test_statement_on_two_records_keeps_windows_inside_their_record():
    T = 6
    row = np.zeros(40, np.int8)
    row[17:20] = 1                                                       # the last bases of record A = [0, 20)
    got = tpo.class_starts(row, [0, 20], [20, 20], T)
    assert got.tolist() == [11, 12, 13]                                  # s <= 20 - 1 - T; nothing of record B although A's run abuts it
    assert tpo.uniform_start(13, [0, 20], [20, 20], T) == 13 and tpo.uniform_start(14, [0, 20], [20, 20], T) == 20
    assert tpo.resolve([(0, 99), (-1, 99), (5, -3)], [got], [0, 20], [20, 20], T).tolist() == [13, 33, 0]


def _truth(n, runs, classes):
    y = np.zeros((classes, n), np.int8)
    for c, a, b in runs:
        y[c, a:b] = 1
    y[0, y[1:].sum(0) == 0] = 1
    return y


@pytest.mark.parametrize("seed", range(6))
def test_rank_sampler_equals_fetch_batch(seed):
    """draw_picks resolved by numpy against fetch_batch, batch for batch, over ten batches; class 2 has too few indices and is left
    out by both, class 3 is absent."""
    n, T = 700, 10
    y = _truth(n, [(1, 100, 300), (2, 6, 7), (1, 500, 503)], classes=4)
    data = preprocessing.Data(np.zeros((5, n), np.int8), y)
    opt = Options(vecsize=T, batch_size=40, repeat_probability=0.6, repeats_to_search=[1, 2, 3])
    quota = int(40 * 0.6 / 3)
    sets = [tpo.class_starts(y[c], [0], [n], T) for c in (1, 2, 3)]
    assert 0 < len(sets[1]) <= quota and len(sets[2]) == 0 and len(sets[0]) > quota
    kept = [s for s in sets if len(s) > quota]
    want = training.fetch_batch(opt, data, np.random.default_rng(seed))()
    rng = np.random.default_rng(seed)
    for _ in range(10):
        picks = training.draw_picks(rng, [len(s) for s in kept], n - T, 40, quota)
        assert picks.shape == (40, 2) and picks.dtype == np.int64
        assert np.array_equal(tpo.resolve(picks, kept, [0], [n], T), next(want))
    assert np.array_equal(rng.integers(0, 1 << 30, 4), _after(opt, data, seed, 10))      # both generators stand at the same place


def _after(opt, data, seed, batches):
    rng = np.random.default_rng(seed)
    gen = training.fetch_batch(opt, data, rng)()
    for _ in range(batches):
        next(gen)
    return rng.integers(0, 1 << 30, 4)


def test_sequence_names_on_the_host(tmp_path):
    text = b">chr1 first record\nACGT\nAC\n>chr2\nTT\n>\nAA\n>chr3\tx\r\nGG\n>chr4"
    plain = tmp_path / "a.fa"
    plain.write_bytes(text)
    assert training.sequence_names(plain) == ["chr1", "chr2", "chr3", "chr4"]
    gz = tmp_path / "a.fa.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    assert training.sequence_names(gz) == ["chr1", "chr2", "chr3", "chr4"]
    two = tmp_path / "a.2bit"
    two.write_bytes(tbc.write([tbc.Rec(b"chrA", [0, 1, 2, 3], [], [], [0, 0, 0]), tbc.Rec(b"chrB", [2, 2], [], [], [0, 0, 0])]))
    assert training.sequence_names(two) == ["chrA", "chrB"]
    assert training.select_contigs(["a", "b", "c"], ["c", "a"], "f") == ["a", "c"]          # file order, whatever the flag's order
    with pytest.raises(ValueError, match="no record named 'x'"):
        training.select_contigs(["a", "b"], ["a", "x"], "f")
    with pytest.raises(ValueError, match="two records are named 'a'"):
        training.select_contigs(["a", "b", "a"], None, "f")
    assert training.select_contigs(["a", "b", "a"], ["b"], "f") == ["b"]                    # the duplicate is not selected


def test_a_kept_row_without_a_truth_row_is_named(tmp_path):
    bed = tmp_path / "rm.bed"
    bed.write_text("chr1\t5\t9\t1\nchr1\t5\t9\t7\nchr1\t1\t2\t3\n")
    rows = training.read_truth_rows(bed, ["chr1"], [1, 2])["chr1"]
    assert rows["label"].tolist() == [1]                                 # 7 and 3 are not searched for
    with pytest.raises(ValueError, match=r"rm\.bed:2: repeat number 7"):
        training.read_truth_rows(bed, ["chr1"], [1, 7])                  # the reference's IndexError: y has rows 0..2 only


# ------------------------------------------------------------------------------------------------ the command's refusals
def _inputs(tmp):
    n = 3000
    idx, _lab = synthetic.synthetic_truth(n, contig=3, flank=50)
    seq = LETTERS[idx].tobytes()
    paths = {"npz": os.path.join(tmp, "chrA.fa.gz.npz"), "fa": os.path.join(tmp, "one.fa"), "two": os.path.join(tmp, "two.fa"),
             "dup": os.path.join(tmp, "dup.fa"), "bed": os.path.join(tmp, "rm.bed"), "toml": os.path.join(tmp, "p.toml")}
    np.savez(paths["npz"], fwd=_onehot(idx))
    with open(paths["fa"], "wb") as fh:
        fh.write(b">chrA\n" + seq + b"\n")
    with open(paths["two"], "wb") as fh:
        fh.write(b">chrA x\n" + seq + b"\n>chrB\n" + seq[::-1] + b"\n")
    with open(paths["dup"], "wb") as fh:
        fh.write(b">chrA x\n" + seq + b"\n>chrA y\n" + seq[::-1] + b"\n")
    with open(paths["bed"], "w") as fh:
        fh.writelines(synthetic.synthetic_annotation(n, contig=3, name="chrA", flank=50))
    with open(paths["toml"], "w") as fh:
        fh.write("units = 4\nvecsize = 20\nbatch_size = 8\nn_batches = 2\nn_epochs = 1\n")
    return paths


@pytest.mark.parametrize("train,valid,flags,words", [
    ("npz", "fa", [], ["chrA.fa.gz.npz", "one.fa", ".npz", "sequence file"]),
    ("fa", "npz", [], ["chrA.fa.gz.npz", "one.fa", ".npz", "sequence file"]),
    ("npz", "npz", ["--train_contigs", "chrA"], ["--train_contigs", ".npz"]),
    ("npz", "npz", ["--valid_contigs", "chrA"], ["--valid_contigs", ".npz"]),
    ("two", "fa", ["--train_contigs", "chrA,chrC"], ["--train_contigs", "'chrC'", "two.fa"]),
    ("fa", "two", ["--valid_contigs", "chrX"], ["--valid_contigs", "'chrX'", "two.fa"]),
    ("dup", "fa", [], ["'chrA'", "dup.fa", "two records"]),
    ("fa", "dup", ["--valid_contigs", "chrA"], ["'chrA'", "dup.fa", "two records"]),
], ids=["npz+fasta", "fasta+npz", "train_contigs+npz", "valid_contigs+npz", "missing-train", "missing-valid", "duplicate", "duplicate-selected"])
def test_train_refuses_by_name_before_torch_or_the_library_is_loaded(tmp_path, train, valid, flags, words):
    tmp = str(tmp_path)
    paths = _inputs(tmp)
    model, logdir = os.path.join(tmp, "m.hdf5"), os.path.join(tmp, "log")
    res = subprocess.run([sys.executable, "-X", "importtime", "-m", "deepgrp_amd", "train", paths["toml"], paths[train], paths[valid],
                          paths["bed"], "--logdir", logdir, "--modelfile", model, "--seed", "1"] + flags,
                         cwd=ROOT, capture_output=True, text=True)
    imported = set(re.findall(r"^import time:\s+\d+ \|\s+\d+ \|\s+(\S+)$", res.stderr, flags=re.M))
    message = "\n".join(l for l in res.stderr.splitlines() if not l.startswith("import time:"))
    assert res.returncode != 0, message
    for word in words:
        assert word in message, (word, message)
    assert "Traceback" not in message
    assert "numpy" in imported, "the import log is not being read"
    assert not {"torch", "deepgrp_amd._lib", "deepgrp_amd.pipeline"} & imported, sorted(m for m in imported if m.startswith(("torch", "deepgrp")))[:20]
    assert not os.path.exists(model) and not os.path.exists(logdir)
