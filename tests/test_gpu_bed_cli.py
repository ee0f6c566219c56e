"""predict --bed_dir end to end: the BED file equals the composition by the Python API (merged -> labels -> segments, then
bed.reference_scores and bed.reference_lines on the merged array read back) on the batch path, the one-by-one path, the staged -vv
path, -m and --fast; the TSV, the masked copy and the tracks are the bytes of a run without the flag; --bed_min_score filters the
BED only; an all-N record leaves no file; BGZF and .npz inputs."""
import logging
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
MODELS = [("model_u8_T20.h5", 20), ("model_u16_T30_att_vlen.h5", 30)]


def _records(T, twins=True, empty=False):
    rng = np.random.default_rng(31)
    seq = lambda n: rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes()
    recs = [(b"ctg1 first of several", seq(700)), (b"ctg2", seq(1501)), (b"ctg3 x", seq(333)),
            (b"withN lead and trail", b"NNNNN" + seq(2000) + b"NN"),
            (b"big", seq(3000)),
            (b"tiny below the window", seq(T - 3)),                                   # no window: the merged array is all zeros
            (b"empty no sequence at all", b""),                                       # no base: no predicted repeat (empty=True only)
            (b"twin one", seq(900)), (b"twin two" if twins else b"twin2 two", seq(801))]  # two records sharing a first word
    return recs if empty else [r for r in recs if r[1]]


def _fasta_bytes(recs):
    return b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in recs)


def _compose(model_file, recs, use_mss=True, fast=False, min_score=0, name=None):
    """-> (BED bytes, column 5 of every line before the filter, lines of the record without a window)
    (a record without a base has no merged array, no rows and no lines: the command line's own rule, RecordRunner.run_record)"""
    from deepgrp_amd import bed, model as dgmodel
    from deepgrp_amd.pipeline import ContigPipeline, upload_sequence
    model = dgmodel.load_model(model_file)
    pipe = ContigPipeline(model, 4, 7, 3, 5, use_mss=use_mss, fast=fast)
    out, col5, tiny = [], [], None
    for header, seq in recs:
        st, d_idx = upload_sequence(seq)
        if d_idx.numel() == 0:
            continue
        merged = pipe.merged(d_idx)
        rows = pipe.segments(pipe.labels(merged), st)
        scores = bed.reference_scores(merged.cpu().numpy(), st, rows)
        nm = name if name is not None else header.split()[0]
        full = bed.reference_lines([nm], False, rows, scores, 0)
        col5 += [int(ln.split(b"\t")[4]) for ln in full.split(b"\n")[:-1]]
        if header.startswith(b"tiny"):
            tiny = full
        out.append(bed.reference_lines([nm], False, rows, scores, min_score))
    pipe.close()
    model.close()
    return b"".join(out), col5, tiny


def _main(argv):
    from deepgrp_amd.__main__ import main
    main(argv)


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.fixture
def quiet():
    yield
    logging.getLogger("deepgrp_amd.__main__").setLevel(logging.WARNING)              # -vv sets the module's level for the process


@pytest.mark.parametrize("model_name,T", MODELS)
def test_bed_is_the_composition_on_every_path(tmp_path, monkeypatch, quiet, model_name, T):
    from deepgrp_amd import runner
    from deepgrp_amd.pipeline import ContigPipeline
    model_file = os.path.join(GOLDEN, model_name)
    recs = _records(T, empty=True)
    fa = tmp_path / "in.fa"
    fa.write_bytes(_fasta_bytes(recs))
    want, col5, tiny = _compose(model_file, recs)
    assert want.count(b"\n") > 8
    # below the window length nothing is merged: every probability is 0, and whatever rows the labels give score 0
    assert all(ln.split(b"\t")[4:] == [b"0", b".", b"0.0000", b"0.0000", b"0.0000"] for ln in tiny.split(b"\n")[:-1])
    names = {ln.split(b"\t")[0] for ln in want.split(b"\n")[:-1]}
    assert names <= {b"ctg1", b"ctg2", b"ctg3", b"withN", b"big", b"tiny", b"twin"} and len(names) >= 4     # none of the empty record
    plain = tmp_path / "plain.tsv"
    _main(FLAGS + ["predict", model_file, str(fa), "--output", str(plain)])
    assert plain.read_bytes().count(b"\n") == want.count(b"\n")                       # a BED line per TSV row

    batched = []
    real = ContigPipeline.run_batch_probs

    def counting(self, d_base, offsets, lengths, *a, **k):
        batched.append(len(lengths))
        return real(self, d_base, offsets, lengths, *a, **k)
    monkeypatch.setattr(ContigPipeline, "run_batch_probs", counting)

    def run(tag, extra=(), top=()):
        d, tsv = tmp_path / f"bed_{tag}", tmp_path / f"{tag}.tsv"
        _main(list(top) + FLAGS + ["predict", model_file, str(fa), "--output", str(tsv), "--bed_dir", str(d)] + list(extra))
        assert os.listdir(d) == ["in.fa.bed"], tag
        return (d / "in.fa.bed").read_bytes(), tsv.read_bytes()

    bed_batch, tsv = run("batch")
    assert sum(batched) == len(recs) - 1 and max(batched) > 1                         # every record with a base went through the batch entry
    assert bed_batch == want and tsv == plain.read_bytes()
    del batched[:]
    with monkeypatch.context() as mp:
        mp.setattr(runner, "SMALL_RECORD", 0)                                         # every record on its own
        bed_single, tsv = run("single")
    assert not batched and bed_single == want and tsv == plain.read_bytes()
    bed_vv, tsv = run("vv", top=["-vv"])
    logging.getLogger("deepgrp_amd.__main__").setLevel(logging.WARNING)
    assert not batched and bed_vv == want and tsv == plain.read_bytes()
    # the README form with the flags in front
    d = tmp_path / "bed_readme"
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        _main(["--bed_dir", str(d), "--bed_min_score", "0"] + FLAGS + [model_file, str(fa)])
    assert (d / "in.fa.bed").read_bytes() == want and buf.getvalue().encode() == plain.read_bytes()

    # -m and --fast: their own compositions, their own TSV
    for tag, extra, kw in (("m", ["-m"], dict(use_mss=False)), ("fast", ["--fast"], dict(fast=True))):
        _main(FLAGS + ["predict", model_file, str(fa), "--output", str(tmp_path / f"plain_{tag}.tsv")] + extra)
        got, tsv = run(tag, extra)
        want_x, _c, _t = _compose(model_file, recs, **kw)
        assert got == want_x and want_x.count(b"\n") > 0, tag
        assert tsv == (tmp_path / f"plain_{tag}.tsv").read_bytes(), tag

    # --bed_min_score: exactly the lines of the full file at or above the threshold; the TSV is not filtered
    distinct = sorted(set(col5))
    assert len(distinct) > 1, "every row has the same score: the filter cannot be told from no filter"
    low = distinct[len(distinct) // 2]
    got, tsv = run("low", ["--bed_min_score", str(low)])
    kept = [ln for ln in want.split(b"\n")[:-1] if int(ln.split(b"\t")[4]) >= low]
    assert 0 < len(kept) < want.count(b"\n")
    assert got == b"".join(ln + b"\n" for ln in kept) and tsv == plain.read_bytes()
    assert got == _compose(model_file, recs, min_score=low)[0]


def test_other_outputs_are_unchanged(tmp_path, monkeypatch):
    """--mask_dir and every kind of --track_dir output beside --bed_dir: the same bytes as without it, and the same BED; under -vv
    (the staged path, both sinks on every record) the same bytes again."""
    from deepgrp_amd import runner
    model_file, T = os.path.join(GOLDEN, MODELS[0][0]), MODELS[0][1]
    recs = _records(T, twins=False)                                                   # (a bigWig takes no two records of one name)
    fa = tmp_path / "in.fa"
    fa.write_bytes(_fasta_bytes(recs))
    want = _compose(model_file, recs)[0]
    combos = {"text": [], "gz": ["--track_gzip", "--track_index"], "bw": ["--track_bigwig"]}
    by_grouping = {}
    for small in (None, 0):
        with monkeypatch.context() as mp:
            if small is not None:
                mp.setattr(runner, "SMALL_RECORD", small)
            for tag, extra in combos.items():
                legs = [("0", False, []), ("1", True, [])]
                # -vv never batches: once per combination.  Text is the same bytes however the records are grouped into writes; a
                # bigWig's zoom blocks span the records of a write, so its bytes are those of the run that writes record by record
                if (tag, small) in (("text", None), ("bw", 0)):
                    legs.append(("vv", True, ["-vv"]))
                outs = []
                for leg, with_bed, top in legs:
                    d = tmp_path / f"{tag}_{small}_{leg}"
                    argv = FLAGS + ["predict", model_file, str(fa), "--output", str(d / "o.tsv"), "--mask_dir", str(d / "mask"),
                                    "--track_dir", str(d / "tracks"), "--track_bin", "3"] + extra
                    os.makedirs(d)
                    try:
                        _main(top + argv + (["--bed_dir", str(d / "bed")] if with_bed else []))
                    finally:
                        logging.getLogger("deepgrp_amd.__main__").setLevel(logging.WARNING)   # -vv sets the level for the process
                    outs.append((open(d / "o.tsv", "rb").read(), _files(d / "mask"), _files(d / "tracks")))
                    if with_bed:
                        assert _files(d / "bed") == {"in.fa.bed": want}, (tag, small, leg)
                assert all(out == outs[0] for out in outs[1:]), (tag, small)
                assert len(outs[1][2]) >= 4 and outs[1][1]
                by_grouping[tag, small] = outs[0]
    # batched or record by record: the same TSV and masked copy, the same track files, and for text tracks the same bytes in them
    for tag in combos:
        a, b = by_grouping[tag, None], by_grouping[tag, 0]
        assert a[:2] == b[:2] and sorted(a[2]) == sorted(b[2]), tag
    assert by_grouping["text", None] == by_grouping["text", 0]


def test_all_n_record_leaves_no_bed(tmp_path):
    model_file, T = os.path.join(GOLDEN, MODELS[0][0]), MODELS[0][1]
    recs = _records(T)
    good, bad = tmp_path / "good.fa", tmp_path / "bad.fa"
    good.write_bytes(_fasta_bytes(recs[:3]))
    bad.write_bytes(_fasta_bytes(recs[:2] + [(b"allN", b"N" * 40)] + recs[2:4]))
    for k, extra in enumerate(([], ["--track_dir", str(tmp_path / "tracks")])):
        d = tmp_path / f"bed{k}"
        with pytest.raises(ValueError, match="negative dimensions"):
            _main(FLAGS + ["predict", model_file, str(good), str(bad), "--output", str(tmp_path / "o.tsv"), "--bed_dir", str(d)] + extra)
        assert os.listdir(d) == ["good.fa.bed"]                                       # the finished input's file; nothing of the other
        assert (d / "good.fa.bed").read_bytes() == _compose(model_file, recs[:3])[0]
    assert all(f.startswith("good.fa.") for f in os.listdir(tmp_path / "tracks"))


def test_bgzf_npz_stdin_and_empty_inputs(tmp_path, monkeypatch):
    import io
    import sys

    from deepgrp_amd.gz import bgzf_compress
    model_file, T = os.path.join(GOLDEN, MODELS[1][0]), MODELS[1][1]
    recs = _records(T)
    text = _fasta_bytes(recs)
    packed = tmp_path / "in.fa.gz"
    packed.write_bytes(bgzf_compress(text, block=5000))                                # several members
    seq = recs[3][1]                                                                  # leading and trailing N
    onehot = np.zeros((5, len(seq)), np.int8)
    onehot[np.frombuffer(seq.translate(bytes.maketrans(b"ACGTN", bytes(range(5)))), np.uint8), np.arange(len(seq))] = 1
    npz = tmp_path / "sample.one.fa.gz.npz"
    np.savez(npz, fwd=onehot)
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    d = tmp_path / "bed"
    monkeypatch.setattr(sys, "stdin", io.StringIO(text.decode()))
    _main(FLAGS + ["predict", model_file, str(packed), str(npz), "-", str(empty), "--output", str(tmp_path / "o.tsv"), "--bed_dir", str(d)])
    want = _compose(model_file, recs)[0]
    got = _files(d)
    assert sorted(got) == ["empty.fa.bed", "in.fa.gz.bed", "sample.one.fa.gz.npz.bed", "stdin.bed"]
    assert got["in.fa.gz.bed"] == want and got["stdin.bed"] == want and want
    assert got["empty.fa.bed"] == b""                                                 # an input without rows: an empty file
    want_npz = _compose(model_file, [recs[3]], name=b"sample")[0]                     # evaluation.record_name of an .npz input
    assert got["sample.one.fa.gz.npz.bed"] == want_npz and want_npz.startswith(b"sample\t")
