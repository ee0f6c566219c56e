"""predict --summary_dir end to end on the GPU, with the trained synthetic model: every form of one input (FASTA, its CRLF twin, BGZF,
plain gzip, .2bit with its soft mask) gives the same two files, the files summary.format_summary gives over summary.count_host and
the oracle pipeline's rows; the TSV and the other outputs do not change; and no case here may count on the host what the device
should count (summary.write_summary's report is asserted, not measured)."""
import gzip
import os

import numpy as np
import pytest

import twobit_corpus as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAGS = ["-b", "7"]
BIN = 500
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
NAMES = "mono,tri,tetra,hexa"


def _record(name, n, contig, flank):
    """One record of the planted chromosome as the 2bit corpus states records: N runs as N blocks, and as its soft mask the planted
    repeats moved 40 bases to the right (so that the mask agrees with a good prediction in part)."""
    from deepgrp_amd import synthetic
    idx, lab = synthetic.synthetic_truth(n, contig=contig, flank=flank)
    codes = np.array([2, 1, 3, 0, 0], np.uint8)[idx]                       # A C G T N -> the two-bit values (T=0 C=1 A=2 G=3)
    masked = np.zeros(n, bool)
    masked[40:] = lab[:-40] > 0
    blocks = lambda flag: [(int(s), int(e - s)) for s, e in tc.intervals(n, [(int(p), 1) for p in np.flatnonzero(flag)])]
    return tc.Rec(name, codes, blocks(idx == 4), blocks(masked), np.zeros(3, np.uint8))


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The model file and the input in its five forms."""
    from deepgrp_amd import gz, model as dgmodel, synthetic
    d = tmp_path_factory.mktemp("summary_cli")
    w = synthetic.trained_weights()
    mpath = str(d / "m.hdf5")
    dgmodel.save_keras_hdf5(mpath, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    # (sizes and seeds at which the planted chromosome holds repeats of two classes: five runs in all)
    recs = [_record(b"chrA", 30000, 0, 100), _record(b"tiny", 150, 5, 10), _record(b"chrB", 15000, 1, 50), _record(b"chrC", 12003, 2, 0)]
    assert sum(len(r.mblocks) for r in recs) >= 5
    text = tc.text(recs)
    assert any(97 <= b <= 122 for b in text) and b"N" in text
    forms = {"in.fa": text, "crlf.fa": text.replace(b"\n", b"\r\n"), "bgzf.fa.gz": gz.bgzf_compress(text),
             "plain.fa.gz": gzip.compress(text), "in.2bit": tc.write(recs)}
    for name, data in forms.items():
        (d / name).write_bytes(data)
    return dict(dir=d, model=mpath, recs=recs, text=text, forms=list(forms))


@pytest.fixture()
def reports(monkeypatch):
    """Every report summary.write_summary returns while the test runs."""
    from deepgrp_amd import summary
    seen = []
    inner = summary.write_summary

    def recording(*a, **k):
        rep = inner(*a, **k)
        seen.append(rep)
        return rep

    monkeypatch.setattr(summary, "write_summary", recording)
    return seen


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _predict(setup, name, tag, *extra):
    from deepgrp_amd.__main__ import main
    d = setup["dir"] / tag
    main(FLAGS + ["predict", setup["model"], str(setup["dir"] / name), "--output", str(d) + ".tsv"] + [str(x).replace("DIR", str(d)) for x in extra])
    return (setup["dir"] / f"{tag}.tsv").read_bytes()


def _expected_rows(orc, setup):
    """The reference CLI's rows per record (oracle, from the GPU's own probabilities), in file order."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.pipeline import upload_sequence
    model = dgmodel.load_model(setup["model"])
    T, Cn = model.input_shape[1], model.output_shape[2]
    out = []
    with open(setup["dir"] / "in.fa") as fh:
        for _header, seq in orc.read_multi_fasta(fh):
            _st, d_idx = upload_sequence(seq.encode())
            nwin = orc.window_count(d_idx.numel(), T, 50)
            probs = model.forward_windows(d_idx, 50, 0, nwin).cpu().numpy() if nwin else np.zeros((0, T, Cn), np.float32)
            out.append([tuple(int(v) for v in r) for r in orc.predict_contig(seq, lambda _i: (lambda a, b: probs[a:a + b]), T, Cn, 50, 7,
                                                                                50, 50, True)])
    return out


def _expected_files(setup, per, names=None):
    from deepgrp_amd import summary
    records, density = [], [summary.density_header(5, names)]
    for r, rows in zip(setup["recs"], per):
        seq = np.frombuffer(tc.letters(r), np.uint8)
        rk = np.array([(s, e, lab, 0) for s, e, lab in rows], SEG)
        counts = summary.count_host(seq, np.arange(seq.size), rk, 5)
        records.append((r.name, counts, rk))
        density.append(summary.format_density(r.name, summary.bins_host(seq, np.arange(seq.size), rk, 5, BIN), seq.size, BIN))
    return summary.format_summary(records, 5, names), b"".join(density)


def test_every_form_gives_the_files_of_the_numpy_statement(orc, setup, reports):
    per = _expected_rows(orc, setup)
    assert sum(len(r) for r in per) >= 3 and len({r[2] for rows in per for r in rows}) > 1
    want_summary, want_density = _expected_files(setup, per)
    assert want_summary.count(b"\n") == 1 + 5 * 6
    # the table says something: repeats were found, the input's soft mask agrees with them in part
    all_line = want_summary.split(b"\n")[-2].split(b"\t")
    assert all_line[:2] == [b"*", b"all"] and 0.0 < float(all_line[16]) < 1.0 and 0.0 < float(all_line[17]) < 1.0
    plain_tsv = _predict(setup, "in.fa", "noflags")
    for name in setup["forms"]:
        tag = "form_" + name.replace(".", "_")
        tsv = _predict(setup, name, tag, "--summary_dir", "DIR", "--summary_bin", str(BIN))
        got = _files(setup["dir"] / tag)
        assert list(got) == [name + ".density.tsv", name + ".summary.tsv"], name
        assert got[name + ".summary.tsv"] == want_summary, name
        assert got[name + ".density.tsv"] == want_density, name
        if name == "in.fa":
            assert tsv == plain_tsv                                        # the TSV of a run without the flags
    assert len(reports) == len(setup["forms"])
    for rep in reports:
        assert rep["host_records"] == 0 and rep["uncounted_records"] == 0 and rep["device_records"] == rep["records"] == 4
    # --bed_names names the labels, in both files; without --summary_bin there is one file
    _predict(setup, "in.fa", "named", "--summary_dir", "DIR", "--summary_bin", str(BIN), "--bed_names", NAMES)
    named = _expected_files(setup, per, [nm.encode() for nm in NAMES.split(",")])
    assert _files(setup["dir"] / "named") == {"in.fa.summary.tsv": named[0], "in.fa.density.tsv": named[1]}
    assert named[0] != want_summary and b"\ttetra\t" in named[0]
    _predict(setup, "in.fa", "nobin", "--summary_dir", "DIR")
    assert _files(setup["dir"] / "nobin") == {"in.fa.summary.tsv": want_summary}
    assert reports[-1]["host_records"] == 0 and reports[-2]["host_records"] == 0


def test_the_three_second_passes_together_give_what_they_give_alone(setup, reports):
    tsv_m = _predict(setup, "in.fa", "only_mask", "--mask_dir", "DIR")
    tsv_q = _predict(setup, "in.fa", "only_seq", "--seq_dir", "DIR")
    tsv_s = _predict(setup, "in.fa", "only_summary", "--summary_dir", "DIR", "--summary_bin", str(BIN))
    tsv_all = _predict(setup, "in.fa", "all3", "--mask_dir", "DIR/m", "--seq_dir", "DIR/q", "--summary_dir", "DIR/s", "--summary_bin", str(BIN))
    assert tsv_m == tsv_q == tsv_s == tsv_all
    d = setup["dir"]
    assert _files(d / "all3" / "m") == _files(d / "only_mask") and list(_files(d / "only_mask")) == ["in.fa"]
    assert _files(d / "all3" / "q") == _files(d / "only_seq") and list(_files(d / "only_seq")) == ["in.fa.repeats.fa"]
    assert _files(d / "all3" / "s") == _files(d / "only_summary") and len(_files(d / "only_summary")) == 2
    assert len(_files(d / "only_seq")["in.fa.repeats.fa"]) > 0
    assert [r["host_records"] for r in reports] == [0, 0]


def test_one_odd_record_among_plain_ones_goes_through_the_host(setup, tmp_path):
    """A record with lone-CR line ends is not plain: it is counted by count_host, the plain records around it on the device, and the
    file is the statement's."""
    from deepgrp_amd import summary
    recs = setup["recs"]
    seqs = [tc.letters(r) for r in recs]
    odd = seqs[2][:3000]
    parts = [b">chrA first\n" + b"\n".join(seqs[0][i:i + 60] for i in range(0, len(seqs[0]), 60)) + b"\n",
             b">odd one\r" + b"\r".join(odd[i:i + 70] for i in range(0, len(odd), 70)) + b"\n",
             b">chrC\r\n" + b"\r\n".join(seqs[3][i:i + 80] for i in range(0, len(seqs[3]), 80)) + b"\r\n",
             b">last\n" + seqs[1]]
    fa = tmp_path / "mixed.fa"
    fa.write_bytes(b"".join(parts))
    per_seq = [seqs[0], odd, seqs[3], seqs[1]]
    names = [b"chrA", b"odd", b"chrC", b"last"]
    rng = np.random.default_rng(8)
    rows = []
    for k, s in enumerate(per_seq):
        p = 0
        while p + 200 < len(s):
            p += int(rng.integers(0, 300))
            e = min(p + int(rng.integers(1, 400)), len(s))
            rows.append((p, e, int(rng.integers(1, 5)), k))
            p = e
    rows = np.array(rows, SEG)
    out = tmp_path / "o"
    out.mkdir()
    rep = summary.write_summary(str(fa), str(out / "s.tsv"), rows, 5, bin=BIN, bin_path=str(out / "d.tsv"))
    assert rep["device_records"] == 3 and rep["host_records"] == 1 and rep["uncounted_records"] == 0 and rep["records"] == 4
    records, density = [], [summary.density_header(5)]
    for k, s in enumerate(per_seq):
        a = np.frombuffer(s, np.uint8)
        rk = rows[rows["contig"] == k]
        counts = summary.count_host(a, np.arange(a.size), rk, 5)
        records.append((names[k], counts, rk))
        density.append(summary.format_density(names[k], summary.bins_host(a, np.arange(a.size), rk, 5, BIN), a.size, BIN))
    assert (out / "s.tsv").read_bytes() == summary.format_summary(records, 5)
    assert (out / "d.tsv").read_bytes() == b"".join(density)
    assert rep["positions"] == sum(len(s) for s in per_seq) and rep["repeat_positions"] == int((rows["end"] - rows["start"]).sum())
    # groups cut at every possible place give the same files
    for group_bytes in (1, 5000):
        rep2 = summary.write_summary(str(fa), str(out / "s2.tsv"), rows, 5, bin=BIN, bin_path=str(out / "d2.tsv"), group_bytes=group_bytes)
        assert rep2 == rep
        assert (out / "s2.tsv").read_bytes() == (out / "s.tsv").read_bytes() and (out / "d2.tsv").read_bytes() == (out / "d.tsv").read_bytes()


def test_a_failing_record_leaves_no_file(setup, tmp_path, reports):
    from deepgrp_amd import summary
    from deepgrp_amd.__main__ import main
    # a row beyond its record, on the device path and on the host path: the error names the record, nothing is left in the directory
    out = tmp_path / "o"
    out.mkdir()
    n = len(tc.letters(setup["recs"][2]))
    bad = np.array([(10, 20, 1, 0), (n - 5, n + 1, 2, 2)], SEG)
    with pytest.raises(ValueError, match="chrB.*beyond"):
        summary.write_summary(str(setup["dir"] / "in.fa"), str(out / "s.tsv"), bad, 5, bin=BIN, bin_path=str(out / "d.tsv"))
    assert os.listdir(out) == []
    with pytest.raises(ValueError, match="rows name record 7"):
        summary.write_summary(str(setup["dir"] / "in.fa"), str(out / "s.tsv"), np.array([(0, 1, 1, 7)], SEG), 5)
    assert os.listdir(out) == []
    # an all-N record stops predict: the summary of that input is not written
    fa = tmp_path / "bad.fa"
    fa.write_bytes(setup["text"] + b">allN\nNNNNNNNNNN\n")
    with pytest.raises(ValueError, match="negative dimensions"):
        main(FLAGS + ["predict", setup["model"], str(fa), "--output", str(tmp_path / "bad.tsv"), "--summary_dir", str(tmp_path / "s")])
    assert os.listdir(tmp_path / "s") == []
    assert all(r["host_records"] == 0 for r in reports)
