"""`evaluate` and `train` given a RepeatMasker listing against the same commands given the table parse_rm writes from it: the same
reports, the same refusal (naming the listing's line), the same model bytes.  Model and records as in tests/test_gpu_evaluate.py and
tests/test_gpu_train.py."""
import gzip
import json

import pytest

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _synthetic_model(tmp_path):
    from deepgrp_amd import model as dgmodel, synthetic
    w = synthetic.trained_weights()
    path = str(tmp_path / "synth.hdf5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path


def _listing_lines(n, contig, name, flank):
    """The planted runs of the synthetic chromosome as `.out` lines (1-based begin), class k as the k-th numbered family; between
    them lines parse_rm skips and one rmsk line."""
    from deepgrp_amd import synthetic
    lines = []
    for k, row in enumerate(synthetic.synthetic_annotation(n, contig=contig, name=name, flank=flank)):
        ctg, b, e, lab = row.split("\t")[:4]
        lines.append(rm_cases.out_line(ctg, int(b) + 1, int(e), "x", rm_cases.FAMILIES[int(lab) - 1], "+C"[k % 2]))
        if k % 3 == 0:
            lines.append(rm_cases.out_line(ctg, int(b) + 1, int(e), "(CA)n", "Simple_repeat"))
    lines.append(rm_cases.rmsk_line(name, flank + 100, flank + 900, "L2a", "LINE", "L2"))
    lines.append(rm_cases.out_line("chrUn", 10, 500, "x", "SINE/MIR"))
    return lines


def _write_pair(tmp_path, lines, stem="rm", packed=False):
    from deepgrp_amd._scripts import parse_rm
    listing, plain, table = tmp_path / (stem + (".out.gz" if packed else ".out")), tmp_path / (stem + ".plain.out"), tmp_path / (stem + ".bed")
    text = rm_cases.HEADER + "\n".join(lines) + "\n"
    plain.write_text(text)
    if packed:
        with gzip.open(listing, "wt") as fh:
            fh.write(text)
    else:
        listing.write_text(text)
    parse_rm.main([str(plain), "-o", str(table)])
    return str(listing), str(table)


@pytest.mark.parametrize("packed", [False, True])
def test_evaluate_gives_the_reports_of_the_table(tmp_path, packed):
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    n, fl = 60_000, 1000
    fa = tmp_path / "one.fa"
    fa.write_text(">chr1 synthetic\n" + synthetic.synthetic_chromosome(n, contig=10, flank=fl).decode() + "\n")
    listing, table = _write_pair(tmp_path, _listing_lines(n, 10, "chr1", fl), packed=packed)
    covered = sum(int(x.split("\t")[2]) - int(x.split("\t")[1]) for x in open(table))
    assert covered > 2000
    model = _synthetic_model(tmp_path)
    out = {}
    for tag, ann, extra in (("table", table, []), ("listing", listing, []), ("named", listing, ["--annotation_format", "repeatmasker"])):
        main(["evaluate", model, ann, str(fa), "--output", str(tmp_path / f"{tag}.tsv"), "--json", str(tmp_path / f"{tag}.json")] + extra)
        js = json.load(open(tmp_path / f"{tag}.json"))
        assert js.pop("annotation") == ann
        out[tag] = (open(tmp_path / f"{tag}.tsv", "rb").read(), js)
    assert out["table"][1]["rows_used"] > 0 and out["table"][1]["metrics"]["MCC"] > 0
    assert out["listing"] == out["table"] and out["named"] == out["table"]


def test_evaluate_refuses_a_negative_begin_naming_the_listings_line(tmp_path):
    from deepgrp_amd.__main__ import main
    lines = [rm_cases.out_line("chr1", 100, 200), rm_cases.out_line("chr1", 0, 50, fam="LINE/L1"), rm_cases.out_line("chr1", 300, 400)]
    listing, table = _write_pair(tmp_path, lines)
    fa = tmp_path / "one.fa"
    fa.write_text(">chr1\n" + "ACGT" * 200 + "\n")
    model = _synthetic_model(tmp_path)
    with pytest.raises(SystemExit) as on_table:
        main(["evaluate", model, table, str(fa)])
    assert str(on_table.value.code).startswith(f"{table}:2: negative begin")
    with pytest.raises(SystemExit) as on_listing:
        main(["evaluate", model, listing, str(fa)])
    assert str(on_listing.value.code) == f"{listing}:5: negative begin: {lines[1]!r}"


def test_train_writes_the_model_of_the_table(tmp_path):
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    sizes = (("chrtrain", 60_000, 10), ("chrvalid", 30_000, 11))
    lines = []
    for name, n, contig in sizes:
        (tmp_path / f"{name}.fa").write_text(f">{name}\n" + synthetic.synthetic_chromosome(n, contig=contig, flank=500).decode() + "\n")
        lines += _listing_lines(n, contig, name, 500)
    listing, table = _write_pair(tmp_path, lines)
    toml = tmp_path / "p.toml"
    toml.write_text("units = 4\nvecsize = 20\nbatch_size = 16\nn_batches = 2\nn_epochs = 1\nattention = true\ndropout = 0.25\n")
    out = {}
    for tag, bed in (("table", table), ("listing", listing)):
        model = tmp_path / f"{tag}.hdf5"
        main(["train", str(toml), str(tmp_path / "chrtrain.fa"), str(tmp_path / "chrvalid.fa"), bed, "--logdir", str(tmp_path / tag),
              "--modelfile", str(model), "--seed", "3"])
        out[tag] = (open(model, "rb").read(), open(tmp_path / tag / "history.tsv").read())
    assert out["listing"] == out["table"]
    # the truth matters: another listing, another model
    other, _t = _write_pair(tmp_path, [x for x in lines if "SINE/Alu" not in x and "HSATII" not in x], stem="other")
    model = tmp_path / "other.hdf5"
    main(["train", str(toml), str(tmp_path / "chrtrain.fa"), str(tmp_path / "chrvalid.fa"), other, "--logdir", str(tmp_path / "o"),
          "--modelfile", str(model), "--seed", "3"])
    assert open(model, "rb").read() != out["table"][0]
