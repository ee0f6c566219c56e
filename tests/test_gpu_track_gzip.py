"""predict --track_dir --track_gzip: every track file is a BGZF file whose inflated bytes are the file --track_dir alone writes, at
either --gzip_level; the TSV does not notice; a raising record leaves nothing behind; --mask_gzip --gzip_level 1 inflates to the
plain masked copy."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN
from deflate_corpus import BLOCK
from test_gpu_tracks import _trained_model, _write_fasta

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _fixture(tmp_path):
    from deepgrp_amd import synthetic
    raw = synthetic.synthetic_chromosome(80_000, contig=2, flank=1000)
    rng = np.random.default_rng(5)
    recs = [(b"short some words", raw[1000:4000]), (b"NC_000001.11 long", b"NN" + raw[4000:64_000] + b"N"), (b"tiny", raw[64_000:64_700]),
            (b"random", rng.choice(list(b"ACGT"), size=5000).astype(np.uint8).tobytes())]
    fa = tmp_path / "in.fa"
    _write_fasta(fa, recs)
    return fa


@pytest.mark.parametrize("digits,width", [(2, 1), (3, 50), (3, 1), (2, 50)])
def test_cli_track_gzip_inflates_to_the_plain_tracks(tmp_path, digits, width):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    model_file, _T = _trained_model(tmp_path)
    fa = _fixture(tmp_path)
    tflags = ["--track_digits", str(digits), "--track_bin", str(width)]
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "none.tsv")])
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "plain.tsv"), "--track_dir", str(tmp_path / "plain")] + tflags)
    want_tsv = (tmp_path / "none.tsv").read_bytes()
    assert want_tsv.count(b"\n") > 3 and (tmp_path / "plain.tsv").read_bytes() == want_tsv
    names = [f"in.fa.class{c}.bedGraph" for c in (1, 2, 3, 4)]
    assert sorted(os.listdir(tmp_path / "plain")) == names
    sizes = {}
    for label, extra in (("default", []), ("level1", ["--gzip_level", "1"]), ("level0", ["--gzip_level", "0"])):
        tdir, tsv = tmp_path / label, tmp_path / f"{label}.tsv"
        argv = ["predict", model_file, str(fa), "--output", str(tsv), "--track_dir", str(tdir), "--track_gzip"] + tflags + extra
        if label == "level1":                                          # README form, the flags in front
            argv = ["--track_dir", str(tdir), "--track_gzip"] + tflags + extra + [model_file, str(fa), "--output", str(tsv)]
        main(argv)
        assert tsv.read_bytes() == want_tsv, label
        assert sorted(os.listdir(tdir)) == [n + ".gz" for n in names], label
        for n in names:
            comp, want = (tdir / (n + ".gz")).read_bytes(), (tmp_path / "plain" / n).read_bytes()
            m = gz.walk_members(comp)
            assert m.kind == "bgzf" and comp.endswith(gz.BGZF_EOF) and (m.isize[:-1] > 0).all(), (label, n)
            assert gzip.decompress(comp) == want, (label, n)
            sizes[label, n] = len(comp)
        if width == 1:                                                 # the long record's text is several members
            assert max(gz.walk_members((tdir / (names[0] + ".gz")).read_bytes()).isize) == BLOCK
    total = lambda label: sum(sizes[label, n] for n in names)
    assert total("default") == total("level1") <= total("level0")
    assert sum(os.path.getsize(tmp_path / "plain" / n) for n in names) > 3 * BLOCK or width > 1


def test_track_text_device_is_track_text(tmp_path):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd import synthetic
    from deepgrp_amd.pipeline import ContigPipeline, upload_sequence
    model_file, _T = _trained_model(tmp_path)
    pipe = ContigPipeline(dgmodel.load_model(model_file), 50, 256, 50, 50, use_mss=True)
    st, d_idx = upload_sequence(synthetic.synthetic_chromosome(20_000, contig=1, flank=500))
    merged = pipe.merged(d_idx)
    for c in (0, 2):
        d = pipe.track_text_device(merged, st, b"chr1", c, 2, 1)
        assert d.is_cuda and d.dtype == torch.uint8
        assert d.cpu().numpy().tobytes() == pipe.track_text(merged, st, b"chr1", c, 2, 1) != b""


def test_cli_track_gzip_failure_leaves_only_finished_inputs(tmp_path):
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    rng = np.random.default_rng(2)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    good, bad = tmp_path / "good.fa", tmp_path / "bad.fa"
    _write_fasta(good, [(b"g1", r(800)), (b"g2", r(300))])
    _write_fasta(bad, [(b"b1", r(700)), (b"allN", b"N" * 40), (b"b3", r(500))])
    tdir = tmp_path / "T"
    for vv in ([], ["-vv"]):
        with pytest.raises(ValueError, match="negative dimensions"):
            main(vv + ["predict", model_file, str(good), str(bad), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir), "--track_gzip"])
        main(["predict", model_file, str(good), "--output", str(tmp_path / "reset.tsv")])
        assert sorted(os.listdir(tdir)) == [f"good.fa.class{c}.bedGraph.gz" for c in (1, 2, 3, 4)], vv
        for c in (1, 2, 3, 4):
            os.remove(tdir / f"good.fa.class{c}.bedGraph.gz")


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_cli_mask_gzip_level_1(tmp_path, mode):
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    model_file, _T = _trained_model(tmp_path)
    fa = _fixture(tmp_path)
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "p.tsv"), "--mask_dir", str(tmp_path / "plain"), "--mask", mode])
    want = (tmp_path / "plain" / "in.fa").read_bytes()
    assert want != fa.read_bytes()
    sizes = {}
    for label, extra in (("default", []), ("level0", ["--gzip_level", "0"]), ("level1", ["--gzip_level", "1"])):
        main(["predict", model_file, str(fa), "--output", str(tmp_path / f"{label}.tsv"), "--mask_dir", str(tmp_path / label), "--mask", mode,
              "--mask_gzip"] + extra)
        comp = (tmp_path / label / "in.fa.gz").read_bytes()
        assert gz.walk_members(comp).kind == "bgzf" and comp.endswith(gz.BGZF_EOF)
        assert gzip.decompress(comp) == want, label
        assert (tmp_path / f"{label}.tsv").read_bytes() == (tmp_path / "p.tsv").read_bytes()
        sizes[label] = comp
    assert sizes["default"] == sizes["level0"] and len(sizes["level1"]) <= len(sizes["level0"])
