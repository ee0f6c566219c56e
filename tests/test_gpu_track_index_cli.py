"""predict --track_dir --track_gzip --track_index: every `.tbi` inflates to tabix.reference_index of its `.gz`, the reader finds what
a brute-force filter finds, the `.gz` files and the TSV are those of a run without the flag, a raising record leaves no index and
no temporary file, and an input whose names cannot be indexed gets a warning, its tracks and no index."""
import gzip
import logging
import os

import numpy as np
import pytest

from conftest import GOLDEN
from tabix_corpus import brute, parse, regions
from test_gpu_track_gzip import _fixture, _trained_model, _write_fasta

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("width,level", [(1, 1), (1, 0), (50, 1), (50, 0)])
def test_cli_track_index(tmp_path, width, level):
    from deepgrp_amd import gz, tabix
    from deepgrp_amd.__main__ import main
    model_file, _T = _trained_model(tmp_path)
    fa = _fixture(tmp_path)
    flags = ["--track_bin", str(width), "--gzip_level", str(level), "--track_gzip"]
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "plain.tsv"), "--track_dir", str(tmp_path / "plain")] + flags)
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "index.tsv"), "--track_dir", str(tmp_path / "index"), "--track_index"] + flags)
    assert (tmp_path / "index.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes() != b""
    names = [f"in.fa.class{c}.bedGraph.gz" for c in (1, 2, 3, 4)]
    assert sorted(os.listdir(tmp_path / "plain")) == names
    assert sorted(os.listdir(tmp_path / "index")) == sorted(names + [n + ".tbi" for n in names])
    found = 0
    for k, n in enumerate(names):
        comp = (tmp_path / "index" / n).read_bytes()
        assert comp == (tmp_path / "plain" / n).read_bytes()
        tbi = (tmp_path / "index" / (n + ".tbi")).read_bytes()
        assert gz.walk_members(tbi).kind == "bgzf" and tbi.endswith(gz.BGZF_EOF)
        pl = gzip.decompress(tbi)
        assert pl == tabix.reference_index(comp), n
        ix = tabix.read_index(pl)
        lines = parse(gzip.decompress(comp))
        assert ix["names"] == list(dict.fromkeys(nm for _l, nm, _s, _e in lines)) != []
        for nm, beg, end in regions(lines, seed=k, count=50)[:60]:
            got = tabix.query(ix, comp, nm, beg, end)
            assert got == brute(lines, nm, beg, end), (n, nm, beg, end)
            found += len(got)
    assert found > 0


def _random_fasta(path, names, seed=2, allN=None):
    rng = np.random.default_rng(seed)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    _write_fasta(path, [(nm, b"N" * 40 if nm == allN else r(500 + 100 * i)) for i, nm in enumerate(names)])


def test_cli_track_index_failure_leaves_no_index_and_no_temporary_file(tmp_path):
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    good, bad = tmp_path / "good.fa", tmp_path / "bad.fa"
    _random_fasta(good, [b"g1", b"g2"])
    _random_fasta(bad, [b"b1", b"allN", b"b3"], allN=b"allN")
    tdir = tmp_path / "T"
    for vv in ([], ["-vv"]):
        with pytest.raises(ValueError, match="negative dimensions"):
            main(vv + ["predict", model_file, str(good), str(bad), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir), "--track_gzip",
                       "--track_index"])
        main(["predict", model_file, str(good), "--output", str(tmp_path / "reset.tsv")])
        want = [f"good.fa.class{c}.bedGraph.gz" for c in (1, 2, 3, 4)]
        assert sorted(os.listdir(tdir)) == sorted(want + [n + ".tbi" for n in want]), vv
        for n in os.listdir(tdir):
            os.remove(tdir / n)


@pytest.mark.parametrize("names,word", [([b"a", b"b", b"a"], "reappears"), ([b"a", b"a", b"b", b"c"], None)])
def test_cli_a_name_that_returns_gets_a_warning_tracks_and_no_index(tmp_path, caplog, names, word):
    from deepgrp_amd import tabix
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    fa = tmp_path / "dup.fa"
    _random_fasta(fa, names, seed=3)
    tdir = tmp_path / "T"
    os.makedirs(tdir)
    stale = tdir / "dup.fa.class1.bedGraph.gz.tbi"
    stale.write_bytes(b"an index of an earlier run")
    with caplog.at_level(logging.WARNING):
        main(["predict", model_file, str(fa), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir), "--track_gzip", "--track_index"])
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "p.tsv"), "--track_dir", str(tmp_path / "P"), "--track_gzip"])
    gzs = [f"dup.fa.class{c}.bedGraph.gz" for c in (1, 2, 3, 4)]
    for n in gzs:
        assert (tdir / n).read_bytes() == (tmp_path / "P" / n).read_bytes()
    warned = [r.getMessage() for r in caplog.records if "no tabix index" in r.getMessage()]
    if word is None:                                                    # the same name twice in a row is one sequence
        assert warned == [] and sorted(os.listdir(tdir)) == sorted(gzs + [n + ".tbi" for n in gzs])
        for n in gzs:
            assert gzip.decompress((tdir / (n + ".tbi")).read_bytes()) == tabix.reference_index((tdir / n).read_bytes())
    else:
        assert len(warned) == 1 and word in warned[0] and "'a'" in warned[0] and "dup.fa" in warned[0]
        assert sorted(os.listdir(tdir)) == gzs                          # no index, no temporary file, and the stale one is gone
