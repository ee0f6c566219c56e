"""predict --track_dir --track_bigwig on the small golden models: every `.bw` states what the `.bedGraph` of the same flags states
(items, total summary and zoom levels restated from the lines), the TSV is that of a run without the flag, in the batched loop and in
the staged one of -vv, at both levels; an input with a duplicate name gets a warning and no `.bw`."""
import logging
import os

import numpy as np
import pytest

from bigwig_reader import BigWig
from conftest import GOLDEN
from test_gpu_track_gzip import _fixture, _trained_model, _write_fasta

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _lines(text):
    """[(name, start, end, decimal text)] of a bedGraph."""
    return [(nm, int(s), int(e), v) for nm, s, e, v in (ln.split(b"\t") for ln in text.split(b"\n")[:-1])]


def _restate(lines, ids, digits, width, longest):
    """Items, total summary and zoom levels of a bigWig from the lines of the bedGraph: integers from the decimal text, one division."""
    scale = 10 ** digits
    q = [int(v.replace(b".", b"")) for _nm, _s, _e, v in lines]
    items = [(ids[nm], s, e, np.float32(np.float64(x) / np.float64(scale))) for (nm, s, e, _v), x in zip(lines, q)]
    bases = sum(e - s for _nm, s, e, _v in lines)
    s1 = sum(x * (e - s) for (_nm, s, e, _v), x in zip(lines, q))
    s2 = sum(x * x * (e - s) for (_nm, s, e, _v), x in zip(lines, q))
    summary = (bases, min(q) / scale, max(q) / scale, s1 / scale, s2 / scale ** 2) if lines else (0, 0.0, 0.0, 0.0, 0.0)
    zooms = []
    for k in range(10):
        red = 16 * width * 4 ** k
        if red >= longest or not lines:
            break
        wins = {}                                                          # (chrom, window) -> [start, end, valid, qmin, qmax, s1, s2]
        for (nm, s, e, _v), x in zip(lines, q):
            for w in range(s // red, (e - 1) // red + 1):
                a, b = max(s, w * red), min(e, (w + 1) * red)
                t = wins.setdefault((ids[nm], w), [a, b, 0, x, x, 0, 0])
                t[1], t[2], t[3], t[4], t[5], t[6] = b, t[2] + b - a, min(t[3], x), max(t[4], x), t[5] + x * (b - a), t[6] + x * x * (b - a)
        f = lambda x, d: np.float32(np.float64(x) / np.float64(d))
        zooms.append((red, [(c, t[0], t[1], t[2], f(t[3], scale), f(t[4], scale), f(t[5], scale), f(t[6], scale * scale))
                            for (c, _w), t in sorted(wins.items())]))
    return items, summary, zooms


@pytest.mark.parametrize("width,level,vv", [(1, 1, False), (50, 0, False), (1, 1, True), (50, 1, True)])
def test_cli_bigwig_states_what_the_bedgraph_states(tmp_path, width, level, vv):
    from deepgrp_amd.__main__ import main
    model_file, _T = _trained_model(tmp_path)
    fa = _fixture(tmp_path)
    flags = ["--track_bin", str(width), "--track_digits", "3"]
    pre = ["-vv"] if vv else []
    main(pre + ["predict", model_file, str(fa), "--output", str(tmp_path / "plain.tsv"), "--track_dir", str(tmp_path / "plain")] + flags)
    main(pre + ["predict", model_file, str(fa), "--output", str(tmp_path / "bw.tsv"), "--track_dir", str(tmp_path / "bw"), "--track_bigwig",
                "--gzip_level", str(level)] + flags)
    assert (tmp_path / "bw.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes() != b""
    assert sorted(os.listdir(tmp_path / "bw")) == [f"in.fa.class{c}.bw" for c in (1, 2, 3, 4)]
    names = [b"short", b"NC_000001.11", b"tiny", b"random"]
    ids = {nm: i for i, nm in enumerate(names)}
    bodies = [b"".join(rec.split(b"\n")[1:]) for rec in fa.read_bytes().split(b">")[1:]]
    sizes = [len(body.rstrip(b"Nn")) for body in bodies]                    # startpos + n: the end of the predicted span
    assert len(sizes) == 4 and sizes[1] == 60_002
    seen = 0
    for c in (1, 2, 3, 4):
        r = BigWig((tmp_path / "bw" / f"in.fa.class{c}.bw").read_bytes())
        lines = _lines((tmp_path / "plain" / f"in.fa.class{c}.bedGraph").read_bytes())
        assert sorted(r.chroms, key=lambda x: x[1]) == [(nm, i, sizes[i]) for i, nm in enumerate(names)]
        for i, nm in enumerate(names):
            assert r.find_chrom(nm) == (i, sizes[i])
        items, summary, zooms = _restate(lines, ids, 3, width, max(sizes))
        got_items, got_zooms = r.check_all()
        assert got_items == items and r.summary == summary, c
        assert r.nzoom == len(zooms) and got_zooms == zooms, c
        if items:
            mid = items[len(items) // 2]
            assert mid in r.query(mid[0], mid[1], mid[2]) and r.query(mid[0], mid[1], mid[1] + 1)[0] == mid
        seen += len(items)
    assert seen > 100


def test_cli_a_duplicate_name_gets_a_warning_no_bigwig_and_the_same_tsv(tmp_path, caplog):
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    rng = np.random.default_rng(3)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    good, dup = tmp_path / "good.fa", tmp_path / "dup.fa"
    _write_fasta(good, [(b"g1", r(600)), (b"g2", r(500))])
    _write_fasta(dup, [(b"a", r(500)), (b"b", r(600)), (b"a", r(700))])
    tdir = tmp_path / "T"
    os.makedirs(tdir)
    (tdir / "dup.fa.class1.bw").write_bytes(b"left by an earlier run")
    main(["predict", model_file, str(good), str(dup), "--output", str(tmp_path / "plain.tsv")])
    with caplog.at_level(logging.WARNING):
        main(["predict", model_file, str(good), str(dup), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir), "--track_bigwig"])
    assert (tmp_path / "o.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes()
    warned = [x.getMessage() for x in caplog.records if "no bigWig" in x.getMessage()]
    assert len(warned) == 1 and "dup.fa" in warned[0] and "two records have the name 'a'" in warned[0]
    assert sorted(os.listdir(tdir)) == [f"good.fa.class{c}.bw" for c in (1, 2, 3, 4)]      # the other input has its files; no temporary file
    for n in os.listdir(tdir):
        assert [k for k, _i, _s in BigWig((tdir / n).read_bytes()).chroms] == [b"g1", b"g2"]
