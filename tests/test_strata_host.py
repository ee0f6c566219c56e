"""`evaluate --strata` on the CPU: the rule for the divergence token, the binning at every edge, both files byte for byte from fixed
counts, the command line's refusals before anything is loaded, the new symbols, and the numpy statements of the two device entries
against a slow loop per base."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rm_cases
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_H5 = os.path.join(GOLDEN, "model_u60_T342_att.h5")       # 5 classes
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


# ------------------------------------------------------------------------- the divergence of a line
@pytest.mark.parametrize("token,want", [("10.5", 105), ("0.0", 0), ("7", 70), ("7.", 70), ("12.34", 123), (".5", -1), ("-1.0", -1),
                                        ("1e1", -1), ("1234567.0", -1), ("999999.9", 9999999), ("12.3x", -1), ("+1", -1), ("1.2.3", -1),
                                        ("007.59", 75)])
def test_millidiv_of_an_out_line(token, want):
    from deepgrp_amd import annotation
    line = rm_cases.out_line().replace("10.5", token, 1)
    assert line.split()[1] == token
    assert annotation.millidiv_of_line(line) == want
    assert annotation.millidiv_of_line(line + "\n") == want


def test_millidiv_of_an_rmsk_line_and_of_no_line():
    from deepgrp_amd import annotation
    assert annotation.millidiv_of_line(rm_cases.rmsk_line()) == 13                      # field 2 of the corpus line
    f = rm_cases.rmsk_line().split("\t")
    for tok, want in (("0", 0), ("1234567", 1234567), ("12345678", -1), ("0000013", 13)):
        assert annotation.millidiv_of_line("\t".join(f[:2] + [tok] + f[3:])) == want
    for line in ("", "# a comment", "chr1 10 20 3 AluY SINE/Alu", "1 2 3", rm_cases.out_line(strand="-"), " " + rm_cases.rmsk_line()):
        assert annotation.millidiv_of_line(line) == -1
    # a line both patterns could claim is `.out`, as parse_rm.parse_line decides
    from deepgrp_amd._scripts import parse_rm
    line = rm_cases.out_line(sep="\t", lead="")
    assert parse_rm._OUT_LINE.match(line) and annotation.millidiv_of_line(line) == 105


def test_the_host_path_fills_millidiv_and_it_travels_with_the_rows(tmp_path):
    from deepgrp_amd import annotation
    lines = [rm_cases.out_line(ctg="chr2", begin=1, end=50).replace("10.5", "3.21", 1),
             rm_cases.out_line(ctg="chr1", begin=11, end=90, fam="LINE/L1").replace("10.5", "x", 1),
             rm_cases.out_line(ctg="chr1", fam="DNA/hAT"),
             rm_cases.rmsk_line(ctg="chr1", start=200, end=300),
             rm_cases.out_line(ctg="chr2", begin=100, end=500, fam="LINE/L2")]
    path = tmp_path / "x.out"
    path.write_bytes(rm_cases.text(lines))
    listing = annotation.read_listing(str(path), device=False)
    assert listing.route == "host" and listing.millidiv.dtype == np.int32
    assert listing.millidiv.tolist() == [32, -1, 13, 105]
    rows = annotation.evaluation_rows(str(path), [3, 4, 6], device=False)
    assert sorted(rows) == ["chr1", "chr2"]
    assert rows.millidiv["chr1"].tolist() == [-1, 13] and rows.millidiv["chr2"].tolist() == [32, 105]
    assert [len(rows.lines[k]) for k in sorted(rows)] == [2, 2]
    only = annotation.evaluation_rows(str(path), [6], device=False)                      # the same filter
    assert list(only) == ["chr2"] and only.millidiv["chr2"].tolist() == [105]
    assert annotation.Listing("p", [1], [2], [3], [1], [0, 1], ["c"], 1, "host").millidiv.tolist() == [-1]


# ------------------------------------------------------------------------- the binning
def test_bins_at_below_and_above_every_edge():
    from deepgrp_amd import strata
    div_edges, len_edges = (50, 100, 125, 300), (100, 300, 1000, 3000)
    for i, e in enumerate(div_edges):
        assert strata.div_bin([e - 1, e, e + 1], div_edges).tolist() == [i, i + 1, i + 1]
    assert strata.div_bin([0, 10 ** 7, -1], div_edges).tolist() == [0, len(div_edges), len(div_edges) + 1]
    for j, e in enumerate(len_edges):
        assert strata.len_bin([e - 1, e, e + 1], len_edges).tolist() == [j, j + 1, j + 1]
    assert strata.len_bin([0, 10 ** 9], len_edges).tolist() == [0, len(len_edges)]
    assert strata.div_labels(div_edges) == ["0-5", "5-10", "10-12.5", "12.5-30", "30+", "NA"]
    assert strata.len_labels(len_edges) == ["0-100", "100-300", "300-1000", "1000-3000", "3000+"]
    rows = np.zeros(4, SEG)
    rows["start"], rows["end"] = [0, 10, 5, 0], [99, 110, 3005, 300]                 # the row's own length, wherever its record ends
    got = strata.strata_of(rows, [49, 50, -1, 299], div_edges, len_edges)
    assert got.dtype == np.uint8 and got.tolist() == [0 * 5 + 0, 1 * 5 + 1, 5 * 5 + 4, 3 * 5 + 2]
    assert strata.strata_of(rows, None, div_edges, len_edges).tolist() == [25, 26, 29, 27]   # a table: NA everywhere


# ------------------------------------------------------------------------- the files
STRATA_TSV = """\
# element_bases and element_hits are sums over elements of the clipped length and of the hits: overlapping annotation rows count twice
#class\tdivergence\tlength\telements\tfound\trecall\telement_bases\telement_hits\tbase_recall
1\t0-10\t0-100\t4\t2\t0.5\t200\t50\t0.25
1\t0-10\t100+\t0\t0\tnan\t0\t0\tnan
1\t10+\t0-100\t1\t1\t1.0\t10\t10\t1.0
1\t10+\t100+\t0\t0\tnan\t0\t0\tnan
1\tNA\t0-100\t0\t0\tnan\t0\t0\tnan
1\tNA\t100+\t3\t0\t0.0\t900\t0\t0.0
1\t*\t0-100\t5\t3\t0.6\t210\t60\t0.2857142857142857
1\t*\t100+\t3\t0\t0.0\t900\t0\t0.0
1\t0-10\t*\t4\t2\t0.5\t200\t50\t0.25
1\t10+\t*\t1\t1\t1.0\t10\t10\t1.0
1\tNA\t*\t3\t0\t0.0\t900\t0\t0.0
1\t*\t*\t8\t3\t0.375\t1110\t60\t0.05405405405405406
"""

BASES_TSV = """\
#class\tdivergence\tlength\tthreshold\tTP\tFN\tTPR
1\t0-10\t0-100\t0.0\t7\t0\t1.0
1\t0-10\t0-100\t0.5\t4\t3\t0.5714285714285714
1\t0-10\t100+\t0.0\t0\t0\tnan
1\t0-10\t100+\t0.5\t0\t0\tnan
1\t10+\t0-100\t0.0\t2\t0\t1.0
1\t10+\t0-100\t0.5\t0\t2\t0.0
1\t10+\t100+\t0.0\t0\t0\tnan
1\t10+\t100+\t0.5\t0\t0\tnan
1\tNA\t0-100\t0.0\t0\t0\tnan
1\tNA\t0-100\t0.5\t0\t0\tnan
1\tNA\t100+\t0.0\t5\t0\t1.0
1\tNA\t100+\t0.5\t5\t0\t1.0
"""


def _fixed():
    from deepgrp_amd import strata
    st = strata.Strata(2, (100,), (100,), bins=2)
    assert (st.S, st.n_div, st.n_len) == (6, 3, 2)
    rows = np.zeros(8, SEG)
    rows["label"] = 1
    rows["end"] = [50, 50, 50, 50, 10, 300, 300, 300]
    md = [0, 99, 5, 7, 100, -1, -1, -1]
    sof = st.strata_of(rows, md)
    clen = np.array([50, 50, 50, 50, 10, 300, 300, 300])
    hits = np.array([25, 25, 0, 0, 10, 0, 0, 0])
    ok = np.ones(8, bool)
    st.count(rows["label"], sof, clen, hits, ok, hits * 2 >= clen)
    st.hist[1, 0], st.hist[1, 2], st.hist[1, 5] = [3, 4], [2, 0], [0, 5]
    return st


def test_both_files_byte_for_byte_and_the_json_key():
    from deepgrp_amd import strata
    st = _fixed()
    assert strata.strata_tsv(st.counts, st.div_edges, st.len_edges) == STRATA_TSV
    assert strata.bases_tsv(st.hist, st.div_edges, st.len_edges) == BASES_TSV
    s = st.summary()
    assert s["divergence_edges"] == [10.0] and s["length_edges"] == [100] and s["bins"] == 2
    assert s["divergence_bins"] == ["0-10", "10+", "NA"] and s["length_bins"] == ["0-100", "100+"]
    assert s["recall_by_divergence"] == [[None, None, None], [0.5, 1.0, 0.0]]
    assert s["recall_by_length"] == [[None, None], [0.6, 0.0]]


def test_rows_outside_their_record_are_not_elements():
    from deepgrp_amd import strata
    st = strata.Strata(3, (100,), (100,), bins=2)
    lab, sof = np.array([1, 2, 2]), np.array([0, 1, 1], np.uint8)
    st.count(lab, sof, np.array([10, 0, 7]), np.array([10, 0, 1]), np.array([True, False, True]), np.array([True, False, False]))
    assert st.counts[:, 1, 0].tolist() == [1, 1, 10, 10] and st.counts[:, 2, 1].tolist() == [1, 0, 7, 1]
    assert st.counts.sum() == 31


def test_write_stages_both_files(tmp_path):
    import logging

    from deepgrp_amd import strata
    st = _fixed()
    prefix = str(tmp_path / "run")
    p = strata.StrataPlan(prefix, st.div_edges, st.len_edges, 2, prefix + ".strata.tsv", prefix + ".strata.bases.tsv")
    st.write(p, logging.getLogger("t"))
    assert sorted(os.listdir(tmp_path)) == ["run.strata.bases.tsv", "run.strata.tsv"]
    assert (tmp_path / "run.strata.tsv").read_text() == STRATA_TSV and (tmp_path / "run.strata.bases.tsv").read_text() == BASES_TSV


# ------------------------------------------------------------------------- command line
def test_strata_flags_parse_and_plan(tmp_path):
    from deepgrp_amd import strata
    from deepgrp_amd.__main__ import CommandLineParser
    parse = lambda *f: CommandLineParser().parse_args(["evaluate", "m.h5", "ann.out", "a.fa", *f]).args
    d = parse()
    assert d.strata is None and d.strata_div is None and d.strata_len is None and d.strata_bins is None
    assert strata.plan(d) is None
    prefix = str(tmp_path / "hg38.v2")
    p = strata.plan(parse("--strata", prefix))
    assert p == strata.StrataPlan(prefix, (50, 100, 150, 200, 250, 300), (100, 300, 1000, 3000), 100, prefix + ".strata.tsv",
                                  prefix + ".strata.bases.tsv")
    p = strata.plan(parse("--strata", prefix, "--strata_div", "2.5,10", "--strata_len", "50", "--strata_bins", "1000"))
    assert (p.div_edges, p.len_edges, p.bins) == ((25, 100), (50,), 1000)
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--strata", "x"])             # on evaluate only
    fa = tmp_path / "hg38.v2.strata.tsv"
    fa.write_text(">x\nACGT\n")
    with pytest.raises(SystemExit) as e:
        strata.plan(CommandLineParser().parse_args(["evaluate", "m.h5", "ann.out", str(fa), "--strata", prefix]).args)
    assert "overwrite" in str(e.value)
    with pytest.raises(SystemExit) as e:                                                         # the annotation is an input too
        strata.plan(CommandLineParser().parse_args(["evaluate", "m.h5", str(fa), "a.fa", "--strata", prefix]).args)
    assert "overwrite" in str(e.value)


CHILD = ("import sys\n"
         "from deepgrp_amd.__main__ import main\n"
         "try:\n"
         "    main(sys.argv[1:])\n"
         "except SystemExit as e:\n"
         "    import deepgrp_amd._lib as l\n"
         "    print('LOADED' if (l._lib is not None or 'torch' in sys.modules or 'h5py' in sys.modules) else 'CLEAN')\n"
         "    raise\n")


def _child(tmp_path, *flags, env=None):
    ann = tmp_path / "a.bed"
    ann.write_text("chr1\t0\t10\t1\n")
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    return subprocess.run([sys.executable, "-c", CHILD, "evaluate", MODEL_H5, str(ann), str(tmp_path / "x.fa"), *flags], env=e,
                          capture_output=True, text=True, timeout=120, cwd=str(tmp_path))


SIXTEEN = ",".join(str(k) for k in range(1, 17))
FIFTEEN = ",".join(str(k) for k in range(1, 16))


@pytest.mark.parametrize("flags,words,env", [
    (["--strata_div", "5,10"], ["--strata_div needs --strata"], None),
    (["--strata_len", "100"], ["--strata_len needs --strata"], None),
    (["--strata_bins", "100"], ["--strata_bins needs --strata"], None),
    (["--strata", "sub/"], ["--strata", "prefix", "directory"], None),
    (["--strata", "sub"], ["--strata", "prefix", "directory"], None),
    (["--strata", "missing_dir/run"], ["--strata", "missing_dir", "does not exist"], None),
    (["--strata", "run"], ["WORLD_SIZE"], {"WORLD_SIZE": "2"}),
    (["--strata", "run", "--strata_div", FIFTEEN, "--strata_len", FIFTEEN], ["272 strata", "256"], None),
    (["--strata", "run", "--strata_div", SIXTEEN], ["--strata_div", "1..15"], None),
    (["--strata", "run", "--strata_len", SIXTEEN], ["--strata_len", "1..15"], None),
    (["--strata", "run", "--strata_div", "10,5"], ["--strata_div", "ascend"], None),
    (["--strata", "run", "--strata_div", "5,5"], ["--strata_div", "ascend"], None),
    (["--strata", "run", "--strata_div", "5.25"], ["--strata_div", "'5.25'"], None),
    (["--strata", "run", "--strata_len", "100,x"], ["--strata_len", "'x'"], None),
    (["--strata", "run", "--strata_len", "300,100"], ["--strata_len", "ascend"], None),
    (["--strata", "run", "--strata_bins", "1"], ["--strata_bins must lie in 2..1000, not 1"], None),
    (["--strata", "run", "--strata_bins", "1001"], ["--strata_bins must lie in 2..1000, not 1001"], None),
])
def test_refusals_come_before_the_model_is_read(tmp_path, flags, words, env):
    (tmp_path / "sub").mkdir()
    r = _child(tmp_path, *flags, env=env)
    assert r.returncode == 1, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert r.stdout.strip() == "CLEAN"
    assert sorted(os.listdir(tmp_path)) == ["a.bed", "sub"]


def test_an_output_that_is_an_input_is_refused_before_the_model_is_read(tmp_path):
    os.symlink(str(tmp_path / "a.bed"), str(tmp_path / "a.strata.bases.tsv"))      # the child's annotation under the output's name
    r = _child(tmp_path, "--strata", "a")
    assert r.returncode == 1 and "--strata" in r.stderr and "overwrite" in r.stderr and "a.bed" in r.stderr, r.stderr
    assert r.stdout.strip() == "CLEAN"
    assert (tmp_path / "a.bed").read_text() == "chr1\t0\t10\t1\n" and sorted(os.listdir(tmp_path)) == ["a.bed", "a.strata.bases.tsv"]


# ------------------------------------------------------------------------- the entries, without a GPU
def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_rm_parse_fields", "dgrp_paint_strata_batch", "dgrp_prob_hist_strata_batch", "dgrp_prob_hist_strata_workspace_bytes"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    assert _lib.lib().dgrp_abi_version() == 1                  # an addition: the version stays


# ------------------------------------------------------------------------- the numpy statements against a loop per base
def _small_world():
    rng = np.random.default_rng(5)
    lengths, origins = [120, 80], [1000, 0]
    rows, sof = [], []
    for n, o in zip(lengths, origins):
        k = 9
        r = np.zeros(k, SEG)
        r["start"] = rng.integers(max(o - 20, 0), o + n, k)
        r["end"] = r["start"] + rng.integers(0, 24, k)
        r["label"] = rng.integers(1, 4, k)
        r[3] = r[2]                                                   # equal rows ...
        rows.append(r)
        s = rng.integers(0, 6, k).astype(np.uint8)
        s[3] = 5 - s[2]                                               # ... of one label with different strata
        sof.append(s)
    return lengths, origins, rows, sof


def test_reference_keys_against_a_loop_per_base():
    from deepgrp_amd import strata
    lengths, origins, rows, sof = _small_world()
    got = strata.reference_keys(origins, lengths, rows, sof)
    assert sum(lengths) == 200
    for r in range(2):
        want = np.full(lengths[r], 0xFFFFFFFF, np.uint32)
        for b in range(lengths[r]):
            x = origins[r] + b
            covering = [(int(q["label"]) << 8) | int(s) for q, s in zip(rows[r], sof[r]) if q["start"] <= x < q["end"]]
            if covering:
                want[b] = min(covering)
        assert got[r].dtype == np.uint32 and np.array_equal(got[r], want)
        assert (want != 0xFFFFFFFF).any() and (want == 0xFFFFFFFF).any()


def test_reference_strata_hist_against_a_loop_per_base():
    from deepgrp_amd import strata
    lengths, origins, rows, sof = _small_world()
    keys = np.concatenate(strata.reference_keys(origins, lengths, rows, sof))
    rng = np.random.default_rng(6)
    C, S, bins = 4, 6, 10
    probs = rng.random((200, C), dtype=np.float32)
    live = np.flatnonzero(keys != 0xFFFFFFFF)
    special = [0.0, 1.0, -0.0, np.nextafter(np.float32(0.3), np.float32(0)), 0.3, np.nan, 1.5, -0.25]
    for b, v in zip(live, special):
        probs[b, keys[b] >> 8] = v
    probs[keys == 0xFFFFFFFF] = np.nan                                # never read: no key, no count and no flag
    want, flag = np.zeros((C, S, bins), np.int64), 0
    for b in range(200):
        if keys[b] == 0xFFFFFFFF:
            continue
        t, s = int(keys[b]) >> 8, int(keys[b]) & 255
        p = probs[b, t]
        if not (p >= 0 and p <= 1):
            flag = 1
            continue
        want[t, s, min(bins - 1, int(np.float32(p) * np.float32(bins)))] += 1
    got, got_flag = strata.reference_strata_hist(probs, keys, S, bins)
    assert np.array_equal(got, want) and got_flag == flag == 1
    assert want.sum() == live.size - 3
    clean = np.where(np.isnan(probs) | (probs > 1) | (probs < 0), np.float32(0.5), probs)
    assert strata.reference_strata_hist(clean, keys, S, bins)[1] == 0
    # a stratum or a class outside the table raises the flag and is not counted
    h, f = strata.reference_strata_hist(clean, keys, 3, bins)
    assert f == 1 and h.sum() == ((keys != 0xFFFFFFFF) & ((keys & 255) < 3)).sum()
    h, f = strata.reference_strata_hist(clean[:, :2], keys, S, bins)
    assert f == 1 and h.sum() == ((keys != 0xFFFFFFFF) & ((keys >> 8) < 2)).sum()
