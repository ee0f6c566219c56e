"""`evaluate --offtarget` on the CPU: the host statement of a listing's ALL rows and their family ids, both files byte for byte from
fixed counts, the `class` fold, the command line's refusals before the model is read, the new symbols, and the numpy statements of
the device entries against a slow loop per base."""
import gzip
import os

import numpy as np
import pytest

import rm_cases
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------------- the host statement of all rows
def _check_all_rows(path, data: bytes):
    """The all-rows listing of `path` against parse_rm itself, line by line; -> the listing."""
    import io

    from deepgrp_amd import annotation
    from deepgrp_amd._scripts import parse_rm
    every = annotation.read_listing(path, device=False, all_rows=True)
    numbered = annotation._listing_host(path)
    assert every.route == "host" and every.family_id.dtype == np.int32 and len(every.family_id) == len(every)
    keep = every.number > 0
    for k in ("begin", "end", "number", "line", "millidiv"):                     # the rows with a number are exactly _listing_host's
        assert np.array_equal(getattr(every, k)[keep], getattr(numbered, k)), k
    names, cid = every.contigs()
    n_names, n_cid = numbered.contigs()
    assert [names[i] for i in cid[keep]] == [n_names[i] for i in n_cid]
    lines = io.StringIO(data.decode("utf-8"), newline=None).read().split("\n")
    matching = [(k + 1, parse_rm.parse_line(line)) for k, line in enumerate(lines)]
    matching = [(k, r) for k, r in matching if r.ctg is not None]
    assert every.line.tolist() == [k for k, _r in matching]
    assert [every.families[i] for i in every.family_id] == [r.fam for _k, r in matching]
    assert [names[i] for i in cid] == [r.ctg for _k, r in matching]
    raw = [f.encode() for f in every.families]
    assert raw == sorted(set(raw)) and len(raw) == len(set(r.fam for _k, r in matching))
    return every


@pytest.mark.parametrize("name,data", rm_cases.cases(32768) + rm_cases.fallback_cases()[:1], ids=lambda c: c if isinstance(c, str) else "")
def test_all_rows_of_the_corpus(tmp_path, name, data):
    path = tmp_path / "case.out"
    path.write_bytes(data)
    every = _check_all_rows(str(path), data)
    if name == "skipped_only":
        assert len(every) == 1 and every.number.tolist() == [0] and every.families == ["DNA/hAT"]


def test_all_rows_of_the_golden_listing(tmp_path):
    from deepgrp_amd import annotation
    gz = os.path.join(GOLDEN, "parse_rm_input.out.gz")
    data = gzip.open(gz).read()
    every = _check_all_rows(gz, data)
    expect = [line.split("\t") for line in open(os.path.join(GOLDEN, "parse_rm_expect.bed")).read().splitlines()]
    keep = every.number > 0
    assert every.begin[keep].tolist() == [int(f[1]) for f in expect] and every.number[keep].tolist() == [int(f[3]) for f in expect]
    assert len(every) >= keep.sum()
    rows = annotation.evaluation_rows(gz, [1, 2, 3, 4], device=False, offtarget=True)
    plain = annotation.evaluation_rows(gz, [1, 2, 3, 4], device=False)
    assert sorted(rows) == sorted(plain) and all(rows[k].tobytes() == plain[k].tobytes() for k in plain)
    assert sum(len(v) for v in rows.values()) + sum(len(v) for v in rows.offtarget_rows.values()) == len(every)
    assert rows.families == every.families


def test_rmsk_and_out_spellings_share_an_id_and_a_prefix_sorts_first(tmp_path):
    from deepgrp_amd import annotation
    lines = [rm_cases.rmsk_line(cls="LINE", fam="L2"), rm_cases.out_line(fam="LINE/L2"),
             rm_cases.rmsk_line(rep="x", cls="Satellite", fam="Satellite"), rm_cases.out_line(rep="x", fam="Satellite"),
             rm_cases.out_line(rep="x", fam="LINE"), rm_cases.out_line(rep="x", fam="LINE/"), rm_cases.out_line(rep="x", fam="LINE/L"),
             rm_cases.out_line(rep="x", fam="LINE0"), rm_cases.rmsk_line(rep="x", cls="LINE", fam="L"), rm_cases.out_line(rep="x", fam="DNA/hAT-Charlie"),
             rm_cases.out_line(ctg="chr2", begin=5, end=3, rep="x", fam="DNA/hAT")]
    path = tmp_path / "x.out"
    path.write_bytes(rm_cases.text(lines))
    every = annotation.read_listing(str(path), device=False, all_rows=True)
    assert every.families == ["DNA/hAT", "DNA/hAT-Charlie", "LINE", "LINE/", "LINE/L", "LINE/L2", "LINE0", "Satellite"]
    fid = every.family_id.tolist()
    assert fid[0] == fid[1] == 5 and fid[2] == fid[3] == 7 and fid[4:9] == [2, 3, 4, 6, 4] and every.number.tolist()[:2] == [6, 6]
    ids, names = annotation.family_ranks(["b", "a/b", "a", "a/", "a", "B"])
    assert names == ["B", "a", "a/", "a/b", "b"] and ids.tolist() == [4, 3, 1, 2, 1, 0]
    # the checks now apply to every row: the un-modelled row with its end below its begin is named with the listing's line
    from deepgrp_amd.evaluation import AnnotationError
    assert "chr2" not in annotation.evaluation_rows(str(path), [6], device=False)
    with pytest.raises(AnnotationError) as e:
        annotation.evaluation_rows(str(path), [6], device=False, offtarget=True)
    assert f"{path}:11: end below begin" in str(e.value)


def test_modelled_and_unmodelled_rows_and_their_keys(tmp_path):
    from deepgrp_amd import annotation
    lines = [rm_cases.out_line(ctg="chr1", begin=1, end=50, fam="SINE/Alu"), rm_cases.out_line(ctg="chr1", begin=11, end=90, fam="LINE/L2"),
             rm_cases.out_line(ctg="chr1", begin=101, end=190, rep="x", fam="DNA/hAT"), rm_cases.out_line(ctg="#c", begin=1, end=9),
             rm_cases.out_line(ctg="chr2", begin=7, end=9, rep="x", fam="Unknown")]
    path = tmp_path / "x.out"
    path.write_bytes(rm_cases.text(lines))
    rows = annotation.evaluation_rows(str(path), [3, 4], device=False, offtarget=True)
    assert sorted(rows) == ["chr1"] and rows["chr1"]["label"].tolist() == [3]
    assert rows.families == ["DNA/hAT", "LINE/L2", "SINE/Alu", "Unknown"]
    assert sorted(rows.offtarget_rows) == ["#c", "chr1", "chr2"]
    assert rows.offtarget_rows["chr1"]["label"].tolist() == [6, 0] and rows.offtarget_rows["chr1"]["start"].tolist() == [10, 100]
    assert rows.offtarget_keys["chr1"].dtype == np.uint32 and rows.offtarget_keys["chr1"].tolist() == [64 + 1, 64 + 0]
    assert rows.offtarget_keys["#c"].tolist() == [64 + 2] and rows.offtarget_keys["chr2"].tolist() == [64 + 3]
    assert rows.lines["chr1"].tolist() == [1] and rows.millidiv["chr1"].tolist() == [105]


# ------------------------------------------------------------------------- the files, from fixed counts
FAMILIES = ["DNA/hAT", "LINE/CR1", "LINE/L2", "SINE/MIR"]


def _fixed():
    hist = np.zeros((2, 3, 64 + 4 + 1), np.int64)
    hist[0, 0, [1, 2, 64, 66, 68]] = [5, 7, 100, 100, 1000]
    hist[0, 1, [1, 2, 65, 66, 67, 68]] = [60, 3, 10, 20, 7, 0]
    hist[0, 2, [2, 68]] = [9, 1]
    hist[1, 1, [2, 65, 66, 67]] = [3, 10, 20, 7]
    hist[1, 2, [68]] = [1]
    return hist


def test_the_table_byte_for_byte():
    from deepgrp_amd import offtarget
    text = offtarget.offtarget_tsv(_fixed(), FAMILIES, "family")
    head, body = text.split("\n", 1)
    assert head.startswith("# ") and "smallest key" in head and "byte order" in head and "\n" not in head
    assert body == ("scope\tpredicted\tunder\tbases\tshare\n"
                    "all\t0\tnone\t1000\t0.825083\n" "all\t0\tDNA/hAT\t100\t0.082508\n" "all\t0\tLINE/L2\t100\t0.082508\n"
                    "all\t0\tclass2\t7\t0.005776\n" "all\t0\tclass1\t5\t0.004125\n"
                    "all\t1\tclass1\t60\t0.600000\n" "all\t1\tLINE/L2\t20\t0.200000\n" "all\t1\tLINE/CR1\t10\t0.100000\n"
                    "all\t1\tSINE/MIR\t7\t0.070000\n" "all\t1\tclass2\t3\t0.030000\n"
                    "all\t2\tclass2\t9\t0.900000\n" "all\t2\tnone\t1\t0.100000\n"
                    "unsupported\t1\tLINE/L2\t20\t0.500000\n" "unsupported\t1\tLINE/CR1\t10\t0.250000\n" "unsupported\t1\tSINE/MIR\t7\t0.175000\n"
                    "unsupported\t1\tclass2\t3\t0.075000\n"
                    "unsupported\t2\tnone\t1\t1.000000\n")


def test_the_class_fold():
    from deepgrp_amd import offtarget
    assert offtarget.fold(["LINE/L2", "LINE/CR1", "Unknown", "DNA/hAT/x"], "class") == ["LINE", "LINE", "Unknown", "DNA"]
    assert offtarget.fold(["LINE/L2"], "family") == ["LINE/L2"]
    body = offtarget.offtarget_tsv(_fixed(), FAMILIES, "class").split("\n", 1)[1]
    assert ("all\t1\tclass1\t60\t0.600000\n" "all\t1\tLINE\t30\t0.300000\n" "all\t1\tSINE\t7\t0.070000\n" "all\t1\tclass2\t3\t0.030000\n") in body
    assert "unsupported\t1\tLINE\t30\t0.750000\n" in body and "LINE/" not in body and "all\t0\tDNA\t100\t0.082508\n" in body
    with pytest.raises(ValueError):
        offtarget.offtarget_tsv(_fixed(), FAMILIES[:3], "family")


def test_the_rows_file_and_the_summary():
    from deepgrp_amd import offtarget
    ot = offtarget.Offtarget(3, FAMILIES)
    assert ot.K == 69 and ot.hist.shape == (2, 3, 69)
    labels = np.array([1, 1, 1, 2, 2, 1, 2, 1])
    kept = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    good = np.array([1, 0, 0, 0, 0, 0, 0, 0], bool)
    cls = np.array([[9, 0, 0, 0], [4, 4, 1, 0], [0, 2, 5, 5], [0, 0, 0, 7], [1, 1, 1, 1], [0, 3, 2, 0], [0, 0, 8, 8], [0, 0, 0, 0]])
    ot.count_rows(labels, kept, good, cls)
    assert ot.rows.tolist() == [[0] * 6, [4, 1, 1, 1, 1, 0], [3, 0, 1, 0, 1, 1]]
    assert (ot.rows[:, 2:].sum(axis=1) == ot.rows[:, 0] - ot.rows[:, 1]).all()
    assert offtarget.rows_tsv(ot.rows) == ("class\trows\tsupported\tmostly_own\tmostly_other_class\tmostly_offtarget\tmostly_unannotated\n"
                                          "1\t4\t1\t1\t1\t1\t0\n" "2\t3\t0\t1\t0\t1\t1\n")
    ot.hist += _fixed()
    s = ot.summary()
    assert s["by"] == "family" and s["families"] == 4 and len(s["classes"]) == 3
    assert s["classes"][1] == dict(unsupported_bases=40, modelled=0.075, offtarget=0.925, unannotated=0.0,
                                   top=[["LINE/L2", 20], ["LINE/CR1", 10], ["SINE/MIR", 7]])
    assert s["classes"][0]["modelled"] is None and s["classes"][2]["top"] == [] and s["classes"][2]["unannotated"] == 1.0
    import json
    json.dumps(s, allow_nan=False)


def test_write_stages_both_files(tmp_path):
    import logging

    from deepgrp_amd import offtarget
    ot = offtarget.Offtarget(3, FAMILIES, "class")
    ot.hist += _fixed()
    p = offtarget.OfftargetPlan(str(tmp_path / "run"), "class", str(tmp_path / "run.offtarget.tsv"), str(tmp_path / "run.offtarget.rows.tsv"))
    ot.write(p, logging.getLogger("test"))
    assert sorted(os.listdir(tmp_path)) == ["run.offtarget.rows.tsv", "run.offtarget.tsv"]
    assert (tmp_path / "run.offtarget.tsv").read_text() == offtarget.offtarget_tsv(_fixed(), FAMILIES, "class")


# ------------------------------------------------------------------------- the refusals
def _refused(monkeypatch, tmp_path, flags, ann=None, env=None):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import main

    def never(*a, **k):
        raise AssertionError("the model was read before the refusal")
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", never)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if ann is None:
        ann = tmp_path / "rm.out"
        ann.write_bytes(rm_cases.text([rm_cases.out_line()]))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        main(["evaluate", "model.hdf5", str(ann), str(tmp_path / "x.fa")] + flags)
    return str(e.value)


@pytest.mark.parametrize("flags,words,env", [
    (["--offtarget_by", "class"], ["--offtarget_by needs --offtarget"], None),
    (["--offtarget", "sub/"], ["--offtarget", "prefix", "directory"], None),
    (["--offtarget", "sub"], ["--offtarget", "prefix", "directory"], None),
    (["--offtarget", "missing_dir/run"], ["--offtarget", "missing_dir", "does not exist"], None),
    (["--offtarget", "run"], ["WORLD_SIZE"], {"WORLD_SIZE": "2"}),               # (evaluate's own refusal comes first)
])
def test_refusals_come_before_the_model_is_read(monkeypatch, tmp_path, flags, words, env):
    (tmp_path / "sub").mkdir()
    said = _refused(monkeypatch, tmp_path, flags, env=env)
    assert all(w in said for w in words), said
    assert sorted(os.listdir(tmp_path)) == ["rm.out", "sub"]


def test_an_output_that_is_an_input_and_the_table_form_are_refused(monkeypatch, tmp_path):
    ann = tmp_path / "rm.out"
    ann.write_bytes(rm_cases.text([rm_cases.out_line()]))
    os.symlink(str(ann), str(tmp_path / "a.offtarget.rows.tsv"))
    said = _refused(monkeypatch, tmp_path, ["--offtarget", "a"], ann=ann)
    assert "--offtarget" in said and "overwrite" in said and "rm.out" in said
    table = tmp_path / "a.bed"
    table.write_text("chr1\t0\t10\t1\n")
    said = _refused(monkeypatch, tmp_path, ["--offtarget", "run"], ann=table)
    assert "--offtarget" in said and "table" in said and "modelled classes only" in said and "genome.fa.out" in said and "rmsk.txt.gz" in said
    said = _refused(monkeypatch, tmp_path, ["--offtarget", "run", "--annotation_format", "table"], ann=ann)
    assert "table" in said and "modelled classes only" in said
    assert not [f for f in os.listdir(tmp_path) if f.startswith("run")]


def test_the_flags_belong_to_evaluate(monkeypatch, tmp_path):
    from deepgrp_amd import offtarget
    from deepgrp_amd.__main__ import CommandLineParser
    args = CommandLineParser().parse_args(["evaluate", "m.h5", "a.out", "a.fa"]).args
    assert args.offtarget is None and args.offtarget_by is None and offtarget.plan(args) is None
    ann = tmp_path / "rm.out"
    ann.write_bytes(rm_cases.text([rm_cases.out_line()]))
    args = CommandLineParser().parse_args(["evaluate", "m.h5", str(ann), "a.fa", "--offtarget", str(tmp_path / "run"), "--offtarget_by", "class"]).args
    p = offtarget.plan(args)
    assert p.by == "class" and p.table_path.endswith("run.offtarget.tsv") and p.rows_path.endswith("run.offtarget.rows.tsv")
    monkeypatch.setenv("WORLD_SIZE", "2")                                         # the plan's own refusal, for a caller other than the command
    with pytest.raises(SystemExit) as e:
        offtarget.plan(args)
    assert "--offtarget" in str(e.value) and "WORLD_SIZE" in str(e.value)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--offtarget", "x"])
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["evaluate", "m.h5", "a.out", "a.fa", "--offtarget", "x", "--offtarget_by", "name"])


# ------------------------------------------------------------------------- the entries, without a GPU
def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_rm_parse_all", "dgrp_rm_parse_all_workspace_bytes", "dgrp_token_ids", "dgrp_token_ids_workspace_bytes",
                 "dgrp_paint_keys_batch", "dgrp_key_crosstab_batch", "dgrp_row_key_classes_batch"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    L = _lib.lib()
    assert L.dgrp_abi_version() == 1                           # an addition: the version stays
    for n in (0, 1, 32768, 10 ** 7):                           # the companions: the all-rows parse needs what the parse needs
        assert L.dgrp_rm_parse_all_workspace_bytes(n) == L.dgrp_rm_parse_workspace_bytes(n) > 0
    assert L.dgrp_token_ids_workspace_bytes(1000, 1 << 20) > 65536 * 8 + (1 << 20) and L.dgrp_token_ids_workspace_bytes(-1, 0) == 0
    assert "#define DGRP_TOKEN_SLOTS 65536" in header and "#define DGRP_TOKEN_MAX 16384" in header


# ------------------------------------------------------------------------- the numpy statements against a loop per base
def _small_world():
    rng = np.random.default_rng(5)
    lengths, origins = [120, 80], [1000, 0]
    rows, keys = [], []
    for n, o in zip(lengths, origins):
        k = 11
        r = np.zeros(k, SEG)
        r["start"] = rng.integers(max(o - 20, 0), o + n, k)
        r["end"] = r["start"] + rng.integers(0, 24, k)
        key = np.where(rng.random(k) < 0.4, rng.integers(1, 4, k), 64 + rng.integers(0, 5, k)).astype(np.uint32)
        r["label"] = np.where(key < 64, key, 0)
        r[3] = r[2]                                                   # equal rows with different keys
        key[3] = 64 + 4 - (key[2] % 4)
        rows.append(r)
        keys.append(key)
    return lengths, origins, rows, keys


def test_reference_keys_against_a_loop_per_base():
    from deepgrp_amd import offtarget
    lengths, origins, rows, keys = _small_world()
    got = offtarget.reference_keys(origins, lengths, rows, keys)
    for r in range(2):
        want = np.full(lengths[r], NONE, np.uint32)
        for b in range(lengths[r]):
            x = origins[r] + b
            covering = [int(k) for q, k in zip(rows[r], keys[r]) if q["start"] <= x < q["end"]]
            if covering:
                want[b] = min(covering)
        assert got[r].dtype == np.uint32 and np.array_equal(got[r], want)
        assert (want == NONE).any() and (want < 64).any() and ((want >= 64) & (want != NONE)).any()


def test_reference_crosstab_and_row_classes_against_a_loop_per_base():
    from deepgrp_amd import offtarget
    lengths, origins, rows, keys = _small_world()
    track = np.concatenate(offtarget.reference_keys(origins, lengths, rows, keys))
    rng = np.random.default_rng(8)
    C, F = 4, 5
    K = 64 + F + 1
    pred = rng.integers(0, C, track.size).astype(np.int8)
    want = np.zeros((C, K), np.int64)
    for p, k in zip(pred, track):
        want[p, K - 1 if k == NONE else int(k)] += 1
    got, flag = offtarget.reference_crosstab(pred, track, C, K)
    assert np.array_equal(got, want) and flag == 0 and got.sum() == 200 and got[:, 0].sum() == 0
    spoiled_p, spoiled_k = pred.copy(), track.copy()
    spoiled_p[3], spoiled_p[4], spoiled_k[10], spoiled_k[11] = C, -1, K - 1, K
    got, flag = offtarget.reference_crosstab(spoiled_p, spoiled_k, C, K)
    assert flag == 1 and got.sum() == 196
    for lab in (1, 2, 3):
        span = track[30:170]
        want4 = [sum(1 for k in span if k == lab), sum(1 for k in span if k < 64 and k != lab), sum(1 for k in span if 64 <= k < NONE),
                 sum(1 for k in span if k == NONE)]
        assert offtarget.reference_row_classes(span, lab).tolist() == want4 and sum(want4) == 140
    assert offtarget.reference_row_classes(track[:0], 1).tolist() == [0, 0, 0, 0]
