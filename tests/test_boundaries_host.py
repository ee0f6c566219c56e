"""`evaluate --boundaries` on the CPU: the numpy statements of the two device entries against a loop per base, the offset rule at
its corners, --boundary_join at its gap, both files byte for byte and the JSON figures from fixed counts, the command line's refusals
before the model is read, and the new symbols."""
import json
import os

import numpy as np
import pytest

import rm_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


def _segs(rows):
    a = np.zeros(len(rows), SEG)
    for i, r in enumerate(rows):
        a[i] = tuple(r) + (0,) * (4 - len(r))
    return a


# ------------------------------------------------------------------------- the numpy statements against a loop per base
def _loop_bounds(o, n, track, q, W):
    """One row by the words of the header: a loop per base."""
    L = int(q["label"])
    a, e = min(max(int(q["start"]), o), o + n), min(max(int(q["end"]), o), o + n)
    inside = lambda b: o <= b < o + n and int(track[b - o]) == L
    if e <= a:
        return (0, 0, -1, -1, 0, 0)
    matched = [b for b in range(a, e) if inside(b)]
    runs = sum(1 for b in matched if b == a or not inside(b - 1))
    lead = 0
    while lead < min(W, a - o) and inside(a - lead - 1):
        lead += 1
    trail = 0
    while trail < min(W, o + n - e) and inside(e + trail):
        trail += 1
    return (len(matched), runs, matched[0] if matched else -1, matched[-1] if matched else -1, lead, trail)


def _world(seed, lengths, origins, count=40):
    rng = np.random.default_rng(seed)
    tracks, rows = [], []
    for n, o in zip(lengths, origins):
        t = np.zeros(n, np.int8)
        i = 0
        while i < n:                                                       # runs of 1..12 bases of the labels 0..3
            k = int(rng.integers(1, 13))
            t[i:i + k] = int(rng.integers(0, 4))
            i += k
        q = np.zeros(count + 10, SEG)
        q["start"][:count] = rng.integers(max(o - 10, 0), o + n + 5, count)
        q["end"][:count] = q["start"][:count] + rng.integers(0, max(n // 2, 2), count)
        q["label"][:count] = rng.integers(1, 4, count)
        lab = int(t[0]) or 1
        q[count:] = _segs([(o, o + 1, lab), (o + n - 1, o + n, int(t[-1]) or 2), (max(o - 7, 0), o + n + 9, 1), (o + n + 3, o + n + 30, 2),
                           (0, max(o - 1, 0), 3), (o + n // 2, o + n // 2, 1), (o, o + n, 2), (o, o + n, 3),
                           (max(o - 3, 0), o + 1, lab), (o + n - 1, o + n + 2, int(t[-1]) or 2)])       # found, one side clipped
        tracks.append(t)
        rows.append(q)
    return tracks, rows


@pytest.mark.parametrize("W", [0, 1, 5, 200, 4096])
def test_reference_bounds_against_a_loop_per_base(W):
    from deepgrp_amd import boundaries
    lengths, origins = [97, 1, 40, 2], [1000, 5, 0, 77]                      # W = 200 and 4096 exceed every record
    tracks, rows = _world(3, lengths, origins)
    got = boundaries.reference_bounds(origins, lengths, tracks, rows, W)
    assert got.dtype == boundaries.BOUND_DTYPE and got.dtype.itemsize == 40 and len(got) == sum(len(q) for q in rows)
    at = 0
    for r in range(len(lengths)):
        for q in rows[r]:
            want = _loop_bounds(origins[r], lengths[r], tracks[r], q, W)
            assert tuple(int(x) for x in got[at]) == want, (r, q, got[at], want)
            at += 1
    assert (got["lead"] > 0).any() == (W > 0) and (got["trail"] > 0).any() == (W > 0) and (got["runs"] > 1).any()
    assert (got["hits"] == 0).any() and (got["first"] == -1).any()


def _loop_hist(origins, lengths, rows, bounds, need, C, W):
    frag, edge, tally = np.zeros((C, 17), np.int64), np.zeros((C, 2, 2 * W + 1), np.int64), np.zeros((C, 2), np.int64)
    flag, at = 0, 0
    for r in range(len(lengths)):
        o, n = origins[r], lengths[r]
        for q in rows[r]:
            b, nd = bounds[at], int(need[at])
            at += 1
            a, e = min(max(int(q["start"]), o), o + n), min(max(int(q["end"]), o), o + n)
            if e <= a:
                continue
            L = int(q["label"])
            if not 0 <= L < C:
                flag = 1
                continue
            frag[L, min(int(b["runs"]), 16)] += 1
            if not (nd > 0 and int(b["hits"]) >= nd):
                continue
            ds = min(int(b["first"]) - a, W) if int(b["first"]) > a else -int(b["lead"])
            de = -min(e - 1 - int(b["last"]), W) if int(b["last"]) + 1 < e else int(b["trail"])
            tally[L, 0] += 1
            cut_s, cut_e = int(q["start"]) < o, int(q["end"]) > o + n
            if not cut_s:
                edge[L, 0, ds + W] += 1
            if not cut_e:
                edge[L, 1, de + W] += 1
            if not cut_s and not cut_e and ds == 0 and de == 0:
                tally[L, 1] += 1
    return frag, edge, tally, flag


@pytest.mark.parametrize("C,W", [(4, 0), (4, 1), (4, 5), (3, 200), (2, 4096)])
def test_reference_bound_hist_against_a_loop_per_row(C, W):
    from deepgrp_amd import boundaries
    from deepgrp_amd.curves import need_of
    lengths, origins = [97, 1, 40, 2], [1000, 5, 0, 77]
    tracks, rows = _world(4, lengths, origins)
    bounds = boundaries.reference_bounds(origins, lengths, tracks, rows, W)
    clen = np.concatenate([np.clip(q["end"], o, o + n) - np.clip(q["start"], o, o + n) for q, o, n in zip(rows, origins, lengths)])
    need = need_of(0.5, np.maximum(clen, 0))
    need[::7] = 0                                                           # need 0: never found
    got = boundaries.reference_bound_hist(origins, lengths, rows, bounds, need, C, W)
    want = _loop_hist(origins, lengths, rows, bounds, need, C, W)
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    assert got[3] == want[3] == (1 if C < 4 else 0)
    frag, edge, tally = got[:3]
    assert tally[:, 0].sum() > 0 and frag.sum() > tally[:, 0].sum()                                                 # rows that are not found
    assert C < 4 or (edge[:, 0].sum() < tally[:, 0].sum() and edge[:, 1].sum() < tally[:, 0].sum())                 # clipped sides
    assert (edge.sum(axis=2) <= tally[:, :1]).all() and (tally[:, 1] <= tally[:, 0]).all()


def test_the_offset_rule_at_its_corners():
    """ds / de at -W, -1, 0, 1 and W on one track: the row [100, 120) of label 1, W = 4."""
    from deepgrp_amd import boundaries
    W, o, n = 4, 50, 200
    row = [_segs([(100, 120, 1)])]

    def offsets(lo, hi):
        t = np.zeros(n, np.int8)
        t[lo - o:hi - o] = 1
        b = boundaries.reference_bounds([o], [n], [t], row, W)
        ds, de = boundaries.offsets_of(b, np.array([100]), np.array([120]), W)
        frag, edge, tally, flag = boundaries.reference_bound_hist([o], [n], row, b, np.array([1]), 2, W)
        assert flag == 0 and frag[1, 1] == 1 and tally[1, 0] == 1 and edge[1, 0, int(ds[0]) + W] == 1 and edge[1, 1, int(de[0]) + W] == 1
        assert tally[1, 1] == int(ds[0] == 0 and de[0] == 0)
        return int(ds[0]), int(de[0])
    assert offsets(100, 120) == (0, 0)
    assert offsets(101, 119) == (1, -1)
    assert offsets(99, 121) == (-1, 1)
    assert offsets(104, 116) == (4, -4) and offsets(110, 111) == (4, -4)        # W or more
    assert offsets(96, 124) == (-4, 4) and offsets(60, 200) == (-4, 4)          # W or more
    assert offsets(97, 122) == (-3, 2)


def test_a_side_the_record_clipped_is_not_counted():
    from deepgrp_amd import boundaries
    t = np.ones(30, np.int8)
    rows = [_segs([(90, 110, 1), (120, 140, 1), (90, 140, 1), (100, 130, 1)])]
    b = boundaries.reference_bounds([100], [30], [t], rows, 8)
    frag, edge, tally, flag = boundaries.reference_bound_hist([100], [30], rows, b, np.array([1, 1, 1, 1]), 2, 8)
    assert tally[1].tolist() == [4, 1] and edge[1, 0].sum() == 2 and edge[1, 1].sum() == 2 and frag[1, 1] == 4
    assert edge[1, 1, 8 + 8] == 1 and edge[1, 0, 8 - 8] == 1 and edge[1, 0, 8] == 1 and edge[1, 1, 8] == 1     # the record's own ends: no flank


# ------------------------------------------------------------------------- --boundary_join
def test_join_at_the_gap_and_on_nested_rows_and_other_labels():
    from deepgrp_amd import boundaries
    G = 3
    rows = _segs([(100, 200, 1), (200 + G - 1, 300, 1),                       # gap G - 1: one unit
                  (400, 500, 1), (500 + G, 600, 1),                           # gap G: one unit
                  (700, 800, 1), (800 + G + 1, 900, 1),                       # gap G + 1: two
                  (1000, 2000, 2), (1100, 1200, 2), (1990, 2100, 2), (2100, 2150, 2),      # nested, overlapping, abutting
                  (2101, 2160, 3),                                            # another label between them: its own unit
                  (2160 + G, 2170, 2)])
    want = [(100, 300, 1), (400, 600, 1), (700, 800, 1), (800 + G + 1, 900, 1), (1000, 2150, 2), (2160 + G, 2170, 2), (2101, 2160, 3)]
    for order in (np.arange(len(rows)), np.arange(len(rows))[::-1], np.random.default_rng(1).permutation(len(rows))):
        got = boundaries.join_rows(rows[order], G)
        assert got.dtype == SEG and [(int(q["start"]), int(q["end"]), int(q["label"])) for q in got] == want
    zero = boundaries.join_rows(_segs([(10, 20, 1), (20, 30, 1), (31, 40, 1), (5, 12, 2)]), 0)
    assert [(int(q["start"]), int(q["end"]), int(q["label"])) for q in zero] == [(10, 30, 1), (31, 40, 1), (5, 12, 2)]
    assert len(boundaries.join_rows(rows[:0], 5)) == 0 and boundaries.join_rows(rows[:1], 5).tobytes() == rows[:1].tobytes()
    bd = boundaries.Boundaries(4, 10)
    assert bd.units(rows) is rows and len(boundaries.Boundaries(4, 10, 0).units(rows)) == 9
    nested_long_first = boundaries.join_rows(_segs([(0, 1000, 1), (10, 20, 1), (1001, 1002, 1)]), 0)     # the largest end so far, not the last row's
    assert [(int(q["start"]), int(q["end"])) for q in nested_long_first] == [(0, 1000), (1001, 1002)]


# ------------------------------------------------------------------------- the files and the JSON, from fixed counts
def _fixed(W=3):
    bd_edge = np.zeros((2, 3, 2, 2 * W + 1), np.int64)
    bd_edge[0, 1, 0] = [1, 0, 0, 4, 2, 0, 1]
    bd_edge[0, 1, 1] = [0, 0, 3, 3, 0, 0, 0]
    bd_edge[1, 2, 0] = [0, 0, 0, 5, 0, 0, 0]
    bd_edge[1, 2, 1] = [2, 0, 0, 0, 0, 0, 2]
    frag = np.zeros((2, 3, 17), np.int64)
    frag[0, 1, [0, 1, 2, 16]] = [2, 5, 2, 1]
    frag[1, 2, [1]] = [5]
    tally = np.zeros((2, 3, 2), np.int64)
    tally[0, 1], tally[1, 2] = [8, 2], [5, 0]
    return bd_edge, frag, tally


def test_the_edge_file_byte_for_byte():
    from deepgrp_amd import boundaries
    edge, _frag, _tally = _fixed()
    text = boundaries.boundaries_tsv(edge, 3)
    head, body = text.split("\n", 1)
    assert head.startswith("# offset: ") and "+-3 stands for 3 or more" in head and "min_overlap" in head and "one unit" not in head
    assert body == ("view\tclass\tside\toffset\tcount\tshare\n"
                    "element\t1\tstart\t-3\t1\t0.125000\n" "element\t1\tstart\t0\t4\t0.500000\n" "element\t1\tstart\t1\t2\t0.250000\n"
                    "element\t1\tstart\t3\t1\t0.125000\n"
                    "element\t1\tend\t-1\t3\t0.500000\n" "element\t1\tend\t0\t3\t0.500000\n"
                    "row\t2\tstart\t0\t5\t1.000000\n"
                    "row\t2\tend\t-3\t2\t0.500000\n" "row\t2\tend\t3\t2\t0.500000\n")
    joined = boundaries.boundaries_tsv(edge, 3, 0).split("\n", 1)
    assert "at most 0 bases apart are one unit" in joined[0] and joined[1] == body


def test_the_fragment_file_byte_for_byte():
    from deepgrp_amd import boundaries
    _edge, frag, _tally = _fixed()
    lines = boundaries.fragments_tsv(frag).split("\n")
    assert lines[0] == "view\tclass\truns\tcount\tshare" and lines[-1] == "" and len(lines) == 1 + 2 * 2 * 17 + 1
    assert lines[1:4] == ["element\t1\t0\t2\t0.200000", "element\t1\t1\t5\t0.500000", "element\t1\t2\t2\t0.200000"]
    assert lines[4] == "element\t1\t3\t0\t0.000000" and lines[17] == "element\t1\t16+\t1\t0.100000"
    assert lines[18] == "element\t2\t0\t0\tnan" and lines[1 + 3 * 17 + 1] == "row\t2\t1\t5\t1.000000"


def test_the_json_figures():
    from deepgrp_amd import boundaries
    W = 12
    bd = boundaries.Boundaries(3, W, 5)
    edge = np.zeros((3, 2, 2 * W + 1), np.int64)
    edge[1, 0, [W - 12, W - 10, W, W + 2, W + 11]] = [1, 1, 3, 2, 1]           # |offset|: 0 0 0 2 2 10 11 12 -> the median of 8 is (2 + 2) / 2
    edge[1, 1, [W, W + 4]] = [1, 1]                                             # an even count with different middles: (0 + 4) / 2
    edge[2, 0, [W - 1, W, W + 6]] = [1, 1, 1]                                   # an odd count
    frag = np.zeros((3, 17), np.int64)
    frag[1, [0, 1, 3, 16]] = [1, 6, 2, 1]
    tally = np.array([[0, 0], [9, 1], [3, 0]])
    bd.count(0, frag, edge, tally)
    bd.count(0, frag * 0, edge * 0, tally * 0)
    s = bd.summary()
    json.dumps(s, allow_nan=False)
    assert sorted(s) == ["join", "max", "views"] and s["max"] == W and s["join"] == 5 and sorted(s["views"]) == ["element", "row"]
    c1 = s["views"]["element"][1]
    assert c1["found"] == 9 and c1["exact_start"] == 3 and c1["exact_end"] == 1 and c1["exact_both"] == 1
    assert c1["start_rows"] == 8 and c1["end_rows"] == 2
    assert c1["within_10_start"] == 6 and c1["within_10_end"] == 2
    assert c1["median_abs_start"] == 2.0 and c1["median_abs_end"] == 2.0
    assert c1["rows"] == 10 and c1["mean_runs"] == (6 + 6 + 16) / 10 and c1["share_runs_ge_2"] == 0.3
    c2 = s["views"]["element"][2]
    assert c2["median_abs_start"] == 1.0 and c2["median_abs_end"] is None and c2["mean_runs"] is None and c2["share_runs_ge_2"] is None
    assert s["views"]["row"][1]["found"] == 0 and s["views"]["row"][1]["median_abs_start"] is None
    narrow = boundaries.Boundaries(2, 10).summary()["views"]["row"][1]
    assert narrow["within_10_start"] is None and narrow["within_10_end"] is None       # +-10 stands for more: the figure cannot be had


def test_write_stages_both_files(tmp_path):
    import logging

    from deepgrp_amd import boundaries
    edge, frag, tally = _fixed()
    bd = boundaries.Boundaries(3, 3)
    for v in (0, 1):
        bd.count(v, frag[v], edge[v], tally[v])
    p = boundaries.BoundaryPlan(str(tmp_path / "run"), 3, None, str(tmp_path / "run.boundaries.tsv"), str(tmp_path / "run.fragments.tsv"))
    bd.write(p, logging.getLogger("test"))
    assert sorted(os.listdir(tmp_path)) == ["run.boundaries.tsv", "run.fragments.tsv"]
    assert (tmp_path / "run.boundaries.tsv").read_text() == boundaries.boundaries_tsv(edge, 3)
    assert (tmp_path / "run.fragments.tsv").read_text() == boundaries.fragments_tsv(frag)


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
    (["--boundary_max", "50"], ["--boundary_max needs --boundaries"], None),
    (["--boundary_join", "0"], ["--boundary_join needs --boundaries"], None),
    (["--boundaries", "run", "--boundary_max", "0"], ["--boundary_max", "1..4096", "not 0"], None),
    (["--boundaries", "run", "--boundary_max", "4097"], ["--boundary_max", "1..4096", "not 4097"], None),
    (["--boundaries", "run", "--boundary_join", "-1"], ["--boundary_join", "0 or more", "not -1"], None),
    (["--boundaries", "sub/"], ["--boundaries", "prefix", "directory"], None),
    (["--boundaries", "sub"], ["--boundaries", "prefix", "directory"], None),
    (["--boundaries", "missing_dir/run"], ["--boundaries", "missing_dir", "does not exist"], None),
    (["--boundaries", "run"], ["WORLD_SIZE"], {"WORLD_SIZE": "2"}),               # (evaluate's own refusal comes first)
])
def test_refusals_come_before_the_model_is_read(monkeypatch, tmp_path, flags, words, env):
    (tmp_path / "sub").mkdir()
    said = _refused(monkeypatch, tmp_path, flags, env=env)
    assert all(w in said for w in words), said
    assert sorted(os.listdir(tmp_path)) == ["rm.out", "sub"]


def test_an_output_that_is_an_input_is_refused(monkeypatch, tmp_path):
    ann = tmp_path / "rm.out"
    ann.write_bytes(rm_cases.text([rm_cases.out_line()]))
    os.symlink(str(ann), str(tmp_path / "a.fragments.tsv"))
    said = _refused(monkeypatch, tmp_path, ["--boundaries", "a"], ann=ann)
    assert "--boundaries" in said and "overwrite" in said and "rm.out" in said
    table = tmp_path / "b.boundaries.tsv"                                         # the table form is taken: here it is the output itself
    table.write_text("chr1\t0\t10\t1\n")
    said = _refused(monkeypatch, tmp_path, ["--boundaries", "b"], ann=table)
    assert "--boundaries" in said and "overwrite" in said and "b.boundaries.tsv" in said


def test_the_flags_belong_to_evaluate(monkeypatch, tmp_path):
    from deepgrp_amd import boundaries
    from deepgrp_amd.__main__ import CommandLineParser
    args = CommandLineParser().parse_args(["evaluate", "m.h5", "a.out", "a.fa"]).args
    assert args.boundaries is None and args.boundary_max is None and args.boundary_join is None and boundaries.plan(args) is None
    args = CommandLineParser().parse_args(["evaluate", "m.h5", "a.bed", "a.fa", "--boundaries", str(tmp_path / "run")]).args
    p = boundaries.plan(args)
    assert p.W == 200 and p.join is None and p.edges_path.endswith("run.boundaries.tsv") and p.fragments_path.endswith("run.fragments.tsv")
    args = CommandLineParser().parse_args(["evaluate", "m.h5", "a.bed", "a.fa", "--boundaries", str(tmp_path / "run"), "--boundary_max", "4096",
                                           "--boundary_join", "0"]).args
    p = boundaries.plan(args)
    assert p.W == 4096 and p.join == 0
    monkeypatch.setenv("WORLD_SIZE", "2")                                         # the plan's own refusal, for a caller other than the command
    with pytest.raises(SystemExit) as e:
        boundaries.plan(args)
    assert "--boundaries" in str(e.value) and "WORLD_SIZE" in str(e.value)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        CommandLineParser().parse_args(["predict", "m.h5", "a.fa", "--boundaries", "x"])
    with pytest.raises(ValueError):
        boundaries.Boundaries(5, 4097)


# ------------------------------------------------------------------------- the entries, without a GPU
def test_symbols_are_declared_bound_and_exported():
    from deepgrp_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    for name in ("dgrp_row_bounds_batch", "dgrp_row_bounds_workspace_bytes", "dgrp_bound_hist_batch", "dgrp_bound_hist_workspace_bytes"):
        assert f" {name}(" in header and name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name) is not None
    L = _lib.lib()
    assert L.dgrp_abi_version() == 1 and "#define DGRP_ABI_VERSION 1" in header          # an addition: the version stays
    assert "} dgrp_row_bound;" in header
    for nrec, rows in ((1, 1), (3, 5000), (40, 10 ** 6)):                       # the eval workspace and eight bytes per row for the flanks
        extra = L.dgrp_row_bounds_workspace_bytes(nrec, rows) - L.dgrp_eval_workspace_bytes(nrec, rows)
        assert 8 * rows <= extra < 8 * rows + 256
    assert L.dgrp_row_bounds_workspace_bytes(-1, 0) == 0 and L.dgrp_bound_hist_workspace_bytes(-1) == 0
    assert L.dgrp_bound_hist_workspace_bytes(10) >= 31 * 8
