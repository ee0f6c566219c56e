"""`evaluate` on the GPU: dgrp_paint_rows_batch and dgrp_row_hits_batch against a numpy brute force (explicit min over rows, hits
by cumsum), and the command line against an independent composition -- `python -m deepgrp_amd predict` in a child process, its TSV
rows painted in numpy, the truth of preprocessing.preprocess_y, a numpy confusion matrix, prediction._calculate_metrics and
element counts by loops."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
NONE = 1000


# ---------------------------------------------------------------- brute force
def brute_paint(buf, off, ln, org, rows_per_rec):
    out = buf.copy()
    for r in range(len(ln)):
        best = np.full(ln[r], NONE, np.int64)
        for s, e, lab in rows_per_rec[r]:
            a, b = max(s - org[r], 0), min(e - org[r], ln[r])
            if b > a:
                best[a:b] = np.minimum(best[a:b], lab)
        seg = out[off[r]:off[r] + ln[r]]
        seg[best < NONE] = best[best < NONE]
    return out


def brute_hits(buf, off, ln, org, rows_per_rec):
    out = []
    for r in range(len(ln)):
        rec = buf[off[r]:off[r] + ln[r]].astype(np.int64)
        rows = np.array(rows_per_rec[r], np.int64).reshape(-1, 3)
        h = np.zeros(len(rows), np.int64)
        for lab in np.unique(rows[:, 2]):
            cs = np.concatenate([[0], np.cumsum(rec == lab)])
            sel = rows[:, 2] == lab
            a = np.clip(rows[sel, 0] - org[r], 0, ln[r])
            b = np.clip(rows[sel, 1] - org[r], 0, ln[r])
            h[sel] = np.where(b > a, cs[np.maximum(a, b)] - cs[a], 0)
        out.append(h)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


# ---------------------------------------------------------------- the kernels
def _call(kind, buf, off, ln, org, rows_per_rec):
    """-> (return code, buffer after the call, hits or None)"""
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    nrec = len(ln)
    ro = np.zeros(nrec + 1, np.int64)
    np.cumsum([len(x) for x in rows_per_rec], out=ro[1:])
    flat = np.zeros(int(ro[-1]), SEG)
    if flat.size:
        allr = np.array([x for rr in rows_per_rec for x in rr], np.int64).reshape(-1, 3)
        flat["start"], flat["end"], flat["label"] = allr[:, 0], allr[:, 1], allr[:, 2]
    d_rows = torch.from_numpy(flat.view(np.uint8)).to(dev) if flat.size else None
    d_buf = torch.from_numpy(buf.copy()).to(dev)
    wb = L.dgrp_eval_workspace_bytes(nrec, int(ro[-1]))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    o, n, g = (np.ascontiguousarray(x, np.int64) for x in (off, ln, org))
    rp = d_rows.data_ptr() if d_rows is not None else None
    if kind == "paint":
        rc = L.dgrp_paint_rows_batch(d_buf.data_ptr(), nrec, o.ctypes.data, n.ctypes.data, g.ctypes.data, rp, ro.ctypes.data,
                                     work.data_ptr(), wb, stream_ptr())
        hits = None
    else:
        d_hits = torch.full((max(int(ro[-1]), 1),), -5, dtype=torch.int64, device=dev)
        rc = L.dgrp_row_hits_batch(d_buf.data_ptr(), nrec, o.ctypes.data, n.ctypes.data, g.ctypes.data, rp, ro.ctypes.data,
                                   d_hits.data_ptr(), work.data_ptr(), wb, stream_ptr())
        hits = d_hits.cpu().numpy()[:int(ro[-1])]
    torch.cuda.synchronize()
    return rc, d_buf.cpu().numpy(), hits


LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 1_000_003]


def _rows_for(rng, n, o, many=False):
    rows = []
    lab = lambda: int(rng.integers(1, 5)) if rng.random() < 0.8 else int(rng.integers(1, 128))
    for _ in range(int(rng.integers(0, 40))):                            # overlapping, any class
        s = int(rng.integers(max(o - 60, 0), o + n + 60))
        rows.append((s, s + int(rng.integers(0, min(n, 5000) + 2)), lab()))
    if n > 100:                                                          # nested, same class and other classes
        s = o + int(rng.integers(0, n // 2))
        e = s + int(rng.integers(30, n - (s - o) + 1))
        rows += [(s, e, 3), (s + 5, e - 5, 1), (s + 7, e - 9, 3), (s + 8, s + 8 + (e - s) // 3, 2)]
    rows += [(o + n // 2, o + n // 2, 1), (o, o, 2)]                      # zero length
    rows += [(max(o - 30, 0), o + min(n, 7), 4), (o + n - min(n, 9), o + n + 25, 2), (0, o + n + 5000, 5)]   # clipped at each end
    rows += [(o + n, o + n + 50, 1), (o + n + 10, o + n + 11, 2)]        # entirely outside
    if o > 3:
        rows.append((0, o - 1, 1))
    if n >= 1_000_000:
        rows.append((o + 1, o + 1_000_001, 6))                           # one megabase
        if many:
            s = o + rng.integers(0, n - 300, 100_000)
            e = s + rng.integers(10, 301, s.size)
            lb = rng.integers(1, 5, s.size)
            rows += list(zip(s.tolist(), e.tolist(), lb.tolist()))
    order = rng.permutation(len(rows))
    return [rows[k] for k in order]


def _case(seed):
    rng = np.random.default_rng(seed)
    nrec = int(rng.integers(1, 8))
    ln = [int(rng.choice(LENGTHS[:-1])) for _ in range(nrec)]
    if seed % 3 == 0:
        ln[int(rng.integers(0, nrec))] = LENGTHS[-1]
    org = [int(rng.integers(0, 5000)) if rng.random() < 0.7 else 0 for _ in range(nrec)]
    gaps = [int(rng.integers(0, 40)) for _ in range(nrec)]                # bytes nobody may write between records
    off, p = [], 7
    for r in range(nrec):
        off.append(p)
        p += ln[r] + gaps[r]
    buf = rng.integers(-128, 0, p + 11).astype(np.int8)                   # sentinel: no valid label
    rows = [_rows_for(rng, ln[r], org[r], many=(seed % 6 == 0)) for r in range(nrec)]
    return buf, off, ln, org, rows


@pytest.mark.parametrize("seed", range(14))
def test_paint_kernel_vs_brute_force(seed):
    buf, off, ln, org, rows = _case(seed)
    rc, got, _ = _call("paint", buf, off, ln, org, rows)
    assert rc == 0
    want = brute_paint(buf, off, ln, org, rows)
    np.testing.assert_array_equal(got, want)
    rc2, again, _ = _call("paint", buf, off, ln, org, rows)
    assert rc2 == 0 and np.array_equal(again, got)                        # deterministic


@pytest.mark.parametrize("seed", range(14))
def test_hits_kernel_vs_brute_force(seed):
    buf, off, ln, org, rows = _case(seed + 100)
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 6, buf.size).astype(np.int8)
    if seed % 2:
        buf = brute_paint(np.zeros_like(buf), off, ln, org, rows)         # the truth of the rows themselves
    rc, after, hits = _call("hits", buf, off, ln, org, rows)
    assert rc == 0 and np.array_equal(after, buf)
    np.testing.assert_array_equal(hits, brute_hits(buf, off, ln, org, rows))


@pytest.mark.parametrize("bad", [(-1, 5, 1), (9, 8, 1), (2, 9, 0), (2, 9, 128), (2, 9, -3)])
def test_bad_rows_are_refused_before_any_write(bad):
    from deepgrp_amd._lib import lib
    rng = np.random.default_rng(5)
    buf = rng.integers(-128, 0, 5000).astype(np.int8)
    rows = [[(0, 100, 1), (10, 20, 2)], [(3, 50, 1), bad, (7, 9, 4)]]
    for kind in ("paint", "hits"):
        rc, got, _ = _call(kind, buf, [0, 2000], [1500, 2500], [0, 3], rows)
        assert rc == -1
        assert np.array_equal(got, buf)
        assert "row 3" in lib().dgrp_last_error().decode()


@pytest.mark.parametrize("seed", range(3))
def test_slices_crossing_thousands_of_rows(seed):
    """More than 2048 rows inside one 8192-position slice (1-3 bp rows, and zero-length or wholly outside rows, which share one
    position of the scan): the hit counts go straight to d_hits instead of through the LDS counters."""
    rng = np.random.default_rng(40 + seed)
    n, o = 20_000, 1000
    s = o + rng.integers(0, 7000, 3000)
    rows = list(zip(s.tolist(), (s + rng.integers(1, 4, s.size)).tolist(), rng.integers(1, 5, s.size).tolist()))
    out = o + n + rng.integers(0, 10**6, 3000)
    rows += list(zip(out.tolist(), (out + rng.integers(0, 50, out.size)).tolist(), rng.integers(1, 5, out.size).tolist()))
    rows += [(o + k, o + k, 2) for k in range(0, 3000, 3)]                            # zero length
    rows = [rows[k] for k in rng.permutation(len(rows))]      # 7000 rows of about 6000 positions: all in the first slice
    rows += [(o + 9000, o + 15000, 3), (o + 100, o + 19000, 4)]
    buf = rng.integers(-128, 0, n + 64).astype(np.int8)
    rc, got, _ = _call("paint", buf, [32], [n], [o], [rows])
    assert rc == 0
    np.testing.assert_array_equal(got, brute_paint(buf, [32], [n], [o], [rows]))
    labels = rng.integers(0, 5, buf.size).astype(np.int8) if seed else got
    rc, _after, hits = _call("hits", labels, [32], [n], [o], [rows])
    assert rc == 0
    np.testing.assert_array_equal(hits, brute_hits(labels, [32], [n], [o], [rows]))


def test_no_rows_and_empty_records():
    buf = np.full(64, -9, np.int8)
    for kind in ("paint", "hits"):
        rc, got, hits = _call(kind, buf, [0, 10, 10], [10, 0, 20], [0, 0, 4], [[], [], []])
        assert rc == 0 and np.array_equal(got, buf)
        rc, got, hits = _call(kind, buf, [0, 10, 10], [10, 0, 20], [0, 0, 4], [[], [(0, 99, 3)], []])
        assert rc == 0 and np.array_equal(got, buf)
        if kind == "hits":
            assert hits.tolist() == [0]


# ---------------------------------------------------------------- the command line against an independent composition
def _write_fasta(path, records):
    with open(path, "wb") as fh:
        for header, seq in records:
            fh.write(b">" + header.encode() + b"\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")


def _compose(flags, model, fasta, records, ann_path, classes, theta, tmp_path):
    """What `evaluate` must report, composed from `predict`'s TSV written by a child process."""
    from deepgrp_amd.prediction import _calculate_metrics
    from deepgrp_amd.preprocessing import preprocess_y
    out = tmp_path / "pred.tsv"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    top = [f for f in flags if f != "-m"]
    fasta = [fasta] if isinstance(fasta, str) else list(fasta)
    subprocess.run([sys.executable, "-m", "deepgrp_amd"] + top + ["predict", model] + fasta + ["--output", str(out)] +
                   (["-m"] if "-m" in flags else []), check=True, cwd=ROOT, env=env, timeout=900)
    rows = {}
    for line in open(out):
        f = line.rstrip("\n").split("\t")
        rows.setdefault(f[1], []).append((int(f[2]), int(f[3]), int(f[4])))
    repeats = list(range(1, classes))
    cnf = np.zeros((classes, classes), np.int64)
    el, fo, sg, su = (np.zeros(classes, np.int64) for _ in range(4))
    bases = used = outside = annotated = 0
    ann_names = {l.split()[0] for l in open(ann_path) if l.strip() and not l.startswith("#")}
    for rec in records:                          # (TSV header, sequence) or (TSV header, annotation name, sequence)
        header, name, seq = rec if len(rec) == 3 else (rec[0], rec[0].split()[0], rec[1])
        a = np.frombuffer(seq, np.uint8)
        nonn = np.flatnonzero(a != ord("N"))
        st, en = int(nonn[0]), int(nonn[-1]) + 1
        pred = np.zeros(en - st, np.int64)
        prow = rows.get(header, [])
        for s, e, lab in prow:
            pred[s - st:e - st] = lab
        truth = preprocess_y(ann_path, name, len(seq), repeats).argmax(axis=0)[st:en].astype(np.int64)
        np.add.at(cnf, (truth, pred), 1)
        bases += en - st
        mine = []
        if name in ann_names:
            for l in open(ann_path):
                c = l.split()
                if c and not c[0].startswith("#") and c[0] == name and int(c[3]) in repeats:
                    mine.append((int(c[1]), int(c[2]), int(c[3])))
        used += len(mine)
        annotated += bool(mine)
        for s, e, lab in mine:
            a0, b0 = max(s, st) - st, min(e, en) - st
            if b0 <= a0:
                outside += 1
                continue
            el[lab] += 1
            fo[lab] += int((pred[a0:b0] == lab).sum()) >= theta * (b0 - a0)
        for s, e, lab in prow:
            sg[lab] += 1
            su[lab] += int((truth[s - st:e - st] == lab).sum()) >= theta * (e - s)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = _calculate_metrics(cnf)
    m["TotalACC"] = np.trace(cnf) / bases
    return dict(cnf=cnf, metrics=m, elements=el, found=fo, segments=sg, supported=su, bases=bases, rows_used=used, outside=outside,
                records=len(records), records_annotated=annotated)


def _same(got, want):
    w = np.asarray(want, float).ravel()
    g = got if isinstance(got, list) else [got]
    assert len(g) == w.size
    for x, y in zip(g, w):
        assert (x is None and math.isnan(y)) or x == float(y), (got, want)


def _check(js, tsv_path, want, classes):
    assert js["confusion_matrix"] == want["cnf"].tolist()
    for k in ("bases", "rows_used", "outside", "records", "records_annotated"):
        assert js[k] == want[k], k
    for k in ("elements", "found", "segments", "supported"):
        assert js[k] == want[k].tolist(), k
    for k, v in want["metrics"].items():
        _same(js["metrics"][k], v)
    assert int(np.sum(js["confusion_matrix"])) == js["bases"]
    lines = open(tsv_path).read().splitlines()
    assert len(lines) == classes + 3
    cnf = want["cnf"]
    for c in range(classes):
        f = lines[1 + c].split("\t")
        assert int(f[1]) == cnf[c].sum() and int(f[2]) == cnf[:, c].sum() and int(f[3]) == cnf[c, c]
        assert f[6:9] == [repr(float(want["metrics"][k][c])) for k in ("TPR", "PPV", "F1")]
        assert [int(x) for x in f[9:]] == [int(want[k][c]) for k in ("elements", "found", "segments", "supported")]
    assert lines[-2] == "#TotalACC\t" + repr(float(want["metrics"]["TotalACC"]))
    assert lines[-1] == "#MCC\t" + repr(float(want["metrics"]["MCC"]))


def _synthetic_model(tmp_path):
    from deepgrp_amd import model as dgmodel, synthetic
    w = synthetic.trained_weights()
    path = str(tmp_path / "synth.hdf5")
    dgmodel.save_keras_hdf5(path, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    return path


def _three_records(tmp_path):
    from deepgrp_amd import synthetic
    recs, lines = [], []
    for k, (n, fl) in enumerate(((240_000, 3000), (160_000, 1500), (90_000, 800))):
        seq = synthetic.synthetic_chromosome(n, contig=10 + k, flank=fl)
        header = f"chr{k + 1}" + (" assembled by hand" if k == 0 else "")
        recs.append((header, seq))
        if k < 2:
            lines += synthetic.synthetic_annotation(n, contig=10 + k, name=f"chr{k + 1}", flank=fl)
            rng = np.random.default_rng(k)
            for _ in range(12):                                   # overlapping rows of another class
                s = int(rng.integers(fl, n - fl - 5000))
                lines.append(f"chr{k + 1}\t{s}\t{s + int(rng.integers(50, 4000))}\t{int(rng.integers(1, 5))}\tx\ty\n")
            lines.append(f"chr{k + 1}\t{fl // 4}\t{fl // 2}\t2\tinN\tflank\n")       # inside the N flank: outside
            lines.append(f"chr{k + 1}\t{n - fl // 2}\t{n - fl // 4}\t1\tinN\tflank\n")
            lines.append(f"chr{k + 1}\t{fl - 20}\t{fl + 30}\t3\tedge\tflank\n")     # clipped by the first non-N base
    lines.append("chrUn\t10\t500\t1\tx\ty\n")                      # a contig no record has
    fa = tmp_path / "three.fa"
    _write_fasta(fa, recs)
    ann = tmp_path / "three.bed"
    ann.write_text("# synthetic truth\n" + "".join(lines))
    return str(fa), recs, str(ann)


@pytest.mark.parametrize("which,flags", [("synthetic", []), ("synthetic", ["-m"]), ("golden", []), ("golden", ["-s", "60", "-m"])])
def test_cli_three_records_vs_composition(tmp_path, which, flags):
    from deepgrp_amd.__main__ import main
    model = _synthetic_model(tmp_path) if which == "synthetic" else os.path.join(GOLDEN, "model_u60_T342_att.h5")
    fa, recs, ann = _three_records(tmp_path)
    theta = 0.5 if which == "synthetic" else 0.3
    top = [f for f in flags if f != "-m"]
    main(top + ["evaluate", model, ann, fa, "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json"),
                "--min_overlap", str(theta)] + (["-m"] if "-m" in flags else []))
    js = json.load(open(tmp_path / "r.json"))
    want = _compose(flags, model, fa, recs, ann, 5, theta, tmp_path)
    assert js["records"] == 3 and js["records_annotated"] == 2 and js["outside"] == 4
    assert js["repeats"] == [1, 2, 3, 4] and js["classes"] == 5 and js["min_overlap"] == theta
    _check(js, tmp_path / "r.tsv", want, 5)
    if which == "synthetic" and not flags:
        assert js["metrics"]["MCC"] > 0                          # the trained model finds planted repeats


def test_cli_no_matching_record_exits(tmp_path, caplog):
    from deepgrp_amd.__main__ import main
    fa, _recs, _ann = _three_records(tmp_path)
    ann = tmp_path / "other.bed"
    ann.write_text("1\t10\t500\t1\n2\t10\t50\t2\n")
    with pytest.raises(SystemExit) as e:
        main(["evaluate", os.path.join(GOLDEN, "model_u60_T342_att.h5"), str(ann), fa])
    msg = str(e.value.code)
    assert "'chr1'" in msg and "'1'" in msg
    # warned as the first record was read, long before the end of the run
    warned = [r.getMessage() for r in caplog.records if r.levelname == "WARNING" and "no annotation rows" in r.getMessage()]
    assert len(warned) == 1 and "'chr1'" in warned[0] and "'1'" in warned[0]


def test_cli_batch_path_vs_composition(tmp_path, monkeypatch):
    """About 300 records of 2-20 kb: they go through dgrp_predict_batch, several records per flat buffer."""
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.runner import SMALL_RECORD
    n = 3_600_000
    seq = synthetic.synthetic_chromosome(n, contig=21, flank=0)
    _idx, lab = synthetic.synthetic_truth(n, contig=21, flank=0)
    rng = np.random.default_rng(9)
    recs, lines, p, k = [], [], 0, 0
    while p < n - 20_000 and k < 300:
        ln = int(rng.integers(2000, 20_001))
        piece, truth = seq[p:p + ln], lab[p:p + ln]
        lead, trail = (int(rng.integers(0, 300)), int(rng.integers(0, 300))) if k % 3 == 0 else (0, 0)
        piece = b"N" * lead + piece + b"N" * trail
        name = f"ctg{k}"
        recs.append((name, piece))
        edge = np.flatnonzero(np.diff(truth.astype(np.int16), prepend=0, append=0))
        for b, e in zip(edge[:-1], edge[1:]):
            if truth[b]:
                lines.append(f"{name}\t{b + lead}\t{e + lead}\t{int(truth[b])}\n")
        if k % 7 == 0:
            lines.append(f"{name}\t0\t{lead + 100}\t{int(rng.integers(1, 5))}\n")
        p += ln
        k += 1
    assert max(len(s) for _h, s in recs) <= SMALL_RECORD
    fa = tmp_path / "many.fa"
    _write_fasta(fa, recs)
    ann = tmp_path / "many.bed"
    ann.write_text("".join(lines))
    model = _synthetic_model(tmp_path)
    from deepgrp_amd.pipeline import ContigPipeline
    batched = []
    real = ContigPipeline.run_batch

    def counting(self, d_base, offsets, *a, **k):
        assert self.batchable()
        batched.append(len(offsets))
        return real(self, d_base, offsets, *a, **k)

    monkeypatch.setattr(ContigPipeline, "run_batch", counting)
    main(["evaluate", model, str(ann), str(fa), "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json")])
    assert sum(batched) == len(recs) and max(batched) > 1             # every record went through dgrp_predict_batch, several per call
    js = json.load(open(tmp_path / "r.json"))
    want = _compose([], model, str(fa), recs, str(ann), 5, 0.5, tmp_path)
    assert js["records"] == len(recs)
    _check(js, tmp_path / "r.tsv", want, 5)


def test_cli_scale_50mbp_vs_composition(tmp_path):
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    n = 50_000_000
    seq = synthetic.synthetic_chromosome(n, contig=33, flank=10_000)
    fa = tmp_path / "big.fa"
    _write_fasta(fa, [("chrBig", seq)])
    ann = tmp_path / "big.bed"
    ann.write_text("".join(synthetic.synthetic_annotation(n, contig=33, name="chrBig", flank=10_000)))
    model = _synthetic_model(tmp_path)
    main(["evaluate", model, str(ann), str(fa), "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json")])
    js = json.load(open(tmp_path / "r.json"))
    want = _compose([], model, str(fa), [("chrBig", seq)], str(ann), 5, 0.5, tmp_path)
    _check(js, tmp_path / "r.tsv", want, 5)
    assert int(np.sum(js["confusion_matrix"])) == js["bases"] == n - 20_000


@pytest.mark.parametrize("how", ["stdin", "fifo"])
def test_cli_text_inputs_vs_composition(tmp_path, monkeypatch, how):
    """Inputs the line loop reads (standard input, a pipe such as `<(zcat chr.fa.gz)`): the records reach the runner as text and
    are uploaded by its worker on the worker's own stream, as `predict` does."""
    import threading
    from deepgrp_amd.__main__ import main
    model = _synthetic_model(tmp_path)
    fa, recs, ann = _three_records(tmp_path)
    argv = ["evaluate", model, ann, "-", "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json")]
    if how == "stdin":
        monkeypatch.setattr(sys, "stdin", open(fa, "r"))
        main(argv)
    else:
        pipe = str(tmp_path / "fifo")
        os.mkfifo(pipe)

        def feed():
            with open(pipe, "wb") as w, open(fa, "rb") as r:
                w.write(r.read())
        t = threading.Thread(target=feed)
        t.start()
        argv[3] = pipe
        main(argv)
        t.join()
    js = json.load(open(tmp_path / "r.json"))
    want = _compose([], model, fa, recs, ann, 5, 0.5, tmp_path)
    assert js["records"] == 3
    _check(js, tmp_path / "r.tsv", want, 5)


def test_cli_npz_input_named_by_file_name(tmp_path):
    """A one-hot `<name>.gz.npz` input is matched to the annotation by its file name up to the first '.'."""
    from deepgrp_amd import synthetic
    from deepgrp_amd.__main__ import main
    n, fl = 120_000, 700
    seq = synthetic.synthetic_chromosome(n, contig=51, flank=fl)
    idx = np.frombuffer(seq, np.uint8)
    code = np.full(256, 4, np.int64)
    code[[65, 67, 71, 84]] = [0, 1, 2, 3]
    fwd = np.zeros((5, n), np.int8)
    fwd[code[idx], np.arange(n)] = 1
    npz = tmp_path / "chrZ.fa.gz.npz"
    np.savez_compressed(npz, fwd=fwd)
    fa, recs, _ann = _three_records(tmp_path)
    ann = tmp_path / "z.bed"
    ann.write_text("".join(synthetic.synthetic_annotation(n, contig=51, name="chrZ", flank=fl)) +
                   "".join(synthetic.synthetic_annotation(240_000, contig=10, name="chr1", flank=3000)))
    model = _synthetic_model(tmp_path)
    main(["evaluate", model, str(ann), str(npz), fa, "--output", str(tmp_path / "r.tsv"), "--json", str(tmp_path / "r.json")])
    js = json.load(open(tmp_path / "r.json"))
    want = _compose([], model, [str(npz), fa], [("chrZ.fa.gz", "chrZ", seq)] + recs, str(ann), 5, 0.5, tmp_path)
    assert js["records"] == 4 and js["records_annotated"] == 2
    _check(js, tmp_path / "r.tsv", want, 5)
